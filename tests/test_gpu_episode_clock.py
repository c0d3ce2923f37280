"""GPU tests of per-trajectory episodes (csrc/episode_clock.hip; TrainPipeline(episodes="per_trajectory")): the boundary call
alone against its NumPy restatement (tests/episode_clock_ref.py) on canary-padded buffers, blow-ups and restarts inside the
pipeline from fixed and from random fields, the mode against the lock-stepped pipeline when nothing blows up, graphs against
eager steps, the 1-D Keller-Segel, the refusals and reset_from().

Where a test needs trajectories that blow up, its inputs were chosen with the fp64 oracle on the CPU (oracle/ks.py under three
noise streams) and the test asserts the mix itself -- at least one episode that timed out and one that was cut short."""
import ctypes as C

import numpy as np
import pytest
import torch

from episode_clock_ref import ClockModel, apply_rows, init_offset, initial_clocks

pytestmark = pytest.mark.gpu

NETS = ("behavior_actor", "behavior_critic", "target_actor", "target_critic")
CANARY = 12345.0
PAD = 64


def _setup(pkg, geom, **kw):
    if geom == "ks22":
        return pkg.KSSetup.KS22(**kw)
    if geom == "c2":
        return pkg.KSSetup.bench_C2(256, **kw)
    if geom == "kseg":
        return pkg.KellerSegelSetup(**kw)
    raise ValueError(geom)


def _make(pkg, geom, B, E, dtype=torch.float32, graphs=False, y0=None, setup_kw=None, agent_kw=None, act_noise=0.3, **kw):
    setup = _setup(pkg, geom, **(setup_kw or {}))
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    if y0 is None and geom != "kseg":
        y0 = setup.generate_random_init(np.random.default_rng(0), B) * 0.15
    env = pkg.PDEenv(setup, B=B, dtype=dtype, y0=y0, stream=s_env, autoreset=False)
    agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                             noise_seed=7, trajectory_length=1, **(agent_kw or {}))
    agent.policy.act_noise = act_noise
    torch.cuda.synchronize()
    return pkg.TrainPipeline(env, agent, lag=2, episode_steps=E, stream_env=s_env, stream_upd=s_upd, use_graphs=graphs,
                             chunks=(6, 1), noise_seed=99, **kw)


def _scaled_y0(setup, B, period=8):
    """rows of generate_random_init(default_rng(0), B), row b scaled by 0.05 (b mod period + 1)"""
    return setup.generate_random_init(np.random.default_rng(0), B) * (0.05 * (np.arange(B) % period + 1))[:, None]


def _adam(nna):
    m = nna.model
    k = sum(int(np.asarray(x).size) for x in m.params())
    a, b, bp = (C.c_float * k)(), (C.c_float * k)(), (C.c_double * 2)()
    assert m.lib.pdec_adam_get_state(m.handle, a, b, bp) == 0
    return bytes(a), bytes(b), bytes(bp)


def _same_fin(a, b):
    assert a["dropped"] == b["dropped"]
    for k in ("trajectory", "episode", "ret", "length", "blew_up", "end_step"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def _assert_mix(fin, E):
    assert (fin["length"] == E).any() and (fin["length"] < E).any(), np.bincount(fin["length"])
    assert fin["blew_up"].any() and not fin["blew_up"].all()


class _Restarts:
    """row b of env.random_init(seed, off) and of env.featurize(that field) for episode n of a pipeline's rank, drawn once per n
    on a second environment of the same setup"""

    def __init__(self, pkg, p):
        self.p = p
        self.ref = pkg.PDEenv(p.env.setup, B=p.env.B, dtype=p.env.dtype, stream=p.s_env, autoreset=False)
        self.cache = {}

    def __call__(self, n):
        if n not in self.cache:
            p, ref = self.p, self.ref
            r, W = p.init_rank
            with torch.cuda.stream(p.s_env):
                y = torch.empty_like(ref.y)
                ref.random_init(p.init_seed, init_offset(n, r, W, ref.B, ref.random_init_coefficients()), out=y)
                s = ref.featurize(y)
            torch.cuda.synchronize()
            self.cache[n] = (y, s)
        return self.cache[n]


# ---------------------------------------------------------------------------------------------------- 1. the launch alone
def _padded(shape, dtype, fill=None):
    """a tensor view with PAD canary elements in front of and behind it"""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * PAD,), CANARY, dtype=dtype, device="cuda")
    view = flat[PAD:PAD + n].view(shape)
    if fill is not None:
        view.copy_(fill)
    return flat, view


def _canaries_intact(flat):
    return bool((flat[:PAD] == CANARY).all()) and bool((flat[-PAD:] == CANARY).all())


@pytest.mark.parametrize("random_init,rank", [(True, (0, 1)), (True, (1, 3)), (False, (0, 1))])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_boundary_launch_equals_the_model(pkg, dtype, random_init, rank):
    _launch_case(pkg, pkg.KSSetup.KS22(), dtype, random_init, rank)


@pytest.mark.parametrize("kind,dtype,rank", [("ks_fd", torch.float32, (0, 1)), ("kseg", torch.float64, (1, 3)),
                                             ("kseg", torch.float32, (0, 1))])
def test_boundary_launch_on_the_other_kinds(pkg, kind, dtype, rank):
    """the finite-difference KS with a temporal stack of two, and the 1-D Keller-Segel (two species, temporal stack of two)"""
    setup = pkg.KSSetup.KS22(integrator="rk4_fd", temporal_steps=2) if kind == "ks_fd" else pkg.KellerSegelSetup()
    assert setup.temporal_steps == 2
    _launch_case(pkg, setup, dtype, True, rank)


def _launch_case(pkg, setup, dtype, random_init, rank):
    B, E, cap, seed = 5, 3, 2, 11
    L = pkg._lib
    s = torch.cuda.Stream()
    y0h = setup.generate_random_init(np.random.default_rng(4), B) if random_init is False else None
    env = pkg.PDEenv(setup, B=B, dtype=dtype, y0=y0h, stream=s, autoreset=False)
    lib = env.lib
    R, nc = setup.reward_len, env.random_init_coefficients()
    h = L.Handle()
    L.check(lib.pdec_epclock_create(C.byref(h), env.handle, E, cap, int(random_init), seed, rank[0], rank[1]))
    model = ClockModel(B, E, cap)
    rng = np.random.default_rng(9)
    npdt = np.float32 if dtype == torch.float32 else np.float64
    with torch.cuda.stream(s):
        state0 = env.featurize(env.y0)
    torch.cuda.synchronize()
    # flags per call: none, first row, last row (on the step the other clocks time out), all rows, then three quiet calls --
    # trajectory 0 ends at calls 1, 3 and 6: three ends in a ring of two slots
    pattern = [[], [0], [B - 1], list(range(B)), [], [], []]
    ends = [[], [0], [1, 2, 3, 4], list(range(B)), [], [], list(range(B))]
    drawn = {}

    def restart_rows(n):
        if not random_init:
            return env.y0, state0
        if n not in drawn:
            with torch.cuda.stream(s):
                y = torch.empty_like(env.y)
                env.random_init(seed, init_offset(n, rank[0], rank[1], B, nc), out=y)
                drawn[n] = (y, env.featurize(y))
            torch.cuda.synchronize()
        return drawn[n]

    def one_call(call, rows, expect):
        flags_h = np.zeros(B, dtype=np.int32)
        flags_h[rows] = 3 if call == 1 else 1          # (any non-zero value is a blow-up)
        host = dict(reward=-rng.uniform(0, 9, (B, R)).astype(npdt), terminal=(flags_h != 0)[:, None].repeat(R, 1).astype(npdt),
                    action=rng.uniform(-1, 1, env._ashape).astype(npdt), aprev=rng.uniform(-1, 1, env._ashape).astype(npdt),
                    y=rng.standard_normal(env._yshape).astype(npdt), state=rng.standard_normal(env._sshape).astype(npdt))
        if call == 1:
            host["reward"][0, 1], host["reward"][0, 2] = np.inf, np.nan      # a blown-up row: becomes 0
            host["reward"][2, 3] = np.nan                                    # not blown up: left alone
        with torch.cuda.stream(s):
            dev = {k: _padded(v.shape, dtype, torch.as_tensor(v)) for k, v in host.items()}
            fflat = torch.full((B + 2 * PAD,), 777, dtype=torch.int32, device="cuda")
            flags = fflat[PAD:PAD + B]
            flags.copy_(torch.as_tensor(flags_h))
            fixed = not random_init
            L.check(lib.pdec_epclock_step(h, L.ptr(dev["reward"][1]), L.ptr(flags), L.ptr(dev["terminal"][1]),
                                          L.ptr(dev["action"][1]), L.ptr(dev["aprev"][1]), L.ptr(dev["y"][1]),
                                          L.ptr(dev["state"][1]), L.ptr(env.y0) if fixed else None,
                                          L.ptr(state0) if fixed else None))
        torch.cuda.synchronize()
        want_r, ended, n = model.step(host["reward"], flags_h)
        assert np.nonzero(ended)[0].tolist() == expect, call
        new_y, new_s = np.zeros(env._yshape, npdt), np.zeros(env._sshape, npdt)
        for b in np.nonzero(ended)[0]:
            y, st = restart_rows(int(n[b]))
            new_y[b], new_s[b] = y[b].cpu().numpy(), st[b].cpu().numpy()
        want = {k: v.copy() for k, v in host.items()}
        want["reward"] = want_r
        apply_rows(ended, want["terminal"], want["action"], want["aprev"], want["y"], want["state"], new_y, new_s)
        for k, (flat, view) in dev.items():
            # every output equals the model exactly -- so nothing outside the rows of ended trajectories is written
            # (action_prev_next apart, which every trajectory writes) -- and the canaries stand
            assert np.array_equal(view.cpu().numpy(), want[k], equal_nan=True), (call, k)
            assert _canaries_intact(flat), (call, k)
        assert bool((fflat[:PAD] == 777).all()) and bool((fflat[-PAD:] == 777).all())
        assert np.array_equal(flags.cpu().numpy(), flags_h)
        cnt = np.empty(B, dtype=np.int64)
        ret, ln = np.empty((B, cap)), np.empty((B, cap), dtype=np.int32)
        blew, end = np.empty((B, cap), dtype=np.int32), np.empty((B, cap), dtype=np.int64)
        L.check(lib.pdec_epclock_read(h, L.ptr(cnt), L.ptr(ret), L.ptr(ln), L.ptr(blew), L.ptr(end)))
        for got, ref in zip((cnt, ret, ln, blew, end), (model.count,) + model.rings()):
            assert np.array_equal(got, ref, equal_nan=True), call

    try:
        for call, (rows, expect) in enumerate(zip(pattern, ends)):
            one_call(call, rows, expect)
        assert model.count[0] == 3 and model.finished()["dropped"] > 0                 # the log wrapped
        one_call(7, [], [])
        # pdec_epclock_set: clocks to the given values, the running episodes cut (len and ret back to 0), counts and logs kept:
        # trajectories 0 and 4 time out at the next call, after one step
        c0 = np.array([2, 0, 1, 0, 2], dtype=np.int32)
        L.check(lib.pdec_epclock_set(h, L.ptr(c0)))
        model.set(c0)
        one_call(8, [], [0, 4])
        assert [model.slots[b][int(model.count[b] - 1) % cap][1] for b in (0, 4)] == [1, 1]
        bad = np.array([0, 0, E, 0, 0], dtype=np.int32)
        assert lib.pdec_epclock_set(h, L.ptr(bad)) != 0 and b"clock0" in lib.pdec_last_error()
    finally:
        lib.pdec_destroy(h)


# ---------------------------------------------------------------------------------------------------- the pipeline, step by step
def _drained(p, n, model, restart_rows):
    """n eager steps, the device drained after each.  After step k the model is fed the read-back reward and flag ring slots;
    checked per step: the terminal rows, the rows of y / state of the trajectories that ended (restart_rows(b, n) -> (y row,
    state row) tensors), and that every row of pipe.y is finite and, unless it restarted in this step, inside max_value.
    (A restart field may itself exceed max_value -- rows 5 and 7 of the fixed fields below start at max|y0| = 1.72 and 1.88
    against 1.5, some Philox draws above 5.0: such a trajectory ends again after one step and restarts from the same rule.)"""
    p.drain_between = True
    max_value = float(p.env.setup.max_value)
    for _ in range(n):
        k = p.tick
        p.step()
        torch.cuda.synchronize()
        rew, flags = p.rring[k % 3].cpu().numpy(), p.fring[k % 3].cpu().numpy()
        out, ended, cnt = model.step(rew, flags)
        assert np.array_equal(out, rew, equal_nan=True)                 # (the ring slot holds the sanitised rows)
        assert ((flags != 0) <= ended).all()
        term = p.tring[k % 3].cpu().numpy()
        assert np.array_equal(term, ended[:, None].repeat(term.shape[1], 1).astype(term.dtype)), k
        y, s = p.ybuf[(k + 1) % 2], p.sring[(k + 1) % 6]
        assert y.data_ptr() == p.y.data_ptr()
        for b in np.nonzero(ended)[0]:
            wy, ws = restart_rows(int(b), int(cnt[b]))
            assert torch.equal(y[b], wy) and torch.equal(s[b], ws), (k, b)
            assert not bool(p.aprev[(k + 1) % 2][b].any())
        live = torch.as_tensor(np.nonzero(~ended)[0], device=y.device)
        assert torch.equal(p.aprev[(k + 1) % 2].index_select(0, live), p.aring[k % 3].index_select(0, live))
        # no runaway field stays in pipe.y: every row is finite; a trajectory that goes on is inside max_value, one that ended
        # holds its restart field (compared bit for bit above), whatever that field's own maximum is
        assert bool(torch.isfinite(p.y).all()), k
        if len(live):
            assert float(p.y.index_select(0, live).abs().max()) <= max_value, k


def _nets_finite(p):
    p.sync()
    for n in NETS:
        for x in getattr(p.policy, n).model.params():
            assert np.isfinite(x).all(), n


def test_blow_ups_restart_in_the_same_step(pkg):
    """fixed fields.  The fp64 oracle puts rows 0 - 4 below max_value = 1.5 for 14 steps and rows 5 and 7 above it after one."""
    B, E = 8, 7
    setup = pkg.KSSetup.KS22(max_value=1.5)
    p = _make(pkg, "ks22", B, E, y0=_scaled_y0(setup, B), setup_kw=dict(max_value=1.5), act_noise=0.1,
              episodes="per_trajectory", log_episodes=8)
    model = ClockModel(B, E, 8)
    y0, s0 = p.env.y0, p.state0
    _drained(p, 3 * E, model, lambda b, n: (y0[b], s0[b]))
    fin = p.finished_episodes()
    _same_fin(fin, model.finished())
    _assert_mix(fin, E)
    assert np.array_equal(p.episodes_finished, model.count)
    _nets_finite(p)


@pytest.mark.parametrize("rank", [(0, 1), (1, 3)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_restarts_draw_the_lockstep_fields(pkg, dtype, rank):
    """random fields, seed 5: by the oracle on these Philox draws some rows cross max_value = 5.0 within 0 - 9 steps, others not in 12"""
    B, E = 8, 7
    p = _make(pkg, "ks22", B, E, dtype=dtype, setup_kw=dict(max_value=5.0), act_noise=0.3, episodes="per_trajectory",
              log_episodes=8, random_init=True, init_seed=5, init_rank=rank)
    model = ClockModel(B, E, 8)
    rows = _Restarts(pkg, p)
    assert init_offset(3, rank[0], rank[1], B, 8) == (3 * rank[1] + rank[0]) * B * 2

    def restart(b, n):
        y, s = rows(n)
        return y[b], s[b]

    # (step 0 is the host's: episode 0 through Inits.draw)
    _drained(p, 1, model, restart)
    y, _ = rows(0)
    assert torch.equal(p.env.y0, y) and p.init_offsets == [init_offset(0, rank[0], rank[1], B, 8)]
    _drained(p, 4 * E - 1, model, restart)
    assert p.init_offsets == [init_offset(0, rank[0], rank[1], B, 8)] and max(rows.cache) == int(model.count.max())
    fin = p.finished_episodes()
    _same_fin(fin, model.finished())
    _assert_mix(fin, E)
    _nets_finite(p)


def test_keller_segel_restarts(pkg):
    B, E = 4, 5
    p = _make(pkg, "kseg", B, E, episodes="per_trajectory", log_episodes=4, random_init=True, init_seed=2)
    model = ClockModel(B, E, 4)
    rows = _Restarts(pkg, p)
    assert rows.ref.random_init_coefficients() == 8 and p.env.setup.temporal_steps == 2

    def restart(b, n):
        y, s = rows(n)
        return y[b], s[b]

    _drained(p, 3 * E, model, restart)
    fin = p.finished_episodes()
    _same_fin(fin, model.finished())
    assert len(fin["ret"]) >= 3 * B and sorted(rows.cache)[:3] == [1, 2, 3]


# ---------------------------------------------------------------------------------------------------- 4. against the lock-stepped mode
@pytest.mark.parametrize("geom,agent_kw", [("ks22", None), ("c2", dict(quirk_target_broadcast=False))])
def test_mode_is_the_lockstep_pipeline_when_nothing_blows_up(pkg, geom, agent_kw):
    """c2 runs with quirk_target_broadcast=False: with the reward broadcast on, the lock-stepped run of the fused 3-layer nets
    sums the batch-mean reward from the env step's per-workgroup partials, the per-trajectory mode (which may have to sanitise
    rows first) by pdec_reward_mean -- another order of the same sum"""
    B, E, n_ep = 64, 17, 3
    kw = dict(agent_kw=agent_kw, random_init=True, init_seed=3, log_episodes=4)
    pl = _make(pkg, geom, B, E, **kw)
    pt = _make(pkg, geom, B, E, episodes="per_trajectory", **kw)
    assert pl.rpart is None and pt.rpart is None
    # three whole episodes and five steps of the fourth: at the boundary itself the two modes hold different things in y -- the
    # clock has already written the next episode's field where the lock-stepped run draws it at the next step
    n = n_ep * E + 5
    pl.run(n)
    pt.run(n)
    pl.sync(); pt.sync()
    assert pt.n_eager_steps == pl.n_eager_steps == n and pl.n_episodes == n_ep
    assert pl.init_offsets == [init_offset(e, 0, 1, B, 8) for e in range(n_ep + 1)] and pt.init_offsets == pl.init_offsets[:1]
    assert torch.equal(pl.y, pt.y) and torch.equal(pl.state, pt.state)
    for n in NETS:
        for x, y in zip(getattr(pl.policy, n).model.params(), getattr(pt.policy, n).model.params()):
            assert np.array_equal(x, y), n
    for n in NETS[:2]:
        assert _adam(getattr(pl.policy, n)) == _adam(getattr(pt.policy, n)), n
    ret, blew, dropped = pl.episode_returns()
    fin = pt.finished_episodes()
    assert dropped == fin["dropped"] == 0 and not blew.any() and not fin["blew_up"].any()
    assert np.array_equal(fin["ret"].reshape(n_ep, B), ret)
    assert np.array_equal(fin["trajectory"], np.tile(np.arange(B), n_ep)) and (fin["length"] == E).all()
    assert np.array_equal(fin["end_step"], np.repeat(E * np.arange(1, n_ep + 1), B))
    with pytest.raises(pkg._lib.PdecError, match="finished_episodes"):
        pt.episode_returns()
    with pytest.raises(pkg._lib.PdecError, match="finished_episodes"):
        pt.rewards
    with pytest.raises(pkg._lib.PdecError, match="per_trajectory"):
        pl.finished_episodes()


# ---------------------------------------------------------------------------------------------------- 5. graphs
def test_graphs_equal_eager_steps(pkg):
    """C2 geometry, staggered clocks, max_value = 6.0 and rows of generate_random_init scaled by 0.05 .. 0.35, every eighth one by
    2.0: by the oracle the eighth rows start above the bound (max|y0| = 7.7, 8.6, ...) and end after one step every time, while
    the others stay below 6.0 for 17 steps at any action amplitude that the clamp to +-1 leaves (noise 0.3: none crosses; noise
    3.0, all but clamped: the earliest after 11 steps)"""
    B, E = 64, 17
    setup = pkg.KSSetup.bench_C2(256, max_value=6.0)
    y0 = _scaled_y0(setup, B)
    y0[7::8] *= 5.0
    kw = dict(y0=y0, setup_kw=dict(max_value=6.0), act_noise=0.3, episodes="per_trajectory", stagger=True, log_episodes=16)
    pg = _make(pkg, "c2", B, E, graphs=True, **kw)
    pe = _make(pkg, "c2", B, E, graphs=False, **kw)
    if not pg.use_graphs:
        pytest.fail("the pipeline refused graphs")
    pg.run(5)
    pg.capture()
    assert pg._captured and len(pg.graphs) == 2 * 6                    # every chunk at every ring phase: nothing is out of reach
    t0, eager0, n = pg.tick, pg.n_eager_steps, 6 * 8
    pg.run(n)
    assert pg.n_eager_steps == eager0 and pg.n_graph_launches == 8 and pg.tick == t0 + n
    pe.run(t0 + n)
    pg.sync(); pe.sync()
    fg, fe = pg.finished_episodes(), pe.finished_episodes()
    _same_fin(fg, fe)
    _assert_mix(fg, E)
    assert np.array_equal(pg.episodes_finished, pe.episodes_finished)
    # the first time-out of trajectory b comes after E - floor(b E / B) steps unless it blew up before
    c0 = initial_clocks(B, E, True)
    first = fg["episode"] == 0
    quiet = first & ~fg["blew_up"]
    assert quiet.any() and np.array_equal(fg["length"][quiet], (E - c0)[fg["trajectory"][quiet]])
    assert torch.equal(pg.y, pe.y)
    for net in NETS:
        for x, y in zip(getattr(pg.policy, net).model.params(), getattr(pe.policy, net).model.params()):
            assert np.array_equal(x, y), net
            assert np.isfinite(x).all(), net


# ---------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_by_name(pkg):
    lib = pkg._lib.load()
    Err = pkg._lib.PdecError

    def pipe(setup, B=2, dtype=torch.float32, agent_kw=None, **kw):
        s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
        env = pkg.PDEenv(setup, B=B, dtype=dtype, stream=s_env, autoreset=False)
        agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                                 noise_seed=7, trajectory_length=1, **(agent_kw or {}))
        agent.policy.act_noise = 0.3
        torch.cuda.synchronize()
        args = dict(lag=2, episode_steps=13, stream_env=s_env, stream_upd=s_upd, use_graphs=False, episodes="per_trajectory")
        args.update(kw)
        return pkg.TrainPipeline(env, agent, **args)

    ks = pkg.KSSetup.KS22
    with pytest.raises(Err, match="fluid environment"):
        pipe(pkg.FluidSetup(nx=32))
    with pytest.raises(Err, match="2-D Keller-Segel"):
        pipe(pkg.KellerSegel2DSetup(nx=64, ny=64))
    with pytest.raises(Err, match="memory_size > 0"):
        pipe(ks(memory_size=2))
    with pytest.raises(Err, match=r"global agent \(mono\)"):
        pipe(pkg.KSSetup.KS22_global())
    with pytest.raises(Err, match="use_replay=True"):
        pipe(ks(), use_replay=True)
    red = pkg.distributed.NativeGradReducer(lib, rank=0, world_size=1, reduce_critic=False, force_split=True)
    with pytest.raises(Err, match="active reducer"):
        pipe(ks(), agent_kw=dict(reducer=red))
    for kw in (dict(eval_every=2, log_episodes=4), dict(min_best_episode=2, log_episodes=4), dict(best_by="eval")):
        with pytest.raises(Err, match="evaluate_actors"):
            pipe(ks(), **kw)
    for E in (0, -3):
        with pytest.raises(Err, match="episode_steps > 0"):
            pipe(ks(), episode_steps=E)
    with pytest.raises(Err, match="'lockstep' or 'per_trajectory'"):
        pipe(ks(), episodes="free")
    with pytest.raises(Err, match="stagger=True"):
        pipe(ks(), episodes="lockstep", stagger=True)
    # ... and the library's own: the clock serves the 1-D per-actuator environments
    h = pkg._lib.Handle()
    for setup, word in ((pkg.KSSetup.KS22_global(), b"mono"), (ks(memory_size=2), b"memory_size")):
        env = pkg.PDEenv(setup, B=2, dtype=torch.float32, stream=torch.cuda.Stream(), autoreset=False)
        assert lib.pdec_epclock_create(C.byref(h), env.handle, 5, 2, 0, 0, 0, 1) != 0 and word in lib.pdec_last_error()
    env = pkg.PDEenv(ks(), B=2, dtype=torch.float32, stream=torch.cuda.Stream(), autoreset=False)
    for args, word in (((0, 2, 0, 0, 0, 1), b"episode_steps"), ((5, 0, 0, 0, 0, 1), b"capacity"), ((5, 2, 0, 0, 2, 2), b"rank")):
        assert lib.pdec_epclock_create(C.byref(h), env.handle, *args) != 0 and word in lib.pdec_last_error()
    # a pipeline without a log keeps the counts and refuses the log by name
    p = pipe(ks())
    p.run(13)
    assert p.episodes_finished.tolist() == [1, 1]
    with pytest.raises(Err, match="log_episodes=0"):
        p.finished_episodes()


# ---------------------------------------------------------------------------------------------------- 8. reset_from
def test_reset_from_cuts_the_running_episodes(pkg):
    B, E, cut = 8, 7, 10
    p = _make(pkg, "ks22", B, E, episodes="per_trajectory", stagger=True, log_episodes=8)
    c0 = initial_clocks(B, E, True)
    assert np.array_equal(p.clock0, c0)
    model = ClockModel(B, E, 8, c0)
    restart = lambda b, n: (p.env.y0[b], p.state0[b])
    y0 = p.env.y0.clone()
    _drained(p, cut, model, restart)
    assert torch.equal(p.env.y0, y0)
    before = p.finished_episodes()
    _same_fin(before, model.finished())
    assert (before["length"] <= E).all() and len(before["ret"]) == int(model.count.sum()) > B
    assert model.len.any()                                           # episodes are running: the reset cuts them
    y1 = (y0 * 0.5).clone()
    p.reset_from(y1)
    model.set()
    assert p._first_tick == cut and p.ep_start == cut and p.tick == cut
    # every trajectory starts from the given field; trajectory B - 1 (clock E - 1) times out in the very next step
    _drained(p, E, model, restart)
    assert torch.equal(p.env.y0, y1) and torch.equal(p.state0, p.env.featurize(y1))
    after = p.finished_episodes()
    _same_fin(after, model.finished())
    new = after["end_step"] > cut
    # every trajectory timed out once more, after E - clock0[b] steps from the reset: the cut episodes left no entry
    assert new.sum() == B and np.array_equal(np.sort(after["trajectory"][new]), np.arange(B))
    assert np.array_equal(after["length"][new], (E - c0)[after["trajectory"][new]])
    assert np.array_equal(after["end_step"][new], cut + (E - c0)[after["trajectory"][new]])
    for key in ("trajectory", "episode", "ret", "length", "end_step"):
        assert np.array_equal(after[key][~new], before[key])
