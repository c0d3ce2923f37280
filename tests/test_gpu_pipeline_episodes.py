"""GPU tests of TrainPipeline's episode bookkeeping (PDEhook, src/PDEhook.jl:42-97): the device episode ledger (returns,
blow-up bits, batch means, best actor), random initial conditions per episode, the rank split of their Philox stream and the
2-D Keller-Segel initialiser."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import rng as orng

pytestmark = pytest.mark.gpu

NETS = ("behavior_actor", "behavior_critic", "target_actor", "target_critic")


def _setup(pkg, geom, **kw):
    if geom == "ks22":
        return pkg.KSSetup.KS22(**kw)
    if geom == "c2":
        return pkg.KSSetup.bench_C2(256, **kw)
    if geom == "kseg2d":
        return pkg.KellerSegel2DSetup(nx=64, ny=64, **kw)
    raise ValueError(geom)


def _make(pkg, geom, B=64, E=17, dtype=torch.float32, graphs=False, y0=None, setup_kw=None, **kw):
    setup = _setup(pkg, geom, **(setup_kw or {}))
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    if y0 is None and geom != "kseg2d":          # (2-D Keller-Segel: the setup's standard field)
        y0 = setup.generate_random_init(np.random.default_rng(0), B) * 0.15
    env = pkg.PDEenv(setup, B=B, dtype=dtype, y0=y0, stream=s_env, autoreset=False)
    agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                             noise_seed=7, trajectory_length=1)
    agent.policy.act_noise = 0.3
    torch.cuda.synchronize()
    return pkg.TrainPipeline(env, agent, lag=2, episode_steps=E, stream_env=s_env, stream_upd=s_upd, use_graphs=graphs,
                             chunks=(6, 1), noise_seed=99, **kw)


def _restate(rews, flags, E):
    """the ledger's order of arithmetic in NumPy: per step (sum over a in index order of fp64 values) / R added to the running
    return; per episode the batch mean summed in b order"""
    rets, blews, means = [], [], []
    for e in range(len(rews) // E):
        ret = np.zeros(rews[0].shape[0])
        blew = np.zeros(rews[0].shape[0], dtype=bool)
        for k in range(e * E, (e + 1) * E):
            r = rews[k].astype(np.float64)
            s = np.zeros(r.shape[0])
            for a in range(r.shape[1]):
                s = s + r[:, a]
            ret = ret + s / r.shape[1]
            blew |= flags[k] != 0
        t = 0.0
        for v in ret:
            t += v
        rets.append(ret)
        blews.append(blew)
        means.append(t / ret.shape[0])
    return np.array(rets), np.array(blews), means


def _drained(p, n, before_last=None):
    """n eager steps, the device drained after each; returns the host copies of every step's reward / flag ring slot.
    before_last(e): called before the last step of episode e"""
    p.drain_between = True
    rews, flags = [], []
    for _ in range(n):
        k = p.tick
        if before_last is not None and (k - p.ep_start) % p.E == p.E - 1:
            torch.cuda.synchronize()
            before_last((k - p.ep_start) // p.E)
        p.step()
        torch.cuda.synchronize()
        rews.append(p.rring[k % 3].cpu().numpy())
        flags.append(p.fring[k % 3].cpu().numpy())
    return rews, flags


@pytest.mark.parametrize("geom,dtype,setup_kw", [("ks22", torch.float32, None), ("c2", torch.float32, None),
                                                 ("ks22", torch.float64, None), ("ks22", torch.float32, dict(max_value=1.0))])
def test_ledger_returns_are_bit_exact(pkg, geom, dtype, setup_kw):
    E = 17
    p = _make(pkg, geom, dtype=dtype, E=E, setup_kw=setup_kw, log_episodes=8)
    assert p.act_in_place == (geom == "ks22")
    rews, flags = _drained(p, 4 * E)
    ret, blew, means = _restate(rews, flags, E)
    g_ret, g_blew, dropped = p.episode_returns()
    assert dropped == 0 and g_ret.shape == (4, 64)
    assert np.array_equal(g_ret, ret, equal_nan=True)
    assert np.array_equal(g_blew, blew)
    assert np.array_equal(np.array(p.rewards), np.array(means), equal_nan=True)
    if setup_kw:                          # a small max_value stops trajectories: their bits are raised
        assert blew.any()


def test_ledger_ring_drops_the_oldest_rows(pkg):
    E = 13
    p = _make(pkg, "ks22", E=E, log_episodes=2)
    rews, flags = _drained(p, 3 * E)
    ret, _, means = _restate(rews, flags, E)
    g_ret, _, dropped = p.episode_returns()
    assert dropped == 1 and np.array_equal(g_ret, ret[1:])
    assert p.rewards == means[1:]


def _state(p):
    p.sync()
    ret, blew, _ = p.episode_returns()
    nets = {n: getattr(p.policy, n).model.params() for n in NETS}
    return ret, blew, p.rewards, p.bestreward, p.bestepisode, p.best_actor().params(), nets, p.y.cpu().numpy()


@pytest.mark.parametrize("geom", ["c2", "ks22"])
def test_graph_replay_equals_eager(pkg, geom):
    E, n_ep = 17, 10
    pg = _make(pkg, geom, graphs=True, E=E, log_episodes=16, min_best_episode=2)
    pe = _make(pkg, geom, graphs=False, E=E, log_episodes=16, min_best_episode=2)
    if not pg.use_graphs:
        pytest.fail("the pipeline refused graphs")
    pg.run(5)
    pg.capture()
    assert pg._captured and pg.graphs and pg.tick < (n_ep - 2) * E
    pg.run(n_ep * E - pg.tick)
    pe.run(n_ep * E)
    assert pg.n_graph_launches > 0 and pg.n_episodes == pe.n_episodes == n_ep
    a, b = _state(pg), _state(pe)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)
    assert a[3:5] == b[3:5] and a[4] >= 2
    for x, y in zip(a[5], b[5]):
        assert np.array_equal(x, y)
    for n in NETS:
        for x, y in zip(a[6][n], b[6][n]):
            assert np.array_equal(x, y), n
    assert np.array_equal(a[7], b[7])


@pytest.mark.parametrize("geom", ["c2", "ks22"])
def test_ledger_has_no_side_effects(pkg, geom):
    E = 17
    pa = _make(pkg, geom, E=E, log_episodes=4)
    pb = _make(pkg, geom, E=E)
    pa.run(3 * E)
    pb.run(3 * E)
    pa.sync(); pb.sync()
    for n in NETS:
        for x, y in zip(getattr(pa.policy, n).model.params(), getattr(pb.policy, n).model.params()):
            assert np.array_equal(x, y), n
    assert torch.equal(pa.y, pb.y)
    for i in range(3):
        assert torch.equal(pa.rring[i], pb.rring[i])


@pytest.mark.parametrize("geom", ["c2", "ks22"])
def test_best_actor_follows_the_hook_rule(pkg, geom):
    E, n_ep, mbe = 13, 5, 2
    p = _make(pkg, geom, E=E, log_episodes=8, min_best_episode=mbe)
    clones = []
    rews, flags = _drained(p, 4 * E, before_last=lambda e: clones.append(p.actor.params()))
    # episode 4 starts with one trajectory from a NaN field: its mean is NaN and it is never chosen
    y0 = p.env.y0.clone()
    y0[3] = float("nan")
    p.reset_from(y0)
    r2, f2 = _drained(p, E, before_last=lambda e: clones.append(p.actor.params()))
    ret, _, means = _restate(rews + r2, flags + f2, E)
    assert np.isnan(means[4]) and np.isnan(p.rewards[4])
    assert np.array_equal(np.array(p.rewards), np.array(means), equal_nan=True)
    best, best_e = -1e6, 0
    seen = []
    for e, m in enumerate(means):
        if e + 1 >= mbe and not np.isnan(m):
            seen.append(m)
            if m >= max(seen):
                best, best_e = m, e + 1
    assert best_e >= mbe and p.bestepisode == best_e and p.bestreward == best
    got = p.best_actor()
    assert isinstance(got, pkg.nna.CustomNeuralNetworkApproximator)
    for x, y in zip(got.params(), clones[best_e - 1]):
        assert np.array_equal(x, y)
    # the best actor serves a rollout once cloned to the env's dtype and stream, and loads through checkpoint.load_actor
    m = got.model.clone(dtype=p.env.dtype)
    out = p.env.rollout(m, 2)
    assert out["reward_sum"].shape[0] == p.env.B
    other = pkg.nna.CustomNeuralNetworkApproximator(got.model.clone())
    pkg.checkpoint.load_actor(other, got.params())
    for x, y in zip(other.params(), got.params()):
        assert np.array_equal(x, y)


def test_random_inits_follow_the_hook_stream(pkg):
    E, seed = 13, 5
    p = _make(pkg, "ks22", E=E, random_init=True, init_seed=seed, log_episodes=4)
    ref = pkg.PDEenv(p.env.setup, B=p.env.B, dtype=p.env.dtype, stream=p.s_env, autoreset=False)
    n = ref.random_init(seed, 0)
    assert n == p.env.B * 2                                     # 8 coefficients: 2 counters per trajectory
    p.drain_between = True
    for e in range(3):
        k = p.tick
        p.step()
        torch.cuda.synchronize()
        want = torch.empty_like(ref.y)
        with torch.cuda.stream(p.s_env):
            ref.random_init(seed, e * n, out=want)
        torch.cuda.synchronize()
        assert torch.equal(p.ybuf[k % 2], want) and torch.equal(p.env.y0, want)
        feat = torch.empty_like(p.state0)
        with torch.cuda.stream(p.s_env):
            pkg._lib.check(ref.lib.pdec_featurize(ref.handle, pkg._lib.ptr(want), None, pkg._lib.ptr(feat)))
        torch.cuda.synchronize()
        assert torch.equal(p.state0, feat)
        for _ in range(E - 1):
            p.step()
        torch.cuda.synchronize()
        assert float(p.tring[(p.tick - 1) % 3].min()) == 1.0         # the last transition is terminal: no bootstrap across
    assert p.init_offsets == [0, n, 2 * n]


def test_random_inits_fluid(pkg):
    """the fluid's draw (setup.random_init_device with the pipeline's init_rng).  The fluid environment does not run in
    TrainPipeline (its env step has no per-column terminal output), so the episode-start draw is called directly."""
    setup = pkg.FluidSetup(nx=32)
    B = 4
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    env = pkg.PDEenv(setup, B=B, dtype=torch.float64, stream=s_env, autoreset=False)
    agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                             noise_seed=7, trajectory_length=1)
    torch.cuda.synchronize()
    p = pkg.TrainPipeline(env, agent, lag=2, episode_steps=3, stream_env=s_env, stream_upd=s_upd, use_graphs=False,
                          random_init=True, init_rng=np.random.default_rng(11))
    rng = np.random.default_rng(11)
    for e in range(2):
        p._draw_init()
        with torch.cuda.stream(s_env):
            want = setup.random_init_device(env, rng)
        torch.cuda.synchronize()
        assert torch.equal(env.y0, want) and bool(torch.isfinite(want).all())
        assert not torch.equal(want, torch.zeros_like(want))


@pytest.mark.parametrize("geom,E", [("ks22", 13), ("kseg2d", 3)])
def test_ranks_share_one_draw(pkg, geom, E):
    B = 32 if geom == "ks22" else 8
    kw = dict(E=E, random_init=True, init_seed=3)
    one = _make(pkg, geom, B=B, **kw)
    half = [_make(pkg, geom, B=B // 2, init_rank=(r, 2), **kw) for r in range(2)]
    for p in [one] + half:
        p.drain_between = True
    for e in range(3):
        fields = []
        for p in [one] + half:
            k = p.tick
            p.step()
            torch.cuda.synchronize()
            fields.append(p.ybuf[k % 2].clone())
            p.run(E - 1)
            p.sync()
        assert torch.equal(fields[0], torch.cat(fields[1:]))


def _kseg2d_numpy(setup, seed, off, B):
    nsx, nsy = int(np.ceil(setup.Lx / 3)), int(np.ceil(setup.ny * setup.dx / 3))
    a = orng.random_init_coefficients(seed, off, B, 2 * (nsx + nsy)).reshape(B, 2, nsx + nsy)
    xx, yy = setup.dx * np.arange(1, setup.nx + 1), setup.dx * np.arange(1, setup.ny + 1)
    y = np.ones((B, 2, setup.ny, setup.nx))
    for i in range(1, nsx + 1):
        y += a[:, :, i - 1, None, None] * np.sin(i * xx / (2 * np.pi * (setup.Lx / 22)))[None, None, None, :]
    for i in range(1, nsy + 1):
        y += a[:, :, nsx + i - 1, None, None] * np.sin(i * yy / (2 * np.pi * (setup.ny * setup.dx / 22)))[None, None, :, None]
    return np.moveaxis(y, 1, -1), (2 * (nsx + nsy) + 3) // 4          # memory [B][ny][nx][2]


@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 3e-7)])
def test_kseg2d_random_init_matches_numpy(pkg, n, dtype, tol):
    setup = pkg.KellerSegel2DSetup(nx=n, ny=n)
    B, seed, off = 3, 17, 1000
    env = pkg.PDEenv(setup, B=B, dtype=dtype, stream=torch.cuda.Stream(), autoreset=False)
    with torch.cuda.stream(env.stream):
        y = torch.empty_like(env.y)
        used = env.random_init(seed, off, out=y)
    torch.cuda.synchronize()
    want, c = _kseg2d_numpy(setup, seed, off, B)
    assert used == B * c
    if n == 256:
        assert c == 9                                          # C4: 36 coefficients
    got = y.cpu().numpy().astype(np.float64)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= tol


def test_refusals(pkg):
    with pytest.raises(pkg._lib.PdecError, match="episode_steps"):
        _make(pkg, "ks22", E=0, log_episodes=4)
    lib = pkg._lib.load()
    setup = pkg.KSSetup.bench_C2(256)
    s_env, s_upd, s_ar = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    y0 = setup.generate_random_init(np.random.default_rng(0), 16) * 0.15
    env = pkg.PDEenv(setup, B=16, dtype=torch.float32, y0=y0, stream=s_env, autoreset=False)
    red = pkg.distributed.NativeGradReducer(lib, rank=0, world_size=1, reduce_critic=False, force_split=True)
    agent = pkg.create_agent(setup=setup, B=16, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                             noise_seed=7, trajectory_length=1, reducer=red)
    torch.cuda.synchronize()
    kw = dict(lag=2, episode_steps=13, stream_env=s_env, stream_upd=s_upd, use_graphs=False, stream_ar=s_ar)
    with pytest.raises(pkg._lib.PdecError, match="reducer"):
        pkg.TrainPipeline(env, agent, log_episodes=4, min_best_episode=2, **kw)
    p = pkg.TrainPipeline(env, agent, log_episodes=4, **kw)
    p.run(13)
    ret, _, _ = p.episode_returns()
    assert ret.shape == (1, 16) and np.isfinite(ret).all()
    with pytest.raises(pkg._lib.PdecError, match="reducer"):
        p.best_actor()
    # a dims mismatch in the best-parameter copy
    q = _make(pkg, "ks22", E=13, log_episodes=2)
    q.run(13)
    m = q.actor
    wrong = pkg.nna.HipMLP([m.dims[0], m.dims[1] + 1] + m.dims[2:], m.acts, None, m.dtype, m.device, 1, m.stream)
    assert lib.pdec_ledger_best_params(q.ledger.h, wrong.handle) != 0
    assert "layer sizes" in lib.pdec_last_error().decode()
    assert q.best_actor().model.dims == m.dims
