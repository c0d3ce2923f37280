"""Temporally correlated exploration noise (pdec_mlp_set_noise_color) on every acting kernel that honours it: the NoiseColor
instantiations of policy_act_fused_kernel, policy_act2_kernel, small_act_kernel (pdec_policy_act_rng_dev, _rng_as),
step_glue_kernel and act_noise_clamp_kernel (the generic sequence).  The rows are those of noise_scale_cases.py, the correlations,
the fp64 model and the bounds noise_color_cases.py; test_noise_color_table.py holds them without a GPU.  Every row asserts its
route through pdec_debug_batched_update_route BEFORE anything is launched, with the state array already set.

What is asserted, over STEPS = 4 consecutive acting calls.  (1) a = 0 everywhere is the run with nothing set bit for bit, once
with the scalar amplitude and once with a mixed noise_scale array; afterwards the state is the last step's z within
state_tolerance(1, 0) and the device noise counter has advanced identically.  (2) with mixed correlations, mixed amplitudes and a
caller-written x0, at every step action - greedy is scale_c x_t[c] of the model within
draw_tolerance(greedy, scale_c, x_c) + scale_c e_t and the state array is the model's within e_t = state_tolerance(t, a).
(3) state elements of rows >= noise_rows keep a sentinel bit for bit and those action rows are greedy.  (4) learning = 0 leaves
the state bit-unchanged, NULL restores the plain run bit for bit.  (5) the refusals, by message.  Everything stated as "bit for
bit" is compared as integers."""
import ctypes as C

import numpy as np
import pytest

import noise_color_cases as cc
from util import to_dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = -123.456


def _dt(prec):
    return torch.float64 if prec == "f64" else torch.float32


def _bits(t):
    t = t.contiguous()
    return t.view({8: torch.int64, 4: torch.int32}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _params(dims, seed):
    rng = np.random.default_rng(seed)
    P = []
    for i in range(len(dims) - 1):
        lim = np.sqrt(6.0 / (dims[i] + dims[i + 1]))
        P += [rng.uniform(-lim, lim, (dims[i + 1], dims[i])).astype(np.float32), rng.uniform(-0.1, 0.1, dims[i + 1]).astype(np.float32)]
    return P


class _Acting:
    """one row: the actor, its states, the colour arrays and STEPS consecutive acting calls through the row's entry point"""

    def __init__(self, pkg, name, how="auto"):
        self.pkg, self.L, self.r = pkg, pkg._lib, cc.ROWS[name]
        r = self.r
        self.cols, self.no, self.n = cc.cols(r), r.dims[-1], cc.entries(r)
        self.nrows = self.no if r.noise_rows < 0 else r.noise_rows
        self.m = pkg.HipMLP(r.dims, list(r.acts), _params(r.dims, 5), dtype=_dt(r.net_dtype), max_cols=self.cols)
        self.lib = self.m.lib
        if r.noise_rows > 0:
            self.L.check(self.lib.pdec_mlp_set_noise_rows(self.m.handle, r.noise_rows))
        self.sdt = _dt(r.state_dtype)
        self.states = to_dev(np.random.default_rng(9).uniform(-1, 1, (self.cols, r.dims[0])), self.sdt)
        self.how = how if how != "auto" else ("as" if r.state_dtype != r.net_dtype else "dev")
        self.inc = cc.counters(r)
        self.state = torch.zeros(self.cols * self.no, dtype=torch.float64, device="cuda:0")
        self.ab = self.scale = None
        # the route with the state array set, before anything is launched: colour does not change it
        self.color(np.zeros(self.n))
        name_, lds = C.create_string_buffer(128), C.c_int64(-1)
        self.L.check(self.lib.pdec_debug_batched_update_route(self.m.handle, 0, 0, 0, self.cols, 4, name_, 128, C.byref(lds)))
        assert name_.value.decode() == r.kernel, (name, name_.value.decode())
        self.color(None)

    def color(self, a, x0=None):
        """a: [n] correlations (None: off); x0 [cols, outputs] (None: zeros)"""
        if a is None:
            self.m.set_noise_color(None)
            return
        self.ab = to_dev(cc.ab_of(a), torch.float64)
        self.state.copy_(torch.as_tensor(np.zeros((self.cols, self.no)) if x0 is None else x0, dtype=torch.float64).reshape(-1))
        self.m.set_noise_color(self.state, self.ab, self.r.cpe)

    def scale_(self, scale):
        if scale is None:
            self.m.set_noise_scale(None)
        else:
            self.scale = to_dev(scale, torch.float64)
            self.m.set_noise_scale(self.scale, self.r.cpe)

    def counter(self):
        v = C.c_uint64()
        self.L.check(self.lib.pdec_noise_counter_get(self.m.handle, C.byref(v)))
        return v.value

    def act(self, t, act_noise, learning=1, limit=cc.ACT_LIMIT):
        """acting call number t of a run (the stream's offset is OFFSET + t counters(row))"""
        r, L, lib, m = self.r, self.L, self.lib, self.m
        out = torch.full((self.cols, self.no), float("nan"), dtype=self.sdt, device="cuda:0")
        off = cc.OFFSET + t * self.inc
        if self.how == "glue":
            assert learning == 1
            served = C.c_int(0)
            L.check(lib.pdec_step_glue(m.handle, m.handle, L.dtype_code(self.sdt), None, None, r.A, 0, None, None, 1, 0, 0, 1,
                                       L.ptr(self.states), self.cols, float(act_noise), float(limit), cc.SEED, off, L.ptr(out),
                                       None, None, 1, 0, 0, L.Handle(0), C.byref(served)))
            assert served.value == 1
        elif self.how == "dev":
            if t == 0:
                L.check(lib.pdec_noise_counter_set(m.handle, cc.OFFSET))
            L.check(lib.pdec_policy_act_rng_dev(m.handle, L.ptr(self.states), self.cols, float(act_noise), float(limit), learning,
                                                cc.SEED, L.ptr(out)))
        else:
            served = C.c_int(0)
            L.check(lib.pdec_policy_act_rng_as(m.handle, L.dtype_code(self.sdt), L.ptr(self.states), self.cols, float(act_noise),
                                               float(limit), learning, cc.SEED, off, L.ptr(out), C.byref(served)))
            assert served.value == 1
        torch.cuda.synchronize()
        return out

    def run(self, act_noise, limit=cc.ACT_LIMIT):
        return [self.act(t, act_noise, limit=limit) for t in range(cc.STEPS)]

    def greedy(self):
        how, self.how = self.how, ("as" if self.r.state_dtype != self.r.net_dtype else "dev")
        try:
            return self.act(0, 0.0, learning=0)
        finally:
            self.how = how

    def z(self):
        from oracle import rng
        return np.stack([rng.randn(cc.SEED, cc.OFFSET + t * self.inc, self.cols * self.no).reshape(self.cols, self.no)
                         for t in range(cc.STEPS)])


CASES = [(name, "auto", cc.ACT_LIMIT) for name in sorted(cc.ROWS)] + [(cc.GLUE_ROW, "glue", cc.ACT_LIMIT), (cc.CLAMP_ROW, "auto", 1.0)]
IDS = [f"{n}-{h}-{'clamp' if lim == 1.0 else 'free'}" for n, h, lim in CASES]


@pytest.mark.parametrize("name,how,limit", CASES, ids=IDS)
def test_zero_correlation_is_the_white_run(pkg, name, how, limit):
    a = _Acting(pkg, name, how)
    z = a.z()
    e1 = float(cc.state_tolerance(1, 0.0))
    for scale in (None, cc.mixed(a.n)):
        a.color(None)
        a.scale_(scale)
        plain = a.run(cc.EQUAL, limit)
        ctr_plain = a.counter() if a.how == "dev" else None
        assert not _same(plain[0], plain[1])
        a.color(np.zeros(a.n))
        got = a.run(cc.EQUAL, limit)
        for t in range(cc.STEPS):
            assert _same(got[t], plain[t]), (name, how, "scale" if scale is not None else "scalar", t)
        if a.how == "dev":
            assert a.counter() == ctr_plain == cc.OFFSET + cc.STEPS * a.inc
        x = _np(a.state).reshape(a.cols, a.no)
        err = np.abs(x[:, :a.nrows] - z[-1][:, :a.nrows]).max()
        print(f"[noise-color {name} {how}] a = 0: |state - z| = {err:.3e}, bound {e1:.3e}")
        assert err <= e1
        assert (x[:, a.nrows:] == 0.0).all()
        # switched off again: the plain run bit for bit
        a.color(None)
        again = a.run(cc.EQUAL, limit)
        assert all(_same(again[t], plain[t]) for t in range(cc.STEPS))
    a.scale_(None)
    a.m.close()


@pytest.mark.parametrize("name,how,limit", CASES, ids=IDS)
def test_recurrence_matches_the_model(pkg, name, how, limit):
    a = _Acting(pkg, name, how)
    r = a.r
    corr, scale = cc.corr(a.n), cc.mixed(a.n)
    # neighbouring entries differ in correlation AND amplitude: shift the amplitudes by one level against the correlations
    scale = np.roll(scale, 1) if a.n > 1 else scale
    a_c, s_c = cc.per_column(corr, r), cc.per_column(scale, r)
    x0 = np.random.default_rng(3).uniform(-1, 1, (a.cols, a.no))
    x0[:, a.nrows:] = SENTINEL
    xs = cc.model(x0, np.repeat(cc.ab_of(corr), r.cpe, axis=0), a.z(), a.nrows)
    g64 = _np(a.greedy())
    a.scale_(scale)
    a.color(corr, x0)
    worst_x = worst_a = 0.0
    clamped = 0
    for t in range(cc.STEPS):
        got = _np(a.act(t, 55.0, limit=limit))                      # (the scalar argument is not read with an array set)
        x = _np(a.state).reshape(a.cols, a.no)
        e_t = cc.state_tolerance(t + 1, a_c)
        for f in range(a.no):
            if f < a.nrows:
                ex = np.abs(x[:, f] - xs[t][:, f])
                worst_x = max(worst_x, float((ex / e_t).max()))
                assert (ex <= e_t).all(), (name, how, t, f, float(ex.max()), float(e_t.min()))
                want = np.clip(g64[:, f] + s_c * xs[t][:, f], -limit, limit)
                clamped += int((np.abs(want) == limit).sum())
                ea = np.abs(got[:, f] - want)
                tol = cc.action_tolerance(g64[:, f], s_c, xs[t][:, f], r.state_dtype, e_t)
                worst_a = max(worst_a, float((ea / np.maximum(tol, 1e-300))[s_c > 0].max(initial=0.0)))
                assert (ea <= tol).all(), (name, how, t, f, float(ea.max()), float(tol.min()))
            else:
                # (3) rows beyond the noise rows: state untouched, action greedy, bit for bit
                assert (x[:, f] == SENTINEL).all() and (got[:, f] == g64[:, f]).all(), (name, how, t, f)
    print(f"[noise-color {name} {how}] error / bound, worst element: state {worst_x:.3f}, action {worst_a:.3f}")
    assert (limit != 1.0) or clamped >= 2                             # the clamp case does clamp
    if r.noise_rows > 0:
        assert a.nrows < a.no
    # (4) learning = 0 touches nothing and is greedy
    if a.how != "glue":
        before = a.state.clone()
        assert (_np(a.act(0, 55.0, learning=0, limit=limit)) == np.clip(g64, -limit, limit)).all()
        assert _same(a.state, before)
    a.scale_(None)
    a.color(None)
    a.m.close()


def test_refusals_by_message(pkg):
    L = pkg._lib
    a = _Acting(pkg, "small_f32")
    r, lib, h = a.r, a.lib, a.m.handle
    out = torch.zeros((a.cols, 1), dtype=a.sdt, device="cuda:0")
    act = lambda learning=1: L.check(lib.pdec_policy_act_rng(h, L.ptr(a.states), a.cols, 0.1, 1.0, learning, 1, 0, L.ptr(out)))
    # a column-count mismatch, naming both numbers; a greedy call does not read the arrays and is served
    ab = to_dev(cc.ab_of(np.zeros(a.n + 1)), torch.float64)
    state = torch.zeros((a.n + 1) * r.cpe, dtype=torch.float64, device="cuda:0")
    a.m.set_noise_color(state, ab, r.cpe)
    with pytest.raises(pkg.PdecError, match=f"pdec_policy_act_rng: {a.cols} columns.*noise color.*{a.n + 1} entries x {r.cpe} columns = "
                                            f"{(a.n + 1) * r.cpe}"):
        act()
    act(0)
    # cols_per_entry differing from the scale's
    ab1 = to_dev(cc.ab_of(np.zeros(a.cols)), torch.float64)
    a.m.set_noise_color(a.state, ab1, 1)
    a.scale_(cc.mixed(a.n))
    with pytest.raises(pkg.PdecError, match=f"noise color set on the actor has 1 columns per entry, its noise scale {r.cpe}"):
        act()
    a.scale_(None)
    act()
    # the setter's own refusals
    for n, cpe, msg in ((0, 5, "0 entries x 5 columns"), (3, 0, "3 entries x 0 columns"), (2 ** 40, 2 ** 20, "entries x 1048576 columns")):
        with pytest.raises(pkg.PdecError, match="pdec_mlp_set_noise_color: .*" + msg):
            L.check(lib.pdec_mlp_set_noise_color(h, L.ptr(a.state), L.ptr(ab1), n, cpe))
    with pytest.raises(pkg.PdecError, match="pdec_mlp_set_noise_color: null .a, b. array"):
        L.check(lib.pdec_mlp_set_noise_color(h, L.ptr(a.state), None, 3, 5))
    with pytest.raises(pkg.PdecError, match="HipMLP.set_noise_color: contiguous float64 device tensors"):
        a.m.set_noise_color(a.state.float(), ab1, 1)
    with pytest.raises(pkg.PdecError, match=f"{a.cols} states, but {a.n} entries x 3 columns"):
        a.m.set_noise_color(a.state, to_dev(cc.ab_of(np.zeros(a.n)), torch.float64), 3)
    a.color(None)
    a.m.close()
    # the policy: correlations outside [0, 1) are refused on the host; it owns ab (b in fp64) and a zeroed state
    setup = pkg.KSSetup.bench_C2(256)
    B = 2
    A = setup.state_shape[1]
    agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(1), dtype=torch.float32, start_steps=-1)
    pol = agent.policy
    for bad, msg in (([0.1, 1.0], r"entry 1 is 1\.0"), ([-0.2, 0.1], r"entry 0 is -0\.2"), (1.5, r"entry 0 is 1\.5"),
                     ([np.nan, 0.1], "entry 0 is nan"), (np.zeros((2, 1)), r"got shape \(2, 1\)")):
        with pytest.raises(ValueError, match="CustomDDPGPolicy.set_noise_corr: .*" + msg):
            pol.set_noise_corr(bad)
    with pytest.raises(ValueError, match="cols_per_entry must be an integer >= 1"):
        pol.set_noise_corr([0.1, 0.2], cols_per_entry=0)
    assert pol.noise_corr is None and pol.noise_state is None and pol.behavior_actor.model.noise_color is None
    pol.set_noise_corr([0.9, 0.0])
    assert np.array_equal(pol.noise_ab.cpu().numpy(), cc.ab_of([0.9, 0.0])) and pol.noise_state.shape == (B * A,)
    assert pol.behavior_actor.model.noise_color[2] == A == pol.number_actuators and not bool(pol.noise_state.any())
    env = pkg.PDEenv(setup, B=B, dtype=torch.float32, autoreset=False)
    pol(env)
    torch.cuda.synchronize()
    assert bool(pol.noise_state.any())
    pol.reset_noise_state()
    torch.cuda.synchronize()
    assert not bool(pol.noise_state.any())
    # an exploring rollout with colour set is refused by name; a greedy one is served
    actor = pol.behavior_actor.model
    with pytest.raises(pkg.PdecError, match="pdec_rollout: a noise color is set on the actor"):
        env.rollout(actor, 2, act_noise=0.1, learning=True)
    env.reset()
    env.rollout(actor, 2, learning=False)
    torch.cuda.synchronize()
    # a scalar is sized by the first acting call
    pol.set_noise_corr(0.5)
    assert pol.noise_corr == 0.5 and pol.noise_state is None
    env.reset()
    pol(env)
    torch.cuda.synchronize()
    assert pol.noise_ab.shape == (B, 2) and pol.noise_ab[:, 0].tolist() == [0.5, 0.5] and bool(pol.noise_state.any())
    pol.set_noise_corr(None)
    assert pol.noise_corr is None and actor.noise_color is None
    env.close()


def test_population_and_per_trajectory_episodes_refuse_it(pkg):
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    setup = pkg.KSSetup.KS22()
    agents = [pkg.create_agent(setup=setup, B=1, rng=np.random.default_rng(i), noise_seed=i, stream=s_upd) for i in range(2)]
    hooks = [pkg.PDEhook(init_seed=i) for i in range(2)]
    agents[1].policy.set_noise_corr(0.5)
    with pytest.raises(pkg.PdecError, match="member 1: a noise correlation is set on its policy"):
        pkg.Population(setup, agents, hooks, stream_env=s_env)
    # the library's own refusal: the Python marks removed, the arrays still set on the handle
    pol = agents[1].policy
    pol.size_noise_state(setup.state_shape[1])
    model = pol.behavior_actor.model
    keep, pol.noise_corr, model.noise_color = (pol.noise_corr, model.noise_color), None, None
    with pytest.raises(pkg.PdecError, match="pdec_population_create: member 1: a noise color is set on its actor"):
        pkg.Population(setup, agents, hooks, stream_env=s_env)
    pol.noise_corr, model.noise_color = keep
    pol.set_noise_corr(None)
    pkg.Population(setup, agents, hooks, stream_env=s_env).close()        # accepted once it is unset
    # per-trajectory episodes
    setup = pkg.KSSetup.bench_C2(256)
    B = 4
    y0 = setup.generate_random_init(np.random.default_rng(0), B) * 0.15
    env = pkg.PDEenv(setup, B=B, dtype=torch.float32, y0=y0, stream=s_env, autoreset=False)
    agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                             trajectory_length=1)
    torch.cuda.synchronize()
    with pytest.raises(pkg.PdecError, match=r"TrainPipeline\(noise_corr=...\) belongs to lock-stepped episodes.*episodes='per_trajectory'"):
        pkg.TrainPipeline(env, agent, lag=2, episode_steps=5, stream_env=s_env, stream_upd=s_upd, use_graphs=False,
                          episodes="per_trajectory", log_episodes=8, noise_corr=0.5)
    # a correlation set on the policy itself: the pipeline owns and zeroes its own states
    agent.policy.set_noise_corr(0.5)
    with pytest.raises(pkg.PdecError, match="TrainPipeline: a noise correlation is set on the policy"):
        pkg.TrainPipeline(env, agent, lag=2, episode_steps=5, stream_env=s_env, stream_upd=s_upd, use_graphs=False)
    agent.policy.set_noise_corr(None)
    env.close()
