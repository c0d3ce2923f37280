"""Per-trajectory exploration amplitude (pdec_mlp_set_noise_scale) on every acting path that honours it: policy_act_fused_kernel,
policy_act2_kernel, small_act_kernel (pdec_policy_act_rng, _rng_as, _rng_dev), step_glue_kernel, act_noise_clamp_kernel (the
generic sequence) and pdec_rollout with learning = 1 in its three forms (ks_rollout_kernel, kseg_rollout_kernel, the enqueued
step loop).  The rows are noise_scale_cases.py; test_noise_scale_table.py holds them without a GPU.  Every acting row asserts its
route through pdec_debug_batched_update_route BEFORE anything is launched, the rollouts through the launch counts of the profile.

What is asserted.  (1) an array of equal values is the scalar call bit for bit; (2) with three distinct amplitudes, one of them 0,
every column is bit for bit the scalar call at its amplitude and a zero-amplitude column equals the learning = 0 call under ==
(rollouts: at the first step; later steps persistent launch against step loop, 2e-11 / 2e-5 as in test_gpu_ks_disturbance.py);
(3) noisy - greedy - scale_c z_c, z from oracle/rng.py at element column * outputs + row, within
3 u (|greedy| + |scale_c z_c|) + 1e-12 scale_c, and memory rows beyond noise_rows bit for bit greedy; (4) the refusals by message,
and NULL restores the scalar path bit for bit.  Everything stated as "bit for bit" is compared as integers.  act_limit = 100 keeps
every element off the clamp (the table test proves it); one case runs at act_limit = 1 to hold the order noise, then clamp."""
import ctypes as C

import numpy as np
import pytest

import ks_geometry_cases as kc
import noise_scale_cases as nc
from util import to_dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


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
    """one row: the actor, its states, and the acting call of the row's entry point"""

    def __init__(self, pkg, name):
        self.pkg, self.L, self.r = pkg, pkg._lib, nc.ROWS[name]
        r = self.r
        self.cols, self.no = nc.cols(r), r.dims[-1]
        self.m = pkg.HipMLP(r.dims, list(r.acts), _params(r.dims, 5), dtype=_dt(r.net_dtype), max_cols=self.cols)
        self.lib = self.m.lib
        if r.noise_rows > 0:
            self.L.check(self.lib.pdec_mlp_set_noise_rows(self.m.handle, r.noise_rows))
        self.sdt = _dt(r.state_dtype)
        self.states = to_dev(np.random.default_rng(9).uniform(-1, 1, (self.cols, r.dims[0])), self.sdt)
        # the route, before anything is launched
        name_, lds = C.create_string_buffer(128), C.c_int64(-1)
        self.L.check(self.lib.pdec_debug_batched_update_route(self.m.handle, 0, 0, 0, self.cols, 4, name_, 128, C.byref(lds)))
        assert name_.value.decode() == r.kernel, (name, name_.value.decode())
        self._keep = None

    def set(self, scale, cpe=None):
        if scale is None:
            self.m.set_noise_scale(None)
        else:
            self._keep = to_dev(scale, torch.float64)
            self.m.set_noise_scale(self._keep, self.r.cpe if cpe is None else cpe)

    def act(self, act_noise, learning=1, limit=nc.ACT_LIMIT, how="rng"):
        r, L, lib, m = self.r, self.L, self.lib, self.m
        out = torch.full((self.cols, self.no), float("nan"), dtype=self.sdt, device="cuda:0")
        if how == "glue":
            served = C.c_int(0)
            L.check(lib.pdec_step_glue(m.handle, m.handle, L.dtype_code(self.sdt), None, None, r.A, 0, None, None, 1, 0, 0, 1,
                                       L.ptr(self.states), self.cols, float(act_noise), float(limit), nc.SEED, nc.OFFSET, L.ptr(out),
                                       None, None, 1, 0, 0, L.Handle(0), C.byref(served)))
            assert served.value == 1
        elif how == "dev":
            L.check(lib.pdec_noise_counter_set(m.handle, nc.OFFSET))
            L.check(lib.pdec_policy_act_rng_dev(m.handle, L.ptr(self.states), self.cols, float(act_noise), float(limit), learning,
                                                nc.SEED, L.ptr(out)))
        elif how == "randn":          # pdec_randn + pdec_policy_act: act_noise_clamp_kernel with the caller's noise
            noise = torch.empty((self.cols, self.no), dtype=self.sdt, device="cuda:0")
            L.check(lib.pdec_randn(m.handle, L.ptr(noise), self.cols * self.no, L.dtype_code(self.sdt), nc.SEED, nc.OFFSET))
            L.check(lib.pdec_policy_act(m.handle, L.ptr(self.states), L.ptr(noise) if learning else None, self.cols, float(act_noise),
                                        float(limit), L.ptr(out)))
        elif r.state_dtype != r.net_dtype:
            served = C.c_int(0)
            L.check(lib.pdec_policy_act_rng_as(m.handle, L.dtype_code(self.sdt), L.ptr(self.states), self.cols, float(act_noise),
                                               float(limit), learning, nc.SEED, nc.OFFSET, L.ptr(out), C.byref(served)))
            assert served.value == 1
        else:
            L.check(lib.pdec_policy_act_rng(m.handle, L.ptr(self.states), self.cols, float(act_noise), float(limit), learning,
                                            nc.SEED, nc.OFFSET, L.ptr(out)))
        torch.cuda.synchronize()
        return out


def _hows(name):
    r = nc.ROWS[name]
    hows = ["rng"]
    if r.state_dtype == r.net_dtype:
        hows.append("dev")
    if r.kernel == "generic":
        hows.append("randn")
    if name == nc.GLUE_ROW:
        hows.append("glue")
    return hows


@pytest.mark.parametrize("name", sorted(nc.ROWS))
def test_acting_rows(pkg, name):
    from oracle import rng
    a = _Acting(pkg, name)
    r, n = a.r, nc.entries(a.r)
    z = rng.randn(nc.SEED, nc.OFFSET, a.cols * a.no).reshape(a.cols, a.no)
    nrows = a.no if r.noise_rows < 0 else r.noise_rows
    worst = 0.0
    for how in _hows(name):
        a.set(None)
        greedy = a.act(0.0, learning=0, how="rng" if how in ("glue", "dev") else how)
        scalar = {lv: a.act(lv, how=how) for lv in set(nc.LEVELS) | {nc.EQUAL}}
        assert not _same(scalar[nc.EQUAL], greedy) and bool(scalar[nc.EQUAL].abs().max() < 14.6)
        if 0.0 in scalar and how != "glue":
            assert bool((scalar[0.0] == greedy).all())
        # (1) equal values are the scalar; the call's own act_noise is not read
        a.set(np.full(n, nc.EQUAL))
        assert _same(a.act(0.0, how=how), scalar[nc.EQUAL]), (name, how, "equal values")
        assert _same(a.act(55.0, how=how), scalar[nc.EQUAL]), (name, how, "the scalar argument was read")
        if how != "glue":             # learning = 0 still means no noise
            assert _same(a.act(nc.EQUAL, learning=0, how=how), greedy), (name, how, "learning = 0")
        # (2) each column is its own scalar call
        mixed = nc.mixed(n)
        percol = nc.per_column(mixed, r)
        a.set(mixed)
        got = a.act(0.0, how=how)
        for lv in nc.LEVELS:
            sel = torch.as_tensor(percol == lv, device="cuda:0")
            assert int(sel.sum()) > 0 or n < 3               # (B = 1 with cols_per_entry = A: one entry, one level)
            assert torch.equal(_bits(got)[sel], _bits(scalar[lv])[sel]), (name, how, lv)
        zero = torch.as_tensor(percol == 0.0, device="cuda:0")
        assert bool((got[zero] == greedy[zero]).all())
        # (3) the draw is the stream's element column * outputs + row at the column's amplitude
        g64, d = _np(greedy), _np(got) - _np(greedy)
        for f in range(a.no):
            if f < nrows:
                err = np.abs(d[:, f] - percol * z[:, f])
                tol = nc.draw_tolerance(g64[:, f], percol, z[:, f], r.state_dtype)
                worst = max(worst, float((err / np.maximum(tol, 1e-300))[percol > 0].max(initial=0.0)))
                assert (err <= tol).all(), (name, how, f, float(err.max()), float(tol.min()))
            else:
                assert _same(got[:, f], greedy[:, f]), (name, how, "memory row", f)
        # NULL restores the scalar path bit for bit
        a.set(None)
        assert _same(a.act(nc.EQUAL, how=how), scalar[nc.EQUAL]), (name, how, "unset")
    print(f"[noise-scale {name}] draw error / bound, worst column: {worst:.3f}")
    a.m.close()


def test_noise_is_added_before_the_clamp(pkg):
    """act_limit = 1: where the scalar call clamps, so does the array call, and at amplitude 2 many elements do"""
    a = _Acting(pkg, nc.CLAMP_ROW)
    n = nc.entries(a.r)
    mixed = nc.mixed(n)
    percol = nc.per_column(mixed, a.r)
    scalar = {lv: a.act(lv, limit=1.0) for lv in nc.LEVELS}
    a.set(mixed)
    got = a.act(0.0, limit=1.0)
    assert bool(got.abs().max() == 1.0) and int((got.abs() == 1.0).sum()) >= 2
    for lv in nc.LEVELS:
        sel = torch.as_tensor(percol == lv, device="cuda:0")
        assert torch.equal(_bits(got)[sel], _bits(scalar[lv])[sel]), lv
    a.m.close()


def test_refusals_by_message(pkg):
    L = pkg._lib
    a = _Acting(pkg, "small_f32")
    r = a.r
    a.set(np.full(nc.entries(r) + 1, 0.5))
    out = torch.zeros((a.cols, 1), dtype=a.sdt, device="cuda:0")
    want = f"{a.cols} columns.*{nc.entries(r) + 1} entries x {r.cpe} columns = {(nc.entries(r) + 1) * r.cpe}"
    with pytest.raises(pkg.PdecError, match="pdec_policy_act_rng: " + want):
        L.check(a.lib.pdec_policy_act_rng(a.m.handle, L.ptr(a.states), a.cols, 0.1, 1.0, 1, 1, 0, L.ptr(out)))
    # a greedy call does not read the array and is served
    L.check(a.lib.pdec_policy_act_rng(a.m.handle, L.ptr(a.states), a.cols, 0.1, 1.0, 0, 1, 0, L.ptr(out)))
    with pytest.raises(pkg.PdecError, match="0 entries x 5"):
        L.check(a.lib.pdec_mlp_set_noise_scale(a.m.handle, L.ptr(a._keep), 0, 5))
    with pytest.raises(pkg.PdecError, match="float64 device tensor"):
        a.m.set_noise_scale(torch.zeros(3, dtype=torch.float32, device="cuda:0"), 5)
    a.set(None)
    a.m.close()
    # the policy's setter: host arrays are checked, the buffer is the policy's own
    setup = pkg.KSSetup.bench_C2(256)
    B = 2
    A = setup.state_shape[1]
    agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(1), dtype=torch.float32, start_steps=-1)
    pol = agent.policy
    for bad, msg in (([0.1, -1.0], r"entry 1 is -1\.0"), ([np.nan, 0.1], "entry 0 is nan"), (np.zeros((2, 1)), r"got shape \(2, 1\)")):
        with pytest.raises(ValueError, match=msg):
            pol.set_noise_scale(bad)
    with pytest.raises(ValueError, match="cols_per_entry must be an integer >= 1"):
        pol.set_noise_scale([0.1, 0.2], cols_per_entry=0)
    assert pol.noise_scale is None and pol.behavior_actor.model.noise_scale is None
    host = np.array([0.25, 0.0])
    pol.set_noise_scale(host)
    host[:] = 9.0                                  # the policy keeps its own copy
    assert pol.noise_scale.dtype == torch.float64 and pol.noise_scale.tolist() == [0.25, 0.0]
    assert pol.behavior_actor.model.noise_scale[1] == A == pol.number_actuators
    env = pkg.PDEenv(setup, B=B, dtype=torch.float32, autoreset=False)
    act = pol(env).clone()
    torch.cuda.synchronize()
    pol.set_noise_scale(None)
    pol._noise_off = 0
    pol.act_noise = 0.0
    greedy = pol(env).clone()
    torch.cuda.synchronize()
    assert bool((act[1] == greedy[1]).all()) and not _same(act[0], greedy[0])
    # a wrong length is refused by the acting call, naming both numbers
    pol.set_noise_scale(np.full(B + 1, 0.1))
    with pytest.raises(pkg.PdecError, match=f"{B * A} columns.*{B + 1} entries x {A} columns"):
        pol(env)
    pol.set_noise_scale(None)
    env.close()


def test_population_refuses_an_actor_with_an_array(pkg):
    """Population by member index before anything is allocated, and pdec_population_create itself for a caller that goes around
    the Python layer"""
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    setup = pkg.KSSetup.KS22()
    A = setup.state_shape[1]
    agents = [pkg.create_agent(setup=setup, B=1, rng=np.random.default_rng(i), noise_seed=i, stream=s_upd) for i in range(2)]
    hooks = [pkg.PDEhook(init_seed=i) for i in range(2)]
    agents[1].policy.set_noise_scale([0.1])
    made = []
    orig = pkg.PDEenv.__init__
    try:
        pkg.PDEenv.__init__ = lambda self, *a, **k: (made.append(1), orig(self, *a, **k))[1]
        with pytest.raises(pkg.PdecError, match="member 1: a noise scale array is set on its actor"):
            pkg.Population(setup, agents, hooks, stream_env=s_env)
    finally:
        pkg.PDEenv.__init__ = orig
    assert not made                                  # refused before the probe environment was made
    # the library's own refusal: the Python mark removed, the array still set on the handle
    model = agents[1].policy.behavior_actor.model
    assert model.noise_scale[1] == A
    keep, model.noise_scale = model.noise_scale, None
    with pytest.raises(pkg.PdecError, match="pdec_population_create: member 1: a noise scale array is set on its actor"):
        pkg.Population(setup, agents, hooks, stream_env=s_env)
    model.noise_scale = keep
    agents[1].policy.set_noise_scale(None)
    pop = pkg.Population(setup, agents, hooks, stream_env=s_env)        # accepted once it is unset
    pop.close()


# ------------------------------------------------------------------ rollouts
def _launches(env, label):
    ms, n = C.c_double(), C.c_int()
    assert env.lib.pdec_prof_get(env.handle, label.encode(), C.byref(ms), C.byref(n)) == 0
    return n.value


def _rollout(pkg, env, actor, T, label, want, **kw):
    """env.rollout from the environment's initial condition, with the route asserted from the profile's launch counts"""
    L = pkg._lib
    env.reset()
    L.check(env.lib.pdec_prof_reset(env.handle))
    L.check(env.lib.pdec_prof_enable(env.handle, 1))
    out = env.rollout(actor, T, act_limit=nc.ACT_LIMIT, learning=kw.pop("learning", True), seed=nc.SEED, offset=nc.OFFSET, log=True, **kw)
    torch.cuda.synchronize()
    assert _launches(env, label) == want, (label, _launches(env, label), want)
    L.check(env.lib.pdec_prof_enable(env.handle, 0))
    out["y_end"], out["state_end"] = env.y.clone(), env.state.clone()
    return out


KEYS = ("y", "p", "action", "reward", "reward_sum", "y_end", "state_end")


def _rollout_body(pkg, monkeypatch, env, actor, B, T, label, persistent):
    monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", persistent)
    want = 1 if persistent == "1" else 0
    run = lambda **kw: _rollout(pkg, env, actor, T, label, want, **kw)
    greedy = run(learning=False)
    scalar = {lv: run(act_noise=lv) for lv in set(nc.ROLL_LEVELS) | {nc.ROLL_EQUAL}}
    assert not _same(scalar[nc.ROLL_EQUAL]["y_end"], greedy["y_end"]) and bool(torch.isfinite(scalar[nc.ROLL_EQUAL]["y_end"]).all())
    # (1) equal values: y, reward_sum and the logs bit for bit the scalar launch; the scalar argument is not read
    eq = run(act_noise=77.0, noise_scale=np.full(B, nc.ROLL_EQUAL))
    for k in KEYS:
        assert _same(eq[k], scalar[nc.ROLL_EQUAL][k]), (label, persistent, k)
    assert actor.noise_scale is None                         # restored after the call
    # (2) a mixed array: at the first step every trajectory is the scalar launch at its amplitude
    mixed = nc.mixed(B, nc.ROLL_LEVELS)
    mx = run(noise_scale=mixed)
    for b in range(B):
        assert _same(mx["action"][0, b], scalar[mixed[b]]["action"][0, b]), (label, persistent, b)
        if mixed[b] == 0.0:          # and a zero amplitude is the greedy action
            assert bool((mx["action"][0, b] == greedy["action"][0, b]).all())
    # (the fields are not compared per trajectory: ks_rollout_kernel packs two trajectories into one complex FFT, so a
    # trajectory's field carries its partner's rounding, and the partner acts at another amplitude here than in the scalar launch)
    assert not _same(mx["action"][0, 0], greedy["action"][0, 0])
    # learning = 0 with an array: no noise
    assert _same(run(learning=False, noise_scale=mixed)["y_end"], greedy["y_end"])
    # a wrong length is refused by name
    with pytest.raises(ValueError, match=f"expected {B} amplitudes"):
        env.rollout(actor, 1, learning=True, noise_scale=np.zeros(B + 1))
    return mx


def _ks_env(pkg, prec):
    from oracle import ks
    case, B, T = nc.KS_ROLL
    setup, _ = kc.build(pkg, ks, case)
    ns, A = setup.state_shape
    y0 = kc.inputs(case, B, seed=3)[0]
    dt = _dt(prec)
    dims = [ns, kc.roll_h(case), 1]
    actor = pkg.HipMLP(dims, ["relu", "tanh"], _params(dims, 11), dtype=dt, max_cols=B * A)
    return pkg.PDEenv(setup, B=B, dtype=dt, y0=y0, autoreset=False), actor, B, T


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_ks_rollout_persistent_and_step_loop(pkg, monkeypatch, prec):
    """ks_rollout_kernel (solo form, B = 3: a lone last trajectory) and the enqueued step loop on the same row, then the two
    against each other under the same mixed array"""
    env, actor, B, T = _ks_env(pkg, prec)
    one = _rollout_body(pkg, monkeypatch, env, actor, B, T, "ks_rollout", "1")
    loop = _rollout_body(pkg, monkeypatch, env, actor, B, T, "ks_rollout", "0")
    sc = 1e-6 if prec == "f64" else 1.0
    worst = {}
    for k, tol in (("y", 2e-5), ("p", 2e-4), ("action", 2e-5), ("reward", 2e-5), ("reward_sum", 2e-5), ("y_end", 2e-5)):
        worst[k] = (float((_np(one[k]) - _np(loop[k])).__abs__().max()), tol * sc)
    print(f"[noise-scale ks rollout {prec}] persistent against the step loop (worst, bound):", worst)
    assert all(e <= t for e, t in worst.values()), worst
    # a direct library call with a wrong entry count is refused, naming both numbers
    L = pkg._lib
    A = env.setup.state_shape[1]
    keep = torch.zeros(B + 2, dtype=torch.float64, device="cuda:0")
    actor.set_noise_scale(keep, A)
    with pytest.raises(pkg.PdecError, match=f"pdec_rollout: {B * A} columns.*{B + 2} entries x {A} columns"):
        env.rollout(actor, 1, learning=True)
    actor.set_noise_scale(None)
    env.close(), actor.close()


def test_kseg_rollout_persistent(pkg, monkeypatch):
    """kseg_rollout_kernel on the shipped Keller-Segel geometry, fp64, B = 2"""
    B, T = nc.KSEG_ROLL
    setup, dt = pkg.KellerSegelSetup(), torch.float64
    y0 = np.ascontiguousarray(np.swapaxes(setup.generate_random_init(np.random.default_rng(0), B), 1, 2))
    agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(1), dtype=dt, start_steps=-1)
    env = pkg.PDEenv(setup, B=B, dtype=dt, y0=y0, autoreset=False)
    _rollout_body(pkg, monkeypatch, env, agent.policy.behavior_actor.model, B, T, "kseg_rollout", "1")
    env.close()
