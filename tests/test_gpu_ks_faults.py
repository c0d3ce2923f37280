"""Per-trajectory actuator and sensor faults (pdec_env_set_faults) on the device: the FLT instantiations of ks_env_step_kernel
(four FFT engines, the SIMD-sharing form, the member layout), of ksfd_wave_step_kernel and ksfd_env_step_kernel (both
integrators), of ks_rollout_kernel (solo, member and amplitude-array forms), of sense_kernel (prepare_action, featurize) and of the
episode clock's epclock_sense_kernel, and the Python layers above them (PDEenv.set_faults, KSSetup.fault_scenario,
evaluate_actors(faults=...), TrainPipeline on an environment that holds the arrays).

The reference is ks_fault_ref.py -- the unchanged pieces of oracle/ks.py on gain * action and gain * dots + bias -- with the rows of
ks_fault_cases.py; fp32 inputs and arrays are rounded once and the reference runs in fp64 from those values.
test_ks_fault_table.py shows without a GPU that another trajectory's arrays, sensor faults indexed by the actuator, a bias behind
the scale and faults let into the reward each move one control step by >= 30 fp32 bounds.

Tolerances: those of test_gpu_ks_geometry.py (ks_geometry_cases.tol_y / tol_p / tol_reward), none raised, and
ks_fault_cases.tol_state (tol_state with the two roundings of g * d + b); a persistent rollout against the enqueued step loop 2e-11 /
2e-5 (p 2e-10 / 2e-4), the bounds of test_rollout_equals_the_step_loop_or_is_not_served.  Everything stated as "bit for bit" is
compared as integers.  Every test prints its worst deviation beside its bound; DESIGN.md 3.1 records them."""
import ctypes as C

import numpy as np
import pytest

import ks_fault_cases as fc
import ks_fault_ref as fr
import ks_geometry_cases as kc
from util import to_dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PRECS = ("f64", "f32")
NETS = ("behavior_actor", "behavior_critic", "target_actor", "target_critic")
CANARY, PAD = 12345.0, 64


def _dt(prec):
    return torch.float64 if prec == "f64" else torch.float32


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _jl(t):
    return _np(t).T


def _cast(a, prec):
    return np.asarray(a, dtype=np.float32).astype(np.float64) if prec == "f32" else np.asarray(a, dtype=np.float64)


def _bits(t):
    t = t.contiguous()
    return t.view({8: torch.int64, 4: torch.int32}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _err(worst, key, dev, ref, tol):
    e = float(np.abs(np.asarray(dev) - np.asarray(ref)).max())
    if key not in worst or e / tol > worst[key][0] / worst[key][1]:
        worst[key] = (e, tol)
    return e <= tol


_MEMO = {}


def _row(pkg, case, prec):
    """(setup, oracle config, fault arrays at the values the device holds, geometry) of a row, built once"""
    from oracle import ks
    key = (case, prec)
    if key not in _MEMO:
        setup, cfg = kc.build(pkg, ks, case)
        f = {k: _cast(v, prec) for k, v in fc.faults(case).items()}
        _MEMO[key] = (setup, cfg, f, kc.geometry(*setup.tables(), case, prec))
    return _MEMO[key]


def _act(env, a, dt):
    return to_dev(a, dt).reshape(env._ashape)


def _actor_params(ns, H, seed):
    rng = np.random.default_rng(seed)
    dims = [ns, H, 1]
    P = []
    for i in range(2):
        lim = np.sqrt(6.0 / (dims[i] + dims[i + 1]))
        P += [rng.uniform(-lim, lim, (dims[i + 1], dims[i])).astype(np.float32), rng.uniform(-0.1, 0.1, dims[i + 1]).astype(np.float32)]
    return dims, P


def _member_layout(pkg, env, on=1):
    pkg._lib.check(env.lib.pdec_env_set_member_layout(env.handle, on))


def _rows(f, b):
    return tuple(f[k][b] for k in fc.KEYS)


# ------------------------------------------------------------------ 1. the fused step and its pieces against the reference
def _step_body(pkg, case, prec, form=""):
    from oracle import ks
    dt = _dt(prec)
    setup, cfg, f, g = _row(pkg, case, prec)
    B = fc.batch(case)
    y0, act, prev = kc.inputs(case, B, steps=fc.STEPS)
    y0, act, prev = _cast(y0, prec), _cast(act, prec), _cast(prev, prec)
    env = pkg.PDEenv(setup, B=B, dtype=dt, y0=y0, autoreset=False)
    pieces = pkg.PDEenv(setup, B=B, dtype=dt, autoreset=False)
    if form == "share":
        assert env.set_simd_sharing(True)
    if form == "member":
        _member_layout(pkg, env)
    for e in (env, pieces):
        e.set_faults(**f)
        assert [getattr(e, k).dtype for k in fc.KEYS] == [dt] * 3 and e.sensor_bias.shape == (B, setup.n_sensors)
    env.reset()                        # the initial state through the sensors the environment now has
    torch.cuda.synchronize()
    worst, ok = {}, True
    gmax = [float(np.abs(f["sensor_gain"][b]).max()) for b in range(B)]
    bmax = [float(np.abs(f["sensor_bias"][b]).max()) for b in range(B)]
    for b in range(B):                 # reset: featurize(y0) through the faults, the temporal stack repeated
        ts = fc.tol_state(prec, case, g, float(np.abs(y0[b]).max()), gmax[b], bmax[b])
        ok &= _err(worst, "state0", _jl(env.state[b]), fr.featurize(ks, cfg, y0[b], f["sensor_gain"][b], f["sensor_bias"][b]), ts)
    env.action.copy_(_act(env, prev, dt))
    a_prev = prev
    for t in range(fc.STEPS):
        y_in, st_in = env.y.clone(), env.state.clone()
        a_dev, ap_dev = _act(env, act[t], dt), _act(env, a_prev, dt)
        env(a_dev)
        # the split closures on the same inputs: prepare_action -> do_step -> reward_function, featurize
        p_pc = pieces.prepare_action(a_dev)
        y_pc, _ = pieces.do_step(y_in, p_pc)
        r_pc = pieces.reward_function(y_pc, a_dev, ap_dev)
        s_pc = pieces.featurize(y_pc, st_in)
        torch.cuda.synchronize()
        assert env.done.tolist() == [False] * B
        assert _same(env.action, a_dev)                       # the commanded action, whatever the gains are
        for b in range(B):
            yb, sb = _np(y_in[b]), _jl(st_in[b])
            ref = fr.env_step(ks, cfg, case, yb, a_prev[b], act[t][b], *_rows(f, b), prev_state=sb, p=_np(env.p[b]))
            assert np.isfinite(ref["y"]).all() and np.abs(ref["y"]).max() < 6.0
            ok &= _err(worst, "p", _np(env.p[b]), ref["p"], kc.tol_p(prec, ref["p"]))
            ok &= _err(worst, "p_pieces", _np(p_pc[b]), ref["p"], kc.tol_p(prec, ref["p"]))
            ty = kc.tol_y(prec, case, ref["y"])
            ok &= _err(worst, "y", _np(env.y[b]), ref["y"], ty)
            ok &= _err(worst, "y_pieces", _np(y_pc[b]), kc.oracle_step(ks, cfg, case, yb, _np(p_pc[b])), ty)
            # sensing at the device's own new field
            for name, y_dev, s_dev, r_dev in (("", env.y[b], env.state[b], env.reward[b]), ("_pieces", y_pc[b], s_pc[b], r_pc[b])):
                y_new = _np(y_dev)
                ymax = float(np.abs(y_new).max())
                ts, tr = fc.tol_state(prec, case, g, ymax, gmax[b], bmax[b]), kc.tol_reward(prec, case, g, ymax)
                s_ref = fr.featurize(ks, cfg, y_new, f["sensor_gain"][b], f["sensor_bias"][b], sb)
                ok &= _err(worst, "state" + name, _jl(s_dev), s_ref, ts)
                r_ref = ks.reward_function(cfg, y_new, act[t][b][None], (act[t][b] - a_prev[b])[None])
                ok &= _err(worst, "reward" + name, _np(r_dev), r_ref, tr)
        a_prev = act[t]
    print(f"[ks-faults step {case} {prec}{' ' + form if form else ''}] (worst, bound):", worst)
    assert ok, worst
    env.close(), pieces.close()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", fc.STEP_ROWS)
def test_step_and_pieces_match_the_reference(pkg, case, prec):
    """three teacher-forced control steps of the fused step, and the split closures at the same inputs: every trajectory against
    the reference with ITS rows of the three arrays"""
    _step_body(pkg, case, prec)


@pytest.mark.parametrize("form", ["share", "member"])
def test_simd_sharing_form_and_member_layout(pkg, form):
    """the same on the fp32 256-cell row in the 64-VGPR form of the step and with one trajectory per work-group"""
    _step_body(pkg, "perm_oddA_256", "f32", form)


# ------------------------------------------------------------------ 2. ones and zeros are the healthy run, bit for bit
def _three_steps(env, act, prev, dt):
    env.reset()
    env.action.copy_(_act(env, prev, dt))
    rows = []
    for t in range(act.shape[0]):
        env(_act(env, act[t], dt))
        rows.append((env.y.clone(), env.p.clone(), env.state.clone(), env.reward.clone(), env._done_flags.clone()))
    torch.cuda.synchronize()
    return rows


IDENTITY = [("perm_oddA_256", "f64", ""), ("perm_oddA_256", "f32", ""), ("perm_oddA_256", "f32", "share"),
            ("perm_oddA_256", "f32", "member"), ("generic_60", "f64", ""), ("stack2_perm_256", "f32", ""),
            ("fd_perm_256", "f32", ""), ("fd_midpoint_100", "f64", "")]


@pytest.mark.parametrize("with_mu", [False, True])
@pytest.mark.parametrize("case,prec,form", IDENTITY)
def test_healthy_arrays_are_bit_for_bit_nothing_set(pkg, case, prec, form, with_mu):
    """gains of one and a bias of zero against an environment that never had arrays: y, p, state, reward and flags of three
    steps as bits -- the fused step in both CNAB2 forms, both finite-difference kernels, the general featurize path -- and once
    more with a disturbance array set on both.  Then one array alone (the others NULL), and all NULL again."""
    dt = _dt(prec)
    setup, cfg, f, g = _row(pkg, case, prec)
    B = fc.batch(case)
    y0, act, prev = kc.inputs(case, B, steps=fc.STEPS)
    y0, act, prev = _cast(y0, prec), _cast(act, prec), _cast(prev, prec)
    envs = [pkg.PDEenv(setup, B=B, dtype=dt, y0=y0, autoreset=False) for _ in range(2)]
    for e in envs:
        if form == "share":
            assert e.set_simd_sharing(True)
        if form == "member":
            _member_layout(pkg, e)
        if with_mu:
            e.set_disturbance(np.array([0.05, -0.05, 0.15, 0.0, 0.1][:B]))
    envs[0].set_faults(**fc.healthy(case))
    a, b = _three_steps(envs[0], act, prev, dt), _three_steps(envs[1], act, prev, dt)
    for t in range(fc.STEPS):
        for k, name in enumerate(("y", "p", "state", "reward", "flags")):
            assert _same(a[t][k], b[t][k]), (t, name)
    # each array alone at its healthy value, the other two NULL
    for k, v in fc.healthy(case).items():
        envs[0].set_faults(**{k: v})
        assert [getattr(envs[0], n) is None for n in fc.KEYS] == [n != k for n in fc.KEYS]
        c = _three_steps(envs[0], act[:1], prev, dt)
        assert all(_same(c[0][i], b[0][i]) for i in range(5)), k
    # while the faults are set they act; all None afterwards is the healthy environment again
    envs[0].set_faults(**f)
    c = _three_steps(envs[0], act[:1], prev, dt)
    assert not _same(c[0][0], b[0][0]) and not _same(c[0][2], b[0][2])
    envs[0].set_faults()
    assert envs[0].actuator_gain is None and envs[0].sensor_gain is None and envs[0].sensor_bias is None
    c = _three_steps(envs[0], act[:1], prev, dt)
    assert all(_same(c[0][i], b[0][i]) for i in range(5))
    for e in envs:
        e.close()


@pytest.mark.parametrize("with_mu", [False, True])
@pytest.mark.parametrize("prec", PRECS)
def test_healthy_arrays_in_the_persistent_rollout(pkg, monkeypatch, prec, with_mu):
    """ks_rollout_kernel<.., FLT> with ones and zeros against ks_rollout_kernel: every logged row, reward_sum and the final y,
    state and action as bits"""
    monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", "1")
    dt, B, T = _dt(prec), 5, fc.ROLL_T
    setup, y0, dims, P, A = _ks_roll_setup(pkg, prec, B)
    actor = pkg.HipMLP(dims, ["relu", "tanh"], P, dtype=dt, max_cols=B * A)
    outs, envs = [], []
    for faulty in (True, False):
        env = pkg.PDEenv(setup, B=B, dtype=dt, y0=y0, autoreset=False)
        if with_mu:
            env.set_disturbance(np.array([0.05, -0.05, 0.15, 0.0, 0.1]))
        if faulty:
            env.set_faults(**fc.healthy(fc.ROLL_CASE))
            env.reset()
        outs.append(_profiled_rollout(pkg, env, actor, T, 1))
        envs.append(env)
    for k in ("y", "p", "action", "reward", "reward_sum", "done_step"):
        assert _same(outs[0][k], outs[1][k]), k
    assert _same(envs[0].y, envs[1].y) and _same(envs[0].state, envs[1].state) and _same(envs[0].action, envs[1].action)
    for e in envs:
        e.close()


# ------------------------------------------------------------------ 3. rollouts
def _ks_roll_setup(pkg, prec, B, seed=3):
    setup, cfg, f, g = _row(pkg, fc.ROLL_CASE, prec)
    ns, A = setup.state_shape
    y0 = _cast(kc.inputs(fc.ROLL_CASE, B, seed=seed)[0], prec)
    dims, P = _actor_params(ns, kc.roll_h(fc.ROLL_CASE), 11)
    return setup, y0, dims, P, A


def _profiled_rollout(pkg, env, actor, T, launches, **kw):
    """env.rollout (learning, noise 0.3, logged) and how many ks_rollout launches it made"""
    L = pkg._lib
    L.check(env.lib.pdec_prof_reset(env.handle))
    L.check(env.lib.pdec_prof_enable(env.handle, 1))
    out = env.rollout(actor, T, act_noise=0.3, act_limit=1.0, learning=True, seed=99, offset=0, log=True, **kw)
    torch.cuda.synchronize()
    ms, n = C.c_double(), C.c_int()
    assert env.lib.pdec_prof_get(env.handle, b"ks_rollout", C.byref(ms), C.byref(n)) == 0
    assert n.value == launches
    L.check(env.lib.pdec_prof_enable(env.handle, 0))
    return out


@pytest.mark.parametrize("control_from", [0, fc.ROLL_FROM])
@pytest.mark.parametrize("prec", PRECS)
def test_persistent_rollout_equals_the_step_loop_with_faults_set(pkg, monkeypatch, prec, control_from):
    """ks_rollout_kernel<.., FLT> (solo form) against the enqueued step loop of the same Philox stream, both environments holding
    the same arrays: ROLL_T steps, learning, noise 0.3.  The arrays add nothing to the launch's LDS (the applied action stands in
    the reward row, the faulty dots in the partial sums' place), so the row the healthy kernel serves stays served: one
    ks_rollout launch.  control_from = 3: the uncontrolled steps apply a zero forcing whatever the gains are."""
    dt, T, B = _dt(prec), fc.ROLL_T, 5
    setup, y0, dims, P, A = _ks_roll_setup(pkg, prec, B)
    f = _row(pkg, fc.ROLL_CASE, prec)[2]
    actor = pkg.HipMLP(dims, ["relu", "tanh"], P, dtype=dt, max_cols=B * A)
    outs, envs = [], []
    for persistent in ("1", "0"):
        monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", persistent)
        env = pkg.PDEenv(setup, B=B, dtype=dt, y0=y0, autoreset=False)
        env.set_faults(**f)
        env.reset()
        outs.append(_profiled_rollout(pkg, env, actor, T, 1 if persistent == "1" else 0, control_from=control_from))
        envs.append(env)
    sc = 1e-6 if prec == "f64" else 1.0
    worst, ok = {}, True
    d = lambda x, y: _np(x) - _np(y)
    for k, tol in (("y", 2e-5), ("p", 2e-4), ("action", 2e-5), ("reward", 2e-5), ("reward_sum", 2e-5)):
        ok &= _err(worst, k, d(outs[0][k], outs[1][k]), 0, tol * sc)
    ok &= _err(worst, "y_end", d(envs[0].y, envs[1].y), 0, 2e-5 * sc)
    ok &= _err(worst, "state_end", d(envs[0].state, envs[1].state), 0, 2e-5 * sc)
    print(f"[ks-faults rollout {prec} control_from={control_from}] (worst, bound):", worst)
    assert ok, worst
    assert outs[0]["done_step"].tolist() == [-1] * B
    for o in outs:
        if control_from:
            assert float(o["action"][:control_from].abs().max()) == 0.0 and float(o["p"][:control_from].abs().max()) == 0.0
        # the logs hold the commanded action, p the forcing the gains made of it
        t = control_from
        for b in (0, fc.HEALTHY):
            want = pkg.PDEenv.prepare_action(envs[1], o["action"][t])[b]
            assert float((o["p"][t, b] - want).abs().max()) <= 2e-4 * sc * max(1.0, float(want.abs().max())), b
    # the faults act: the same launch without them is elsewhere by the last step, the healthy trajectory's first step is not
    monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", "1")
    plain = pkg.PDEenv(setup, B=B, dtype=dt, y0=y0, autoreset=False)
    out = plain.rollout(actor, T, act_noise=0.3, act_limit=1.0, learning=True, seed=99, offset=0, log=True, control_from=control_from)
    assert float((out["y"][-1, 0] - outs[0]["y"][-1, 0]).abs().max()) > 1e-3
    assert float((out["y"][0, fc.HEALTHY] - outs[0]["y"][0, fc.HEALTHY]).abs().max()) <= 2e-5 * sc
    plain.close()
    for e in envs:
        e.close()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", fc.STEP_ROWS + ("narrow_256", "irregular_256", "sparse_240"))
def test_the_arrays_do_not_change_what_the_persistent_launch_serves(pkg, monkeypatch, case, prec):
    """rollout_lds counts nothing for the arrays: with them set, a row is served by ks_rollout_kernel exactly when the restated
    ks_rollout_shape_ok of ks_geometry_cases.py says the healthy row is -- perm_oddA_256 in fp64 stands at 63.4 of 64 KiB"""
    monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", "1")
    from oracle import ks
    dt = _dt(prec)
    setup, cfg = kc.build(pkg, ks, case)
    geo = kc.geometry(*setup.tables(), case, prec)
    ns, A = setup.state_shape
    B = 3
    dims, P = _actor_params(ns, kc.roll_h(case), 11)
    actor = pkg.HipMLP(dims, ["relu", "tanh"], P, dtype=dt, max_cols=B * A)
    served = kc.rollout_served(geo, case, prec)
    for arrays in (False, True):
        env = pkg.PDEenv(setup, B=B, dtype=dt, y0=_cast(kc.inputs(case, B, seed=3)[0], prec), autoreset=False)
        if arrays:
            env.set_faults(actuator_gain=np.full((B, A), 0.5), sensor_gain=np.full((B, setup.n_sensors), 1.2),
                           sensor_bias=np.full((B, setup.n_sensors), 0.25))
        _profiled_rollout(pkg, env, actor, 1, 1 if served else 0)
        env.close()
    if case == fc.ROLL_CASE:
        assert served


@pytest.mark.parametrize("case", ["stack2_perm_256", "fd_perm_256"])
def test_rows_the_persistent_launch_does_not_serve_take_the_step_loop(pkg, case):
    """a temporal stack and the finite-difference kernels: env.rollout with arrays set is the enqueued step loop, bit for bit the
    loop made by hand (pdec_policy_act_rng -> (env)(action)) on an environment with the same arrays"""
    L = pkg._lib
    prec, dt, T, B, noise, seed = "f32", torch.float32, 4, fc.batch(case), 0.3, 99
    setup, cfg, f, g = _row(pkg, case, prec)
    ns, A = setup.state_shape
    y0 = _cast(kc.inputs(case, B, seed=3)[0], prec)
    dims, P = _actor_params(ns, 20, 11)
    actor = pkg.HipMLP(dims, ["relu", "tanh"], P, dtype=dt, max_cols=B * A)
    env, ref = (pkg.PDEenv(setup, B=B, dtype=dt, y0=y0, autoreset=False) for _ in range(2))
    for e in (env, ref):
        e.set_faults(**f)
        e.reset()
    out = _profiled_rollout(pkg, env, actor, T, 0)
    cols = B * A
    for t in range(T):
        a = torch.zeros(ref._ashape, dtype=dt, device="cuda:0")
        L.check(ref.lib.pdec_policy_act_rng(actor.handle, L.ptr(ref.state), cols, noise, 1.0, 1, seed, t * ((cols + 3) // 4), L.ptr(a)))
        ref(a)
        torch.cuda.synchronize()
        for name, want in (("y", ref.y), ("p", ref.p), ("action", ref.action), ("reward", ref.reward)):
            assert _same(out[name][t], want), (t, name)
    assert _same(env.state, ref.state)
    env.close(), ref.close()


# ------------------------------------------------------------------ 4. evaluate_actors over scenarios
def _scenarios(setup, A, S):
    return [setup.fault_scenario(),
            setup.fault_scenario(dead_actuators=(1, 4, A), dead_sensors=(17,)),
            setup.fault_scenario(actuator_gain=np.where(np.arange(A) % 3 == 0, -1.0, 0.5), sensor_gain=np.full(S, 1.2),
                                 sensor_bias=np.where(np.arange(S) % 2 == 0, 0.5, -0.25))]


@pytest.mark.parametrize("persistent", ["1", "0"])
def test_evaluate_actors_over_scenarios(pkg, monkeypatch, persistent):
    """faults = [healthy, two others], M = 3, K = 3 on perm_oddA_256: one launch of M n_f ceil(K / 2) work-groups; every (member,
    scenario) block bit for bit the single-scenario call and the solo rollout on an environment with that scenario set; the healthy
    block bit for bit the call without faults.  persistent = 0: the member-by-member form, the same numbers."""
    monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", persistent)
    prec, dt, M, K, T = "f64", torch.float64, 3, 3, 6
    setup, y0, dims, P, A = _ks_roll_setup(pkg, prec, K, seed=5)
    S = setup.n_sensors
    y0 = to_dev(y0, dt)
    actors = [pkg.HipMLP(dims, ["relu", "tanh"], _actor_params(dims[0], dims[1], 100 + m)[1], dtype=torch.float32, max_cols=K * A)
              for m in range(M)]
    scen = _scenarios(setup, A, S)
    nf = len(scen)
    res = pkg.evaluate_actors(setup, actors, y0=y0, dtype=dt, steps=T, log=True, faults=scen)
    assert res["one_launch"] is (persistent == "1")
    if persistent == "1":
        assert res["workgroups"] == M * nf * ((K + 1) // 2)
    assert res["episode_reward"].shape == (M, nf, K) and res["reward_sum"].shape == (M, nf, K, A) and res["done_step"].shape == (M, nf, K)
    assert res["score"].shape == (M, nf) and res["y"].shape[:4] == (T, M, nf, K) and "mu" not in res
    assert len(res["faults"]) == nf and all(np.array_equal(res["faults"][i][k], scen[i][k]) for i in range(nf) for k in fc.KEYS)
    assert np.isfinite(res["score"]).all()
    mean = res["score"].mean(axis=1)
    assert res["order"] == sorted(range(M), key=lambda m: (-mean[m], m))
    for i, sc in enumerate(scen):
        one = pkg.evaluate_actors(setup, actors, y0=y0, dtype=dt, steps=T, log=True, faults=[sc])
        assert one["episode_reward"].shape == (M, 1, K)
        for k in ("episode_reward", "reward_sum", "done_step"):
            assert _same(res[k][:, i], one[k][:, 0]), (i, k)
        for k in ("y", "p", "action", "reward"):
            assert _same(res[k][:, :, i], one[k][:, :, 0]), (i, k)
        assert np.array_equal(res["score"][:, i], one["score"][:, 0])
        for m, actor in enumerate(actors):
            env = pkg.PDEenv(setup, B=K, dtype=dt, y0=y0, autoreset=False)
            env.set_faults(**{k: np.tile(sc[k], (K, 1)) for k in fc.KEYS})
            env.reset()
            solo = env.rollout(actor.clone(dtype=dt, max_cols=K * A), T, learning=False, log=True)
            torch.cuda.synchronize()
            for k in ("y", "p", "action", "reward"):
                assert _same(res[k][:, m, i], solo[k]), (i, m, k)
            assert _same(res["reward_sum"][m, i], solo["reward_sum"])
            env.close()
    assert not _same(res["y"][:, :, 0], res["y"][:, :, 1]) and not _same(res["y"][:, :, 1], res["y"][:, :, 2])
    # faults = None: today's keys and shapes, and the healthy block is that call
    plain = pkg.evaluate_actors(setup, actors, y0=y0, dtype=dt, steps=T, log=True)
    assert "faults" not in plain and plain["episode_reward"].shape == (M, K) and plain["score"].shape == (M,)
    for k in ("y", "p", "action", "reward"):
        assert _same(res[k][:, :, 0], plain[k]), k
    assert _same(res["reward_sum"][:, 0], plain["reward_sum"]) and np.array_equal(res["score"][:, 0], plain["score"])
    # a NaN under one scenario (a forcing that is not a number: the field is not, the blow-up flag rises) is a NaN of the member's mean
    bad = [scen[0], dict(actuator_gain=np.full(A, np.nan))]
    res2 = pkg.evaluate_actors(setup, [actors[0]], y0=y0, dtype=dt, steps=2, faults=bad)
    assert np.isnan(res2["score"][0, 1]) and np.isfinite(res2["score"][0, 0]) and res2["order"] == [0]


# ------------------------------------------------------------------ 5. the reset image and the episode clock
@pytest.mark.parametrize("prec", PRECS)
def test_a_per_trajectory_reset_restores_the_state_the_faulty_sensors_see(pkg, prec):
    """set_faults refreshes the reset image from y0 through the arrays and touches neither y nor state nor action; trajectory 1
    patched past max_value restarts in its step with that image, bit for bit pdec_featurize of y0"""
    case, dt = "perm_oddA_256", _dt(prec)
    setup, cfg, f, g = _row(pkg, case, prec)
    B = fc.batch(case)
    y0, act, prev = kc.inputs(case, B, steps=1, seed=7)
    y0, act, prev = _cast(y0, prec), _cast(act, prec), _cast(prev, prec)
    env = pkg.PDEenv(setup, B=B, dtype=dt, y0=y0, autoreset=True)
    before = (env.y.clone(), env.state.clone(), env.action.clone(), env._state0.clone())
    env.set_faults(**f)
    torch.cuda.synchronize()
    assert _same(env.y, before[0]) and _same(env.state, before[1]) and _same(env.action, before[2])
    want = env.featurize(env.y0)
    assert _same(env._state0, want) and not _same(env._state0, before[3])
    assert _same(env._state0[fc.HEALTHY], before[3][fc.HEALTHY])
    env.action.copy_(_act(env, prev, dt))
    env.y[0, -3:] = kc.BLOWUP_PATCH
    env(_act(env, act[0], dt))
    torch.cuda.synchronize()
    assert env.done.tolist() == [True] + [False] * (B - 1)
    assert _same(env.y[0], env.y0[0]) and _same(env.state[0], want[0]) and not _same(env.state[2], want[2])
    env.close()


def _padded(shape, dtype, fill=None):
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * PAD,), CANARY, dtype=dtype, device="cuda")
    view = flat[PAD:PAD + n].view(shape)
    if fill is not None:
        view.copy_(fill)
    return flat, view


@pytest.mark.parametrize("prec", PRECS)
def test_the_episode_clock_restarts_through_the_sensor_faults(pkg, prec):
    """pdec_epclock_step with random initial fields on canary-padded buffers, KS22, B = 6, episodes of 4 steps: a trajectory that
    ends (a blow-up flag at call 1, the time-out at call 3) gets a new field and the state pdec_featurize makes of that field
    through ITS sensor faults, bit for bit; the rows of the others and the canaries stand"""
    L = pkg._lib
    dt, B, E = _dt(prec), 6, 4
    setup = pkg.KSSetup.KS22()
    A, S = setup.n_actuators, setup.n_sensors
    rng = np.random.default_rng(5)
    f = dict(actuator_gain=rng.uniform(-1, 1.5, (B, A)), sensor_gain=rng.uniform(0, 2, (B, S)), sensor_bias=rng.uniform(-2, 2, (B, S)))
    for k in fc.KEYS:
        f[k][fc.HEALTHY] = fc.HEALTHY_VALUE[k]
    s = torch.cuda.Stream()
    env = pkg.PDEenv(setup, B=B, dtype=dt, stream=s, autoreset=False)
    env.set_faults(**f)
    h = L.Handle()
    L.check(env.lib.pdec_epclock_create(C.byref(h), env.handle, E, 2, 1, 11, 0, 1))
    npdt = np.float32 if prec == "f32" else np.float64
    try:
        for call, rows in enumerate(([], [0, B - 1], [], list(range(1, B - 1)))):
            flags_h = np.zeros(B, dtype=np.int32)
            if call == 1:
                flags_h[rows] = 1
            host = dict(reward=-rng.uniform(0, 9, (B, A)).astype(npdt), terminal=np.zeros((B, A), npdt),
                        action=rng.uniform(-1, 1, env._ashape).astype(npdt), aprev=rng.uniform(-1, 1, env._ashape).astype(npdt),
                        y=rng.standard_normal(env._yshape).astype(npdt), state=rng.standard_normal(env._sshape).astype(npdt))
            with torch.cuda.stream(s):
                dev = {k: _padded(v.shape, dt, torch.as_tensor(v)) for k, v in host.items()}
                flags = torch.as_tensor(flags_h).cuda()
                L.check(env.lib.pdec_epclock_step(h, L.ptr(dev["reward"][1]), L.ptr(flags), L.ptr(dev["terminal"][1]), L.ptr(dev["action"][1]),
                                                  L.ptr(dev["aprev"][1]), L.ptr(dev["y"][1]), L.ptr(dev["state"][1]), None, None))
                seen = env.featurize(dev["y"][1])            # pdec_featurize of the fields the call left, through the arrays
            torch.cuda.synchronize()
            ended = sorted(np.flatnonzero(dev["terminal"][1][:, 0].cpu().numpy() != 0).tolist())
            assert ended == rows, (call, ended)
            y_dev, s_dev = dev["y"][1], dev["state"][1]
            for b in range(B):
                if b in rows:
                    assert not np.array_equal(y_dev[b].cpu().numpy(), host["y"][b])
                    assert _same(s_dev[b], seen[b]), (call, b)
                else:
                    assert np.array_equal(y_dev[b].cpu().numpy(), host["y"][b]) and np.array_equal(s_dev[b].cpu().numpy(), host["state"][b])
            for k, (flat, view) in dev.items():
                assert bool((flat[:PAD] == CANARY).all()) and bool((flat[-PAD:] == CANARY).all()), (call, k)
            if rows:
                # ... and they are the faulty sensors: the healthy environment's features of the same fields differ, except on
                # the healthy trajectory
                env.set_faults()
                with torch.cuda.stream(s):
                    plain = env.featurize(y_dev)
                torch.cuda.synchronize()
                env.set_faults(**f)
                for b in rows:
                    assert _same(plain[b], s_dev[b]) == (b == fc.HEALTHY), (call, b)
    finally:
        env.lib.pdec_destroy(h)
    env.close()


def _pipe(pkg, B, E, graphs, f, **kw):
    setup = pkg.KSSetup.KS22()
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    y0 = setup.generate_random_init(np.random.default_rng(0), B) * 0.15
    env = pkg.PDEenv(setup, B=B, dtype=torch.float32, y0=y0, stream=s_env, autoreset=False)
    if f is not None:
        env.set_faults(**f)
    agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                             noise_seed=7, trajectory_length=1)
    agent.policy.act_noise = 0.3
    torch.cuda.synchronize()
    return pkg.TrainPipeline(env, agent, lag=2, episode_steps=E, stream_env=s_env, stream_upd=s_upd, use_graphs=graphs,
                             chunks=(6, 1), noise_seed=99, **kw)


def _ks22_faults(B, seed=5):
    setup_A = setup_S = 8
    rng = np.random.default_rng(seed)
    f = dict(actuator_gain=rng.uniform(-1, 1.5, (B, setup_A)), sensor_gain=rng.uniform(0, 2, (B, setup_S)),
             sensor_bias=rng.uniform(-2, 2, (B, setup_S)))
    for k in fc.KEYS:
        f[k][fc.HEALTHY] = fc.HEALTHY_VALUE[k]
    f["actuator_gain"][0, :2] = 0.0
    return f


def test_the_pipelines_episode_clock_restarts_through_the_sensor_faults(pkg):
    """TrainPipeline(episodes="per_trajectory", random_init), B = 6, episode_steps = 4, staggered, stepped with the device drained:
    the state row of every trajectory that restarted in a step is bit for bit pdec_featurize of its new field through the arrays
    the environment holds"""
    B, E = 6, 4
    f = _ks22_faults(B)
    p = _pipe(pkg, B, E, False, f, episodes="per_trajectory", stagger=True, random_init=True, init_seed=3, log_episodes=4)
    p.drain_between = True
    restarted = 0
    for _ in range(3 * E):
        k = p.tick
        p.step()
        torch.cuda.synchronize()
        ended = np.flatnonzero(p.tring[k % 3][:, 0].cpu().numpy() != 0)
        y, s = p.ybuf[(k + 1) % 2], p.sring[(k + 1) % 6]
        with torch.cuda.stream(p.s_env):
            seen = p.env.featurize(y)
        torch.cuda.synchronize()
        for b in ended:
            assert _same(s[b], seen[b]), (k, b)
        restarted += len(ended)
        assert bool(torch.isfinite(p.y).all())
    assert restarted >= 2 * B
    p.close()


# ------------------------------------------------------------------ 6. the training pipeline
def _adam(nna):
    m = nna.model
    k = sum(int(np.asarray(x).size) for x in m.params())
    a, b, bp = (C.c_float * k)(), (C.c_float * k)(), (C.c_double * 2)()
    assert m.lib.pdec_adam_get_state(m.handle, a, b, bp) == 0
    return bytes(a), bytes(b), bytes(bp)


def _same_learner(p, q):
    assert _same(p.y, q.y) and _same(p.state, q.state)
    for nm in NETS:
        for x, y in zip(getattr(p.policy, nm).model.params(), getattr(q.policy, nm).model.params()):
            assert np.array_equal(x, y), nm
    for nm in ("behavior_actor", "behavior_critic"):
        assert _adam(getattr(p.policy, nm)) == _adam(getattr(q.policy, nm)), nm


@pytest.mark.parametrize("E", [6, 13])
def test_train_pipeline_steps_through_the_faults_the_environment_holds(pkg, E):
    """KS22, B = 6, lag 2, two episodes on an environment with arrays set: steps issued one by one with the device drained (eager),
    replayed from the recorded library calls, and (E = 13) launched from captured graphs of six steps leave y, the state, the four
    networks and the ADAM moments equal as bits -- and not those of the run without arrays.  Then new values are written into the
    arrays between two run() calls: the recorded calls and the graphs stay, and the next steps read the new values, again the same
    bits on all three routes."""
    B = 6
    f = _ks22_faults(B)
    pe, pr, pg, p0 = _pipe(pkg, B, E, False, f), _pipe(pkg, B, E, False, f), _pipe(pkg, B, E, True, f), _pipe(pkg, B, E, False, None)
    pe.drain_between = True
    if E > 12:
        pg.run(5)
        pg.capture()
        pe.run(pg.tick), pr.run(pg.tick), p0.run(pg.tick)
    for p in (pe, pr, pg, p0):
        p.run(2 * E)
        p.sync()
    assert pe.tick == pr.tick == pg.tick == p0.tick and (pg.n_graph_launches > 0) == (E > 12)
    assert len(pr._progs) > 0 and len(pe._progs) == 0
    _same_learner(pe, pr), _same_learner(pe, pg)
    assert bool(torch.isfinite(pg.y).all()) and float((pe.y - p0.y).abs().max()) > 1e-3
    # a fault that appears mid-run: trajectory 2 loses every actuator, sensor 3 of trajectory 4 gets an offset
    progs, graphs, launches = dict(pr._progs), dict(pg.graphs) if E > 12 else None, pg.n_graph_launches
    for p in (pe, pr, pg):
        with torch.cuda.stream(p.s_env):
            p.env.actuator_gain[2].zero_()
            p.env.sensor_bias[4, 2] = 1.5
    for p in (pe, pr, pg, p0):
        p.run(E)
        p.sync()
    assert pr._progs == progs and (E <= 12 or (pg.graphs == graphs and pg.n_graph_launches > launches))
    _same_learner(pe, pr), _same_learner(pe, pg)
    # the new values were read: trajectory 2's forcing is zero in the last step (p of the step = prepare_action of its action)
    with torch.cuda.stream(pr.s_env):
        forcing = pr.env.prepare_action(pr.aring[(pr.tick - 1) % 3])
    torch.cuda.synchronize()
    assert float(forcing[2].abs().max()) == 0.0 and float(forcing[3].abs().max()) > 0.0
    # and a control: the same run without the write ends elsewhere
    pc = _pipe(pkg, B, E, False, f)
    pc.run(pr.tick)
    pc.sync()
    assert float((pc.y - pr.y).abs().max()) > 1e-4
    for p in (pe, pr, pg, p0, pc):
        p.close()


# ------------------------------------------------------------------ 7. refusals, by name
def test_refusals(pkg):
    from oracle import ks
    mono, _ = kc.build(pkg, ks, "mono_256")
    rows = [(mono, 5, "mono"), (pkg.KSSetup.KS22(memory_size=2), 3, "memory_size"), (pkg.KellerSegelSetup(), 3, "Keller-Segel"),
            (pkg.KellerSegel2DSetup(nx=64, ny=64), 2, "2-D Keller-Segel"),
            (pkg.FluidSetup(nx=32, sensors_per_axis=4, oversampling=2), 2, "fluid")]
    for setup, B, word in rows:
        env = pkg.PDEenv(setup, B=B, dtype=torch.float64, autoreset=False)
        one = torch.ones((B, 1), dtype=torch.float64, device="cuda:0")
        for name in fc.KEYS:                                   # each array alone is refused, by the library, by name
            rc = env.lib.pdec_env_set_faults(env.handle, *[pkg._lib.ptr(one) if k == name else None for k in fc.KEYS])
            assert rc != 0 and word.encode() in env.lib.pdec_last_error() and b"pdec_env_set_faults" in env.lib.pdec_last_error(), (word, name)
        # and so is PDEenv.set_faults, by the library's name for the environment, whatever shape the arrays have
        for shape in ((B, setup.state_shape[1]), (B, 1), (3,)):
            with pytest.raises(pkg.PdecError, match=word):
                env.set_faults(actuator_gain=np.ones(shape))
        assert env.actuator_gain is None
        before = env._state0.clone()
        env._state0.fill_(7.0)
        assert env.lib.pdec_env_set_faults(env.handle, None, None, None) == 0      # nothing to return from: accepted
        env.set_faults()
        torch.cuda.synchronize()
        assert env.actuator_gain is None and bool((env._state0 == 7.0).all())      # healthy before and after: no launch
        env._state0.copy_(before)
        env.close()
    setup, cfg, f, g = _row(pkg, "perm_oddA_256", "f64")
    A, S = fc.sizes("perm_oddA_256")
    env = pkg.PDEenv(setup, B=5, dtype=torch.float64, autoreset=False)
    for kw, word in ((dict(actuator_gain=np.ones((5, S))), "actuator_gain"), (dict(actuator_gain=np.ones(A)), "actuator_gain"),
                     (dict(sensor_gain=np.ones((5, A))), "sensor_gain"), (dict(sensor_gain=np.ones((4, S))), "sensor_gain"),
                     (dict(sensor_bias=np.zeros((5, S, 1))), "sensor_bias")):
        with pytest.raises(pkg.PdecError, match=word):
            env.set_faults(**kw)
    assert env.actuator_gain is None and env.sensor_gain is None and env.sensor_bias is None
    # a wrong shape leaves the arrays of before in place, in the library too
    env.set_faults(**f)
    kept = env.sensor_gain
    with pytest.raises(pkg.PdecError, match="sensor_bias"):
        env.set_faults(sensor_bias=np.zeros((5, A)))
    assert env.sensor_gain is kept
    ref = pkg.PDEenv(setup, B=5, dtype=torch.float64, autoreset=False)
    ref.set_faults(**f)
    assert _same(env.featurize(env.y0), ref.featurize(ref.y0)) and not _same(env.featurize(env.y0), env.state)
    env.close(), ref.close()
    # a launch sync with arrays set: refused by name (the synchronised step has no fault-carrying form)
    s22 = pkg.KSSetup.KS22()
    env = pkg.PDEenv(s22, B=1, dtype=torch.float64, autoreset=False)
    env.set_faults(actuator_gain=np.full((1, 8), 0.5))
    flag = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    pkg._lib.check(env.lib.pdec_set_launch_sync(env.handle, None, 0, pkg._lib.ptr(flag[1:2]), 1))
    with pytest.raises(pkg.PdecError, match="pdec_env_set_faults"):
        env(torch.zeros(env._ashape, dtype=torch.float64, device="cuda:0"))
    env(torch.zeros(env._ashape, dtype=torch.float64, device="cuda:0"))          # the refused call consumed the sync
    torch.cuda.synchronize()
    assert int(flag[1]) == 0
    from importlib import import_module
    assert not import_module(pkg.__name__ + ".run")._launch_sync_ok(env)
    env.set_faults()
    assert import_module(pkg.__name__ + ".run")._launch_sync_ok(env)
    env.close()
    actor = pkg.HipMLP([3, 4, 1], ["relu", "tanh"], _actor_params(3, 4, 1)[1], dtype=torch.float32, max_cols=64)
    with pytest.raises(pkg.PdecError, match="faults together with mu"):
        pkg.evaluate_actors(setup, [actor], n_inits=2, steps=2, faults=[setup.fault_scenario()], mu=[0.0])
    with pytest.raises(pkg.PdecError, match="KS setups only"):
        pkg.evaluate_actors(pkg.KellerSegelSetup(), [actor], n_inits=2, steps=2, faults=[dict()])
