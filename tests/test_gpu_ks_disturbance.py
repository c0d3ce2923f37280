"""Per-trajectory KS disturbance (pdec_env_set_disturbance) and delayed control (pdec_env_set_control_from) on the device:
ks_env_step_kernel<.., MU> with four FFT engines, its split form, its SIMD-sharing form and the member layout, ks_rollout_kernel
in its solo and member forms, ksfd_wave_step_kernel and ksfd_env_step_kernel with both integrators, kseg_rollout_kernel and the
enqueued step loop of csrc/rollout.hip, and the Python layers above them (PDEenv.set_disturbance, PDEenv.rollout(control_from),
evaluate_actors(mu, control_from), TrainPipeline on an environment that holds an amplitude array).

The reference is oracle/ks.py with ONE KSConfig per trajectory (cfg.mu = mu[b]; ks_disturbance_cases.configs); fp32 inputs are
rounded once and the oracle runs in fp64 from those values.  test_ks_disturbance_table.py shows without a GPU that the inputs are
tame and that a swapped, a neighbour's or the batch's mean amplitude moves one control step by >= 30 fp32 bounds.

Tolerances: those of test_gpu_ks_geometry.py (ks_geometry_cases.tol_*), none raised -- y 1e-11 / 3e-5 max(1, |ref|) per
teacher-forced step (finite differences 1e-11 / 2e-4 max |ref|), p 1e-12 / 1e-5, state and reward from the format at the device's
own new field; a persistent rollout against the enqueued step loop 2e-11 / 2e-5 (p 2e-10 / 2e-4).  Everything stated as "bit for
bit" is compared as integers.

Worst deviation / bound on an MI355X, the row with the largest ratio (every test prints its own line):
                                  fp64                                 fp32
  fused step  p                   2.1e-14 / 1.9e-11 dense_192          6.5e-6 / 1.6e-4 dense_192
              y (also the pieces) 6.7e-15 / 1.2e-11 generic_60         2.0e-6 / 3.1e-5 generic_60
              state               1.4e-17 / 1.8e-16 fd_midpoint_100    3.7e-9 / 2.8e-8 subset_1024
              reward              4.4e-16 / 8.2e-15 fd_perm_256        3.3e-7 / 3.5e-6 fd_perm_256
  perm_oddA_256 fp32: SIMD-sharing form y 1.2e-6 / 3.4e-5, member layout y 1.6e-6 / 4.7e-5
  autoreset, the restarted trajectory's next step   y 3.1e-15 / 1.1e-11     8.0e-7 / 3.3e-5
  persistent rollout against the step loop   y 9.4e-16 / 2e-11, reward_sum 4.4e-16 / 2e-11     5.7e-7 / 2e-5, 2.4e-7 / 2e-5
  control_from, persistent against the loop given zero actions   KS y 1.0e-15 / 2e-11, 5.4e-7 / 2e-5; Keller-Segel fp64 0 / 2e-11
No quantity exceeded its bound."""
import ctypes as C

import numpy as np
import pytest

import ks_disturbance_cases as dc
import ks_geometry_cases as kc
from util import to_dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PRECS = ("f64", "f32")
ROLL_CASE = "perm_oddA_256"          # served by ks_rollout_kernel in both dtypes (ks_geometry_cases.ROLL_MUST_SERVE)


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
    """(setup, one oracle config per trajectory at the values the device holds, amplitudes, geometry) of a row, built once"""
    from oracle import ks
    key = (case, prec)
    if key not in _MEMO:
        mu = _cast(dc.amplitudes(case), prec)
        setup, cfgs = dc.configs(pkg, ks, case, mu)
        _MEMO[key] = (setup, cfgs, mu, kc.geometry(*setup.tables(), case, prec))
    return _MEMO[key]


def _act(env, a, dt):
    return to_dev(a, dt).reshape(env._ashape)


def _sense_bounds(prec, case, g, y):
    ymax = float(np.abs(y).max())
    return kc.tol_state(prec, case, g, ymax), kc.tol_reward(prec, case, g, ymax)


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


# ------------------------------------------------------------------ a. the fused step and its pieces against the per-trajectory oracle
def _step_body(pkg, case, prec, form=""):
    from oracle import ks
    dt = _dt(prec)
    setup, cfgs, mu, g = _row(pkg, case, prec)
    B = dc.batch(case)
    y0, act, prev = kc.inputs(case, B, steps=dc.STEPS)
    y0, act, prev = _cast(y0, prec), _cast(act, prec), _cast(prev, prec)
    env = pkg.PDEenv(setup, B=B, dtype=dt, y0=y0, autoreset=False)
    pieces = pkg.PDEenv(setup, B=B, dtype=dt, autoreset=False)
    if form == "share":
        assert env.set_simd_sharing(True)
    if form == "member":
        _member_layout(pkg, env)
    for e in (env, pieces):
        e.set_disturbance(mu)
        assert e.mu.dtype == dt and e.mu.shape == (B,)
    env.action.copy_(_act(env, prev, dt))
    worst, ok, a_prev = {}, True, prev
    for t in range(dc.STEPS):
        y_in, st_in = env.y.clone(), env.state.clone()
        a_dev, ap_dev = _act(env, act[t], dt), _act(env, a_prev, dt)
        env(a_dev)
        p_pc = pieces.prepare_action(a_dev)
        y_pc, _ = pieces.do_step(y_in, p_pc)
        torch.cuda.synchronize()
        assert env.done.tolist() == [False] * B
        for b in range(B):
            yb, sb = _np(y_in[b]), _jl(st_in[b])
            p_ref = ks.prepare_action(cfgs[b], act[t][b][None])
            ok &= _err(worst, "p", _np(env.p[b]), p_ref, kc.tol_p(prec, p_ref))
            y_ref = kc.oracle_step(ks, cfgs[b], case, yb, _np(env.p[b]))        # the oracle at mu[b], from the device's own inputs
            assert np.isfinite(y_ref).all() and np.abs(y_ref).max() < 6.0
            ty = kc.tol_y(prec, case, y_ref)
            ok &= _err(worst, "y", _np(env.y[b]), y_ref, ty)
            ok &= _err(worst, "y_pieces", _np(y_pc[b]), kc.oracle_step(ks, cfgs[b], case, yb, _np(p_pc[b])), ty)
            y_new = _np(env.y[b])
            ts, tr = _sense_bounds(prec, case, g, y_new)
            ok &= _err(worst, "state", _jl(env.state[b]), ks.featurize(cfgs[b], y_new, sb), ts)
            r_ref = ks.reward_function(cfgs[b], y_new, act[t][b][None], (act[t][b] - a_prev[b])[None])
            ok &= _err(worst, "reward", _np(env.reward[b]), r_ref, tr)
        a_prev = act[t]
    print(f"[ks-disturbance step {case} {prec}{' ' + form if form else ''}] (worst, bound):", worst)
    assert ok, worst
    env.close(), pieces.close()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", dc.STEP_ROWS)
def test_step_and_pieces_match_the_per_trajectory_oracle(pkg, case, prec):
    """three teacher-forced control steps of the fused step, and the split pieces prepare_action -> do_step at the same inputs:
    every trajectory against the oracle configured at ITS amplitude"""
    _step_body(pkg, case, prec)


@pytest.mark.parametrize("form", ["share", "member"])
def test_simd_sharing_form_and_member_layout(pkg, form):
    """the same on the fp32 256-cell row in the 64-VGPR form of the step (pdec_env_set_simd_sharing) and with one trajectory per
    work-group (pdec_env_set_member_layout: m0 only)"""
    _step_body(pkg, "perm_oddA_256", "f32", form)


# ------------------------------------------------------------------ b. unset again, and equal values on the finite-difference rows
def _three_steps(env, act, prev, dt):
    env.action.copy_(_act(env, prev, dt))
    rows = []
    for t in range(act.shape[0]):
        env(_act(env, act[t], dt))
        rows.append((env.y.clone(), env.p.clone(), env.state.clone(), env.reward.clone()))
    torch.cuda.synchronize()
    return rows


@pytest.mark.parametrize("case,prec,form", [("perm_oddA_256", "f64", ""), ("perm_oddA_256", "f32", ""), ("perm_oddA_256", "f32", "share"),
                                            ("perm_oddA_256", "f32", "member"), ("generic_60", "f64", ""), ("fd_perm_256", "f32", "")])
def test_unset_again_is_bit_for_bit_an_environment_that_never_had_one(pkg, case, prec, form):
    """set_disturbance(mu), one step, set_disturbance(None), reset: the next steps are bit for bit those of an environment that
    never had an array (perm_oddA_256 and fd_perm_256 have a non-zero scalar mu of their own, which comes back)"""
    dt = _dt(prec)
    setup, cfgs, mu, g = _row(pkg, case, prec)
    B = dc.batch(case)
    y0, act, prev = kc.inputs(case, B, steps=dc.STEPS)
    y0, act, prev = _cast(y0, prec), _cast(act, prec), _cast(prev, prec)
    envs = [pkg.PDEenv(setup, B=B, dtype=dt, y0=y0, autoreset=False) for _ in range(2)]
    for e in envs:
        if form == "share":
            assert e.set_simd_sharing(True)
        if form == "member":
            _member_layout(pkg, e)
    envs[0].set_disturbance(mu)
    first = _three_steps(envs[0], act[:1], prev, dt)
    envs[0].set_disturbance(None)
    assert envs[0].mu is None
    envs[0].reset()
    a, b = _three_steps(envs[0], act, prev, dt), _three_steps(envs[1], act, prev, dt)
    for t in range(dc.STEPS):
        for k, name in enumerate(("y", "p", "state", "reward")):
            assert _same(a[t][k], b[t][k]), (t, name)
    assert not _same(first[0][0], b[0][0])                 # while it was set, it acted
    for e in envs:
        e.close()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", ["fd_perm_256", "fd_irregular_256", "fd_midpoint_100"])
def test_equal_values_are_the_scalar_on_the_finite_difference_rows(pkg, case, prec):
    """an array that holds cfg.mu for everyone is bit for bit the scalar in ksfd_wave_step_kernel and ksfd_env_step_kernel"""
    dt = _dt(prec)
    setup, cfgs, mu, g = _row(pkg, case, prec)
    B = dc.batch(case)
    y0, act, prev = kc.inputs(case, B, steps=dc.STEPS)
    y0, act, prev = _cast(y0, prec), _cast(act, prec), _cast(prev, prec)
    envs = [pkg.PDEenv(setup, B=B, dtype=dt, y0=y0, autoreset=False) for _ in range(2)]
    envs[0].set_disturbance(np.full(B, kc.CASES[case].mu))
    a, b = _three_steps(envs[0], act, prev, dt), _three_steps(envs[1], act, prev, dt)
    for t in range(dc.STEPS):
        for k, name in enumerate(("y", "p", "state", "reward")):
            assert _same(a[t][k], b[t][k]), (t, name)
    envs[0].set_disturbance(mu)                            # and other values are not
    c = _three_steps(envs[0], act[:1], act[-1], dt)
    envs[1].set_disturbance(np.full(B, kc.CASES[case].mu))
    d = _three_steps(envs[1], act[:1], act[-1], dt)
    assert not _same(c[0][0], d[0][0])
    for e in envs:
        e.close()


# ------------------------------------------------------------------ c. autoreset keeps the amplitude
@pytest.mark.parametrize("prec", PRECS)
def test_autoreset_leaves_the_amplitude_with_the_batch_slot(pkg, prec):
    """trajectory 1 (the second half of pair 0) patched past max_value: the step raises its flag, pdec_env_autoreset restarts it
    from y0 in that step, and the NEXT step integrates it at mu[1] as before"""
    from oracle import ks
    case, dt = "perm_oddA_256", _dt(prec)
    setup, cfgs, mu, g = _row(pkg, case, prec)
    B = dc.batch(case)
    y0, act, prev = kc.inputs(case, B, steps=2, seed=7)
    y0, act, prev = _cast(y0, prec), _cast(act, prec), _cast(prev, prec)
    env = pkg.PDEenv(setup, B=B, dtype=dt, y0=y0, autoreset=True)
    env.set_disturbance(mu)
    env.action.copy_(_act(env, prev, dt))
    env.y[1, -3:] = kc.BLOWUP_PATCH
    env(_act(env, act[0], dt))
    torch.cuda.synchronize()
    assert env.done.tolist() == [False, True, False, False, False]
    assert _same(env.y[1], env.y0[1]) and not _same(env.y[0], env.y0[0])       # restarted in that step
    y_in = env.y.clone()
    env(_act(env, act[1], dt))
    torch.cuda.synchronize()
    assert env.done.tolist() == [False] * B
    worst, ok = {}, True
    for b in range(B):
        y_ref = kc.oracle_step(ks, cfgs[b], case, _np(y_in[b]), _np(env.p[b]))
        ok &= _err(worst, "y_restarted" if b == 1 else "y", _np(env.y[b]), y_ref, kc.tol_y(prec, case, y_ref))
    print(f"[ks-disturbance autoreset {prec}] (worst, bound):", worst)
    assert ok, worst
    env.close()


# ------------------------------------------------------------------ d. rollouts
def _ks_roll_setup(pkg, prec, B, seed=3):
    setup, cfgs, mu, g = _row(pkg, ROLL_CASE, prec)
    ns, A = setup.state_shape
    y0 = _cast(kc.inputs(ROLL_CASE, B, seed=seed)[0], prec)
    dims, P = _actor_params(ns, kc.roll_h(ROLL_CASE), 11)
    return setup, y0, dims, P, A


@pytest.mark.parametrize("prec", PRECS)
def test_persistent_rollout_equals_the_step_loop_with_amplitudes_set(pkg, monkeypatch, prec):
    """ks_rollout_kernel (solo form) against the enqueued step loop of the same Philox stream, both environments holding the
    amplitude array: 6 steps, learning, noise 0.3; the bounds of test_rollout_equals_step_by_step_loop"""
    dt, T, B = _dt(prec), 6, 5
    setup, y0, dims, P, A = _ks_roll_setup(pkg, prec, B)
    mu = dc.amplitudes(ROLL_CASE)
    actor = pkg.HipMLP(dims, ["relu", "tanh"], P, dtype=dt, max_cols=B * A)
    outs, envs = [], []
    for persistent in ("1", "0"):
        monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", persistent)
        env = pkg.PDEenv(setup, B=B, dtype=dt, y0=y0, autoreset=False)
        env.set_disturbance(mu)
        L = pkg._lib
        L.check(env.lib.pdec_prof_reset(env.handle))
        L.check(env.lib.pdec_prof_enable(env.handle, 1))
        outs.append(env.rollout(actor, T, act_noise=0.3, act_limit=1.0, learning=True, seed=99, offset=0, log=True))
        torch.cuda.synchronize()
        ms, n = C.c_double(), C.c_int()
        assert env.lib.pdec_prof_get(env.handle, b"ks_rollout", C.byref(ms), C.byref(n)) == 0
        assert n.value == (1 if persistent == "1" else 0)
        L.check(env.lib.pdec_prof_enable(env.handle, 0))
        envs.append(env)
    sc = 1e-6 if prec == "f64" else 1.0
    worst, ok = {}, True
    d = lambda x, y: _np(x) - _np(y)
    for k, tol in (("y", 2e-5), ("p", 2e-4), ("action", 2e-5), ("reward", 2e-5), ("reward_sum", 2e-5)):
        ok &= _err(worst, k, d(outs[0][k], outs[1][k]), 0, tol * sc)
    ok &= _err(worst, "y_end", d(envs[0].y, envs[1].y), 0, 2e-5 * sc)
    print(f"[ks-disturbance rollout {prec}] (worst, bound):", worst)
    assert ok, worst
    # the amplitudes act: the same launch without them is elsewhere by the last step
    monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", "1")
    plain = pkg.PDEenv(setup, B=B, dtype=dt, y0=y0, autoreset=False)
    out = plain.rollout(actor, T, act_noise=0.3, act_limit=1.0, learning=True, seed=99, offset=0, log=True)
    assert float((out["y"][-1] - outs[0]["y"][-1]).abs().max()) > 1e-3
    plain.close()
    for e in envs:
        e.close()


@pytest.mark.parametrize("prec", PRECS)
def test_member_rollout_is_bit_for_bit_its_blocks_solo_rollouts(pkg, monkeypatch, prec):
    """pdec_rollout_members on M = 2 blocks of K = 3 trajectories with six different amplitudes: block m's rows are bit for bit
    pdec_rollout on a B = 3 environment that holds its three amplitudes (the lone third trajectory included)"""
    monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", "1")
    L = pkg._lib
    dt, M, K, T = _dt(prec), 2, 3, 6
    setup, y0, dims, P, A = _ks_roll_setup(pkg, prec, K, seed=5)
    mu = np.array([0.05, -0.05, 0.15, 0.0, 0.1, -0.1])
    actors = [pkg.HipMLP(dims, ["relu", "tanh"], _actor_params(dims[0], dims[1], 100 + m)[1], dtype=dt, max_cols=M * K * A) for m in range(M)]
    env = pkg.PDEenv(setup, B=M * K, dtype=dt, y0=np.concatenate([y0] * M), autoreset=False)
    env.set_disturbance(mu)
    kw = dict(dtype=dt, device="cuda:0")
    rsum, dstep = torch.zeros((M * K, A), **kw), torch.zeros(M * K, dtype=torch.int32, device="cuda:0")
    ly, lr = torch.empty((T, M * K, setup.nx), **kw), torch.empty((T, M * K, A), **kw)
    handles, got = (L.Handle * M)(*[int(getattr(a.handle, "value", a.handle)) for a in actors]), C.c_int(-1)
    L.check(env.lib.pdec_rollout_members(env.handle, handles, M, K, T, L.ptr(env.y), L.ptr(env.state), L.ptr(env.action), 1.0, 0, L.ptr(rsum),
                                         L.ptr(ly), None, None, L.ptr(lr), None, L.ptr(dstep), C.byref(got)))
    torch.cuda.synchronize()
    assert got.value == 1
    for m in range(M):
        solo_env = pkg.PDEenv(setup, B=K, dtype=dt, y0=y0, autoreset=False)
        solo_env.set_disturbance(mu[m * K:(m + 1) * K])
        solo = solo_env.rollout(actors[m], T, learning=False, log=True)
        torch.cuda.synchronize()
        sl = slice(m * K, (m + 1) * K)
        assert _same(ly[:, sl], solo["y"]) and _same(lr[:, sl], solo["reward"]) and _same(rsum[sl], solo["reward_sum"]), m
        assert _same(env.y[sl], solo_env.y) and dstep[sl].tolist() == [-1] * K
        solo_env.close()
    assert not _same(ly[:, 0], ly[:, K])
    env.close()


def _control_from_body(pkg, setup, dt, B, y0, actor, persistent, tol, mu=None, zero_actor=None):
    """rollout(control_from = ROLL_FROM) of ROLL_T steps, learning with noise, against (a) the step loop that is GIVEN zero actions
    for the first steps and acts from the same Philox offsets afterwards and (b), on the persistent route, the same launch with
    an actor that returns exactly zero.  tol = None: bit for bit (the rollout IS that step loop)."""
    L = pkg._lib
    T, n0, noise, seed = dc.ROLL_T, dc.ROLL_FROM, 0.3, 99
    ns, A = setup.state_shape
    cols = B * A
    mk = lambda: pkg.PDEenv(setup, B=B, dtype=dt, y0=y0, autoreset=False)
    env, ref = mk(), mk()
    for e in (env, ref):
        if mu is not None:
            e.set_disturbance(mu)
    out = env.rollout(actor, T, act_noise=noise, act_limit=1.0, learning=True, seed=seed, offset=0, log=True, control_from=n0)
    rows = []
    for t in range(T):
        a = torch.zeros(ref._ashape, dtype=dt, device="cuda:0")
        if t >= n0:
            L.check(ref.lib.pdec_policy_act_rng(actor.handle, L.ptr(ref.state), cols, noise, 1.0, 1, seed, t * ((cols + 3) // 4), L.ptr(a)))
        ref(a)
        rows.append((ref.y.clone(), ref.p.clone(), ref.action.clone(), ref.reward.clone()))
    torch.cuda.synchronize()
    assert out["done_step"].tolist() == [-1] * B and env.steps == T
    # the uncontrolled prefix: exactly the zero action, and no forcing
    assert float(out["action"][:n0].abs().max()) == 0.0 and float(out["p"][:n0].abs().max()) == 0.0
    assert float(out["action"][n0:].abs().max()) > 1e-3
    worst, ok = {}, True
    for t in range(T):
        for k, name in enumerate(("y", "p", "action", "reward")):
            if tol is None:
                assert _same(out[name][t], rows[t][k]), (t, name)
            else:
                ok &= _err(worst, name + ("_prefix" if t < n0 else ""), _np(out[name][t]) - _np(rows[t][k]), 0, tol * (10 if name == "p" else 1))
    assert ok, worst
    # reward_sum: the rows n0 .. T - 1 in step order, nothing of the prefix
    rs = torch.zeros_like(out["reward_sum"])
    for t in range(n0, T):
        rs += out["reward"][t]
    assert _same(out["reward_sum"], rs) and float(out["reward"][:n0].abs().max()) > 0.0
    if zero_actor is not None:      # the same kernel driven by an actor that returns 0: the prefix bit for bit
        z = mk()
        if mu is not None:
            z.set_disturbance(mu)
        zo = z.rollout(zero_actor, n0, learning=False, log=True)
        torch.cuda.synchronize()
        for name in ("y", "p", "action", "reward"):
            assert _same(out[name][:n0], zo[name]), name
        z.close()
    # flags cover the prefix as well: a trajectory that starts past max_value is reported at step 0
    if not env.is_fluid:
        env.reset()
        env.y[B - 1].fill_(1e3)
        out2 = env.rollout(actor, n0 + 1, learning=False, control_from=n0)
        torch.cuda.synchronize()
        assert out2["done_step"].tolist()[B - 1] == 0
    # and control_from = 0 afterwards is the plain rollout again (the Python layer sets it on every call)
    env.reset(), ref.reset()
    o1, o2 = env.rollout(actor, 2, learning=False, log=True), ref.rollout(actor, 2, learning=False, log=True, control_from=0)
    torch.cuda.synchronize()
    assert _same(o1["y"], o2["y"]) and float(o1["action"][0].abs().max()) > 0.0
    env.close(), ref.close()
    return worst


@pytest.mark.parametrize("prec,persistent", [("f64", "1"), ("f32", "1"), ("f32", "0")])
def test_control_from_on_ks(pkg, monkeypatch, prec, persistent):
    monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", persistent)
    dt, B = _dt(prec), 5
    setup, y0, dims, P, A = _ks_roll_setup(pkg, prec, B)
    actor = pkg.HipMLP(dims, ["relu", "tanh"], P, dtype=dt, max_cols=B * A)
    zero = pkg.HipMLP(dims, ["relu", "tanh"], [np.zeros_like(p) for p in P], dtype=dt, max_cols=B * A)
    tol = None if persistent == "0" else (2e-11 if prec == "f64" else 2e-5)
    worst = _control_from_body(pkg, setup, dt, B, y0, actor, persistent, tol, mu=dc.amplitudes(ROLL_CASE),
                               zero_actor=zero if persistent == "1" else None)
    print(f"[ks-disturbance control_from ks {prec} persistent={persistent}] (worst, bound):", worst)


def test_control_from_on_keller_segel(pkg, monkeypatch):
    """kseg_rollout_kernel, fp64: the bounds of test_rollout_equals_step_by_step_loop (2e-11)"""
    monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", "1")
    setup, dt, B = pkg.KellerSegelSetup(), torch.float64, 3
    y0 = np.ascontiguousarray(np.swapaxes(setup.generate_random_init(np.random.default_rng(0), B), 1, 2))
    agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(1), dtype=dt, start_steps=-1)
    worst = _control_from_body(pkg, setup, dt, B, y0, agent.policy.behavior_actor.model, "1", 2e-11)
    print("[ks-disturbance control_from keller_segel f64] (worst, bound):", worst)


def test_control_from_on_the_fluid_step_loop(pkg):
    """the enqueued step loop (csrc/rollout.hip) on a 32 x 32 fluid: bit for bit the loop given zero actions first"""
    setup, dt, B = pkg.FluidSetup(nx=32, sensors_per_axis=4, oversampling=2), torch.float64, 2
    agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(1), dtype=dt, start_steps=-1)
    probe = pkg.PDEenv(setup, B=B, dtype=dt, autoreset=False)
    y0 = setup.random_init_device(probe, np.random.default_rng(3)).clone()
    probe.close()
    _control_from_body(pkg, setup, dt, B, y0, agent.policy.behavior_actor.model, "0", None)


# ------------------------------------------------------------------ e. evaluate_actors
@pytest.mark.parametrize("persistent", ["1", "0"])
def test_evaluate_actors_over_amplitudes(pkg, monkeypatch, persistent):
    """mu = [0.0, 0.05], M = 2, K = 3: the shapes, every (member, amplitude) block bit for bit the call with that single
    amplitude, the order by the mean over the amplitudes; mu = None keeps its shapes and is the members' solo rollouts.  One
    launch where ks_rollout_kernel serves (persistent = 1), M n_mu solo rollouts otherwise."""
    monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", persistent)
    prec, dt, M, K, T, n0 = "f64", torch.float64, 2, 3, 6, 2
    setup, y0, dims, P, A = _ks_roll_setup(pkg, prec, K, seed=5)
    y0 = to_dev(y0, dt)
    actors = [pkg.HipMLP(dims, ["relu", "tanh"], _actor_params(dims[0], dims[1], 100 + m)[1], dtype=torch.float32, max_cols=K * A)
              for m in range(M)]
    mus = [0.0, 0.05]
    res = pkg.evaluate_actors(setup, actors, y0=y0, dtype=dt, steps=T, log=True, mu=mus, control_from=n0)
    assert res["one_launch"] is (persistent == "1")
    assert res["episode_reward"].shape == (M, 2, K) and res["reward_sum"].shape == (M, 2, K, A) and res["done_step"].shape == (M, 2, K)
    assert res["score"].shape == (M, 2) and np.array_equal(res["mu"], np.array(mus)) and res["y"].shape[:4] == (T, M, 2, K)
    assert np.isfinite(res["score"]).all() and float(res["action"][:n0].abs().max()) == 0.0
    mean = res["score"].mean(axis=1)
    assert res["order"] == sorted(range(M), key=lambda m: (-mean[m], m))
    for i, m_ in enumerate(mus):
        one = pkg.evaluate_actors(setup, actors, y0=y0, dtype=dt, steps=T, log=True, mu=[m_], control_from=n0)
        assert one["episode_reward"].shape == (M, 1, K)
        for k in ("episode_reward", "reward_sum", "done_step"):
            assert _same(res[k][:, i], one[k][:, 0]), (i, k)
        for k in ("y", "p", "action", "reward"):
            assert _same(res[k][:, :, i], one[k][:, :, 0]), (i, k)
        assert np.array_equal(res["score"][:, i], one["score"][:, 0])
    assert not _same(res["y"][:, :, 0], res["y"][:, :, 1])
    # mu = None: today's shapes, and the members' solo rollouts at the setup's own mu
    plain = pkg.evaluate_actors(setup, actors, y0=y0, dtype=dt, steps=T, log=True)
    assert "mu" not in plain and plain["episode_reward"].shape == (M, K) and plain["score"].shape == (M,) and plain["y"].shape[:3] == (T, M, K)
    for m, actor in enumerate(actors):
        env = pkg.PDEenv(setup, B=K, dtype=dt, y0=y0, autoreset=False)
        solo = env.rollout(actor.clone(dtype=dt, max_cols=K * A), T, learning=False, log=True)
        torch.cuda.synchronize()
        for k in ("y", "p", "action", "reward"):
            assert _same(plain[k][:, m], solo[k]), (m, k)
        assert _same(plain["reward_sum"][m], solo["reward_sum"])
        env.close()
    # a NaN at one amplitude is a NaN of the member's mean: last in the order
    bad = y0.clone()
    res2 = pkg.evaluate_actors(setup, [actors[0]], y0=bad, dtype=dt, steps=2, mu=[0.0, np.nan])
    assert np.isnan(res2["score"][0, 1]) and np.isfinite(res2["score"][0, 0]) and res2["order"] == [0]


# ------------------------------------------------------------------ f. the training pipeline
def _pipeline(pkg, use_graphs, mu, E):
    B = 4
    setup = pkg.KSSetup.bench_C2(256)
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    y0 = setup.generate_random_init(np.random.default_rng(0), B) * 0.15
    env = pkg.PDEenv(setup, B=B, dtype=torch.float32, y0=y0, stream=s_env, autoreset=False)
    if mu is not None:
        env.set_disturbance(mu)
    agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                             noise_seed=7, trajectory_length=1)
    agent.policy.act_noise = 0.3
    torch.cuda.synchronize()
    return pkg.TrainPipeline(env, agent, lag=2, episode_steps=E, stream_env=s_env, stream_upd=s_upd, use_graphs=use_graphs,
                             chunks=(6, 1), noise_seed=99)


@pytest.mark.parametrize("E", [6, 13])
def test_train_pipeline_steps_what_the_environment_holds(pkg, E):
    """KS, B = 4, two episodes on an environment with amplitudes set: use_graphs=True bit for bit use_graphs=False, and not the
    run without amplitudes.  E = 6: episodes too short for a graph period, so both pipelines replay their recorded library calls.
    E = 13: the interior steps come from captured graphs of six steps, which keep reading the array the environment holds."""
    mu = np.array([0.05, -0.05, 0.15, 0.1])
    pe, pg, p0 = _pipeline(pkg, False, mu, E), _pipeline(pkg, True, mu, E), _pipeline(pkg, False, None, E)
    if E > 12:
        pg.run(5)
        pg.capture()
        pe.run(pg.tick), p0.run(pg.tick)
    n = 2 * E
    for p in (pe, pg, p0):
        p.run(n)
        p.sync()
    assert pe.tick == pg.tick == p0.tick and (pg.n_graph_launches > 0) == (E > 12)
    assert _same(pe.y, pg.y) and _same(pe.state, pg.state) and bool(torch.isfinite(pg.y).all())
    for nm in ("behavior_actor", "behavior_critic", "target_actor", "target_critic"):
        for x, y in zip(getattr(pe.policy, nm).model.params(), getattr(pg.policy, nm).model.params()):
            assert np.array_equal(x, y), nm
    assert float((pe.y - p0.y).abs().max()) > 1e-3
    for p in (pe, pg, p0):
        p.close()


# ------------------------------------------------------------------ g. refusals, by name
def test_refusals(pkg):
    from oracle import ks
    L = pkg._lib
    mono, _ = kc.build(pkg, ks, "mono_256")
    for setup, B, word in ((mono, 5, "mono"), (pkg.KellerSegelSetup(), 3, "Keller-Segel"),
                           (pkg.FluidSetup(nx=32, sensors_per_axis=4, oversampling=2), 2, "fluid")):
        env = pkg.PDEenv(setup, B=B, dtype=torch.float64, autoreset=False)
        with pytest.raises(pkg.PdecError, match=word):
            env.set_disturbance(np.zeros(B))
        assert env.mu is None
        env.set_disturbance(None)              # nothing to return from: accepted
        env.close()
    setup, cfgs, mu, g = _row(pkg, "perm_oddA_256", "f64")
    env = pkg.PDEenv(setup, B=5, dtype=torch.float64, autoreset=False)
    for wrong in (np.zeros(4), np.zeros((5, 1)), np.zeros(6)):
        with pytest.raises(pkg.PdecError, match="expected 5 amplitudes"):
            env.set_disturbance(wrong)
    assert env.mu is None
    with pytest.raises(pkg.PdecError, match="negative"):
        L.check(env.lib.pdec_env_set_control_from(env.handle, -1))
    env.close()
