"""The Kuramoto-Sivashinsky kernels (csrc/ks_step.hip: ks_env_step_kernel with every FFT engine, its SIMD-sharing form; ks_rollout.hip:
ks_rollout_kernel in its solo and member forms; ksfd.hip: ksfd_env_step_kernel, ksfd_wave_step_kernel; env.hip: sense_kernel, and the band tables pdec_env_create builds)
against oracle/ks.py over the geometries of ks_geometry_cases.py: both actuation branches of every engine, A != S, odd A,
permuted and repeated actuators_to_sensors, bands narrower than sense_dots' unrolled body, cells no actuator reaches, every
grouping of sense_dots, the global agent with A != S, the temporal stack, all three blow-up tests, punishments and the disturbance
in the packed pair.  test_ks_geometry_table.py proves without a GPU that each row reaches what it is there for and that plausible
mistakes move the oracle by at least 100 bounds.  B = 5 throughout: two full pairs and a lone last trajectory; every trajectory is
compared.  fp32 inputs are rounded once and the oracle runs in fp64 FROM those values.

Tolerances (ks_geometry_cases.tol_*; none taken from the kernels under test).
  y       1e-11 / 3e-5 max(1, |ref|) after one control step from the device's own previous field
          (test_every_fft_engine_and_size_limit); finite differences 1e-11 / 2e-4 max |ref| (test_rk4_fd_variant_matches_its_oracle)
  p       1e-12 / 1e-5 max(1, |p|)
  state, reward: compared at the DEVICE's new field, so the integrator's rounding stays out of them, with bounds from the format
          (u = 2^-53 / 2^-24, |y| <= ymax of that trajectory):
          state   2 (Wd + 3) u ymax / max_value -- a dot of Wd non-negative weights that sum to 1, in any order of summation
          reward  2 [f'(ymax) (Wd + 2) u ymax + 9 u f(ymax) + ...], f(d) = (6 d)^1.3 / (3 max_value); the terms are listed at
                  ks_geometry_cases.tol_reward.  The factor 2 is the oracle's own fp64 sum in the fp64 comparison.
  rollouts  against the per-step loop of the same Philox stream: test_rollout_equals_step_by_step_loop's figures (fp32 actions
          2e-6 at the first step, everything 2e-5, p 2e-4 over 6 steps; fp64 1e-6 of that); the member form bit for bit
  reward partials  (depth) u sum |r|, derived at the assert

Worst deviation / bound over all rows on an MI355X, the row with the largest ratio (every test prints its own line):
                               fp64                               fp32
  pieces   p                   2.7e-14 / 2.7e-11 dense_192        6.5e-6 / 2.3e-4  dense_192
           y                   4.3e-15 / 1.3e-11 generic_60       2.0e-6 / 3.5e-5  generic_60
           state (reset form)  3.5e-18 / 3.5e-17 narrower_256     1.9e-9 / 1.5e-8  narrower_256
           state (prev_state)  6.9e-18 / 9.7e-17 fd_midpoint_100  4.3e-9 / 2.8e-8  subset_1024
           reward              4.2e-17 / 7.4e-16 narrow_256       2.3e-8 / 2.2e-7  narrow_256
  fused    p                   2.1e-14 / 1.9e-11 dense_192        6.5e-6 / 1.6e-4  dense_192
           y                   5.7e-15 / 1.3e-11 generic_60       2.0e-6 / 3.5e-5  generic_60
           state               6.9e-18 / 9.7e-17 fd_midpoint_100  4.0e-9 / 2.3e-8  fd_midpoint_100
           reward              8.3e-17 / 1.4e-15 narrow_256       2.8e-8 / 2.7e-7  narrow_256
           vs pieces: p 0 / 0 (bit for bit), y 2.2e-16 / 1.2e-7, state 1.4e-17 / 7.5e-9, reward 8.3e-17 / 4.5e-8
  SIMD-sharing form (fp32): y 4.8e-6 / 8e-5, p 6.5e-7 / 1e-5, reward 2.8e-7 / 1e-5; against the register form y 3.7e-7 / 2e-6,
           p 0, state 1.0e-8 / 2e-6, reward 2.4e-7 / 6e-6
  blow-up  y of the patched one's partner  1.8e-14 / 4.0e-10 sparse_240   5.5e-6 / 1.2e-3 sparse_240
           y of the patched one            3.6e-14 / 4.1e-10              3.6e-5 / 1.2e-3
           y of trajectories 2, 3          2.3e-15 / 1.0e-11              9.3e-7 / 3.0e-5
           state / reward (tame)           1.0e-17 / 1.9e-16, 8.9e-16 / 8.8e-15     3.3e-9 / 3.9e-8, 1.5e-7 / 3.5e-6
           state / reward (patched)        2.2e-16 / 1.0e-14, 1.8e-15 / 1.9e-13     1.3e-7 / 2.3e-6, 1.5e-6 / 5.9e-5
  rollout  first action        1.1e-16 / 2e-12                    6.0e-8 / 2e-6
           y, p (logged rows)  7.1e-15 / 2e-11, 7.1e-15 / 2e-10   2.4e-6 / 2e-5, 3.8e-6 / 2e-4   dense_192
           action, reward      1.1e-16, 6.7e-16 / 2e-11           6.0e-8, 4.8e-7 / 2e-5
           reward_sum          1.8e-15 / 2e-11                    9.5e-7 / 2e-5
  reward partials (fp32)       8.5e-7 / 5.2e-6 perm_oddA_256
  engine switches (PDEC_KS_LDS_FFT=1: FftR4, PDEC_KS_GENERIC_FFT=1: FftGeneric; perm_oddA_256 and subset_1024, the bounds above)
  fused    p                   1.8e-15 / 6.4e-12 perm_oddA_256 R4   6.5e-7 / 6.8e-5  perm_oddA_256 R4
           y                   2.8e-15 / 1.0e-11 perm_oddA_256 R4   1.2e-6 / 3.0e-5  perm_oddA_256 R4
           state               6.9e-18 / 1.6e-16 subset_1024 R4     4.3e-9 / 2.8e-8  subset_1024 R4
           reward              4.4e-16 / 8.2e-15 perm_oddA_256 R4   2.8e-7 / 3.4e-6  perm_oddA_256 generic
           vs pieces: p 0 / 0, y 0 / 0 (bit for bit), state 6.9e-18 / 5.6e-9, reward 2.2e-16 / 6.0e-8
  rollout  served by ks_rollout_kernel on perm_oddA_256 in fp32 only (the other six rows exceed 64 KiB of LDS with the larger
           transform buffers and run as the step loop, bit for bit): first action 3.0e-8 / 2e-6, y 6.3e-7 / 2e-5,
           p 4.8e-7 / 2e-4, action 6.0e-8, reward 2.4e-7, reward_sum 3.6e-7 / 2e-5 (R4; generic: no larger)
No quantity exceeded its bound and no kernel or table had to change."""
import ctypes as C

import numpy as np
import pytest

import ks_geometry_cases as kc
from util import to_dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

B = 5
ROWS = [(n, p) for n, c in kc.CASES.items() for p in c.precs]
IDS = [f"{n}-{p}" for n, p in ROWS]


def _dt(prec):
    return torch.float64 if prec == "f64" else torch.float32


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _jl(t):    # device [A, ns] -> Julia-shaped [ns, A] float64 host array
    return _np(t).T


def _cast(a, prec):
    """the values the device sees: fp32 inputs are rounded once, the oracle then runs in fp64 FROM those values"""
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
    """(setup, oracle config, geometry) of a row, built once per session: the Gaussian tables of the large grids take longer
    than the kernels under test"""
    from oracle import ks
    if case not in _MEMO:
        setup, cfg = kc.build(pkg, ks, case)
        _MEMO[case] = (setup, cfg, {p: kc.geometry(*setup.tables(), case, p) for p in ("f64", "f32")})
    setup, cfg, geo = _MEMO[case]
    return setup, cfg, geo[prec]


def _act(env, a, dt):
    return to_dev(a, dt).reshape(env._ashape)


def _sense_bounds(prec, case, g, y):
    ymax = float(np.abs(y).max())
    return kc.tol_state(prec, case, g, ymax), kc.tol_reward(prec, case, g, ymax)


# ------------------------------------------------------------------ a. the pieces through the C ABI
@pytest.mark.parametrize("case,prec", ROWS, ids=IDS)
def test_pieces_match_the_oracle(pkg, case, prec):
    """prepare_action, do_step, featurize (without and with prev_state) and reward_function: sense_kernel at its 128 threads and
    the unfused step, every trajectory of B = 5"""
    from oracle import ks
    dt = _dt(prec)
    setup, cfg, g = _row(pkg, case, prec)
    y0, act, prev = kc.inputs(case, B)
    y0, a0, a1 = _cast(y0, prec), _cast(prev, prec), _cast(act[0], prec)
    env = pkg.PDEenv(setup, B=B, dtype=dt, autoreset=False)
    yd, a0d, a1d = to_dev(y0, dt), _act(env, a0, dt), _act(env, a1, dt)
    p_dev = env.prepare_action(a1d)
    y1_dev, flags = env.do_step(yd, p_dev)
    st0_dev = env.featurize(yd)
    st1_dev = env.featurize(y1_dev, st0_dev)
    r_dev = env.reward_function(y1_dev, a1d, a0d)
    torch.cuda.synchronize()
    assert flags.tolist() == [0] * B
    worst, ok = {}, True
    for b in range(B):
        p_ref = ks.prepare_action(cfg, a1[b][None])
        ok &= _err(worst, "p", _np(p_dev[b]), p_ref, kc.tol_p(prec, p_ref))
        ref = kc.oracle_step(ks, cfg, case, y0[b], _np(p_dev[b]))                 # downstream: the oracle at the device's own inputs
        assert np.isfinite(ref).all()
        ok &= _err(worst, "y", _np(y1_dev[b]), ref, kc.tol_y(prec, case, ref))
        ts, _ = _sense_bounds(prec, case, g, y0[b])
        ok &= _err(worst, "state0", _jl(st0_dev[b]), ks.featurize(cfg, y0[b], None), ts)
        y1 = _np(y1_dev[b])
        ts, tr = _sense_bounds(prec, case, g, y1)
        ok &= _err(worst, "state1", _jl(st1_dev[b]), ks.featurize(cfg, y1, _jl(st0_dev[b])), ts)
        ok &= _err(worst, "reward", _np(r_dev[b]), ks.reward_function(cfg, y1, a1[b][None], (a1[b] - a0[b])[None]), tr)
    print(f"[ks-geometry pieces {case} {prec}] (worst, bound):", worst)
    assert ok, worst
    env.close()


# ------------------------------------------------------------------ b. the fused step, three control steps
def _fused_step_body(pkg, case, prec, tag=""):
    """the body of test_fused_step_matches_the_oracle_and_the_pieces (tag: what the printed line adds to the row's name)"""
    from oracle import ks
    dt = _dt(prec)
    c = kc.CASES[case]
    setup, cfg, g = _row(pkg, case, prec)
    y0, act, prev = kc.inputs(case, B)
    y0, act, prev = _cast(y0, prec), _cast(act, prec), _cast(prev, prec)
    env = pkg.PDEenv(setup, B=B, dtype=dt, y0=y0, autoreset=False)
    pieces = pkg.PDEenv(setup, B=B, dtype=dt, autoreset=False)
    term = torch.full((B, setup.reward_len), 7.0, dtype=dt, device="cuda:0")
    env.set_terminal_out(term)
    env.action.copy_(_act(env, prev, dt))
    worst, ok = {}, True
    for b in range(B):
        ok &= _err(worst, "state_reset", _jl(env.state[b]), ks.featurize(cfg, y0[b], None), _sense_bounds(prec, case, g, y0[b])[0])
    a_prev = prev
    for t in range(act.shape[0]):
        y_in, st_in = env.y.clone(), env.state.clone()
        a_dev, ap_dev = _act(env, act[t], dt), _act(env, a_prev, dt)
        env(a_dev)
        torch.cuda.synchronize()
        assert env.done.tolist() == [False] * B and float(term.abs().max()) == 0.0        # tame rows (test_ks_geometry_table.py)
        p_pc = pieces.prepare_action(a_dev)
        y_pc, _ = pieces.do_step(y_in, p_pc)
        st_pc = pieces.featurize(env.y, st_in)                    # sensing pieces at the fused step's own new field
        r_pc = pieces.reward_function(env.y, a_dev, ap_dev)
        torch.cuda.synchronize()
        for b in range(B):
            yb, sb = _np(y_in[b]), _jl(st_in[b])
            p_ref = ks.prepare_action(cfg, act[t][b][None])
            tp = kc.tol_p(prec, p_ref)
            ok &= _err(worst, "p", _np(env.p[b]), p_ref, tp)
            y_ref = kc.oracle_step(ks, cfg, case, yb, _np(env.p[b]))
            assert np.isfinite(y_ref).all() and np.abs(y_ref).max() < 6.0
            ty = kc.tol_y(prec, case, y_ref)
            ok &= _err(worst, "y", _np(env.y[b]), y_ref, ty)
            y_new = _np(env.y[b])
            ts, tr = _sense_bounds(prec, case, g, y_new)
            ok &= _err(worst, "state", _jl(env.state[b]), ks.featurize(cfg, y_new, sb), ts)
            r_ref = ks.reward_function(cfg, y_new, act[t][b][None], (act[t][b] - a_prev[b])[None])
            ok &= _err(worst, "reward", _np(env.reward[b]), r_ref, tr)
            assert kc.want_done(case, y_new, r_ref) is False
            ok &= _err(worst, "p_vs_pieces", _np(env.p[b]), _np(p_pc[b]), tp)
            ok &= _err(worst, "y_vs_pieces", _np(env.y[b]), _np(y_pc[b]), ty)
            ok &= _err(worst, "state_vs_pieces", _jl(env.state[b]), _jl(st_pc[b]), ts)
            ok &= _err(worst, "reward_vs_pieces", _np(env.reward[b]), _np(r_pc[b]), tr)
        a_prev = act[t]
    print(f"[ks-geometry fused {case} {prec}{tag}] (worst, bound):", worst)
    assert ok, worst
    if c.temporal_steps > 1:       # the stack really shifted: the older block is the fresh block of the step before
        assert _same(env.state[:, :, c.window_size:], st_in[:, :, :c.window_size]) and not _same(env.state[:, :, :c.window_size], st_in[:, :, :c.window_size])
    env.close(), pieces.close()


@pytest.mark.parametrize("case,prec", ROWS, ids=IDS)
def test_fused_step_matches_the_oracle_and_the_pieces(pkg, case, prec):
    """three control steps, each teacher-forced: the oracle starts every step from the device's own previous field, so chaos
    does not accumulate.  p, y, reward, state, done and the terminal columns; state and reward at the device's new field; and the
    fused step against the stand-alone pieces at the same inputs"""
    _fused_step_body(pkg, case, prec)


# the two engines that only a switch reaches (README, the table of switches): radix-4 through LDS at 256 / 1024 cells, and the
# generic engine on a grid that has a compile-time one.  These two rows are the only grids on which the switches select anything.
SWITCHES = {"PDEC_KS_LDS_FFT": "FftR4", "PDEC_KS_GENERIC_FFT": "FftGeneric"}
SWITCH_ROWS = [(sw, n, p) for sw in SWITCHES for n in ("perm_oddA_256", "subset_1024") for p in ("f64", "f32")]
SWITCH_IDS = [f"{sw}-{n}-{p}" for sw, n, p in SWITCH_ROWS]


@pytest.mark.parametrize("switch,case,prec", SWITCH_ROWS, ids=SWITCH_IDS)
def test_fused_step_under_the_engine_switches(pkg, monkeypatch, switch, case, prec):
    """test_fused_step_matches_the_oracle_and_the_pieces with the engine of the switch (read when the environments are created),
    held to the same bounds as the default engines"""
    monkeypatch.setenv(switch, "1")
    _fused_step_body(pkg, case, prec, tag=f" {switch}=1")


def test_simd_sharing_form_with_odd_a(pkg):
    """the 64-VGPR form of the fused step (its lane-private constant slots lie behind act | actp | dots | part | red, which A = 23
    moves off the shipped offsets) on perm_oddA_256 in fp32: against the oracle and against the register form, free-running over
    four control steps, with the bounds of test_simd_sharing_form_of_the_fused_step"""
    from oracle import ks
    case, dt, T = "perm_oddA_256", torch.float32, 4
    setup, cfg, g = _row(pkg, case, "f32")
    y0, act, prev = kc.inputs(case, B, steps=T)
    y0, act, prev = _cast(y0, "f32"), _cast(act, "f32"), _cast(prev, "f32")
    envs = [pkg.PDEenv(setup, B=B, dtype=dt, y0=y0, autoreset=False) for _ in range(2)]
    assert envs[1].set_simd_sharing(True)
    for e in envs:
        e.action.copy_(_act(e, prev, dt))
    yo, a_prev, worst, ok = [y0[b].copy() for b in range(B)], prev, {}, True
    for t in range(T):
        for e in envs:
            e(_act(e, act[t], dt))
        torch.cuda.synchronize()
        for b in range(B):
            o = ks.env_step(cfg, yo[b], a_prev[b][None], act[t][b][None], 0.0)
            yo[b] = o["y"]
            ok &= _err(worst, "y", _np(envs[1].y[b]), o["y"], 2e-5 * (t + 1))
            ok &= _err(worst, "p", _np(envs[1].p[b]), o["p"], 1e-5)
            ok &= _err(worst, "reward", _np(envs[1].reward[b]), o["reward"], 1e-5 * (t + 1))
        for name in ("y", "p", "state", "reward"):
            ok &= _err(worst, name + "_vs_register_form", _np(getattr(envs[1], name)), _np(getattr(envs[0], name)), 2e-6 * (t + 1))
        a_prev = act[t]
    print("[ks-geometry simd-sharing perm_oddA_256 f32] (worst, bound):", worst)
    assert ok, worst
    assert not bool(envs[1].done.any())
    for e in envs:
        e.close()


# ------------------------------------------------------------------ c. blow-up handling
@pytest.mark.parametrize("case,prec", [(n, p) for n in kc.BLOWUP for p in ("f64", "f32")])
def test_blowup_flag_per_half_of_a_pair(pkg, case, prec):
    """B = 5 with trajectory 1 -- the second half of pair 0 -- set to +40 on its last three cells and one NaN cell in trajectory 4,
    the lone last one (ordinary data: the fields are plain numbers to every kernel).  done and the terminal columns follow
    ks_geometry_cases.blown on the oracle's field / reward: a NaN raises the flag, "off" never does.  Trajectory 0 shares the
    packed transform with the patched one, so the rounding of ITS field scales with the partner's magnitude: it is held to the
    oracle at u x 40 (the tolerance on y times 40) instead of u x max |y_0|; trajectories 2 and 3 stay at the tame bound.  The
    finite-difference rows integrate one trajectory per work-group: the tame bound for trajectory 0 as well."""
    from oracle import ks
    dt = _dt(prec)
    c = kc.CASES[case]
    setup, cfg, g = _row(pkg, case, prec)
    y0, bad, act, prev = kc.blowup_inputs(case, B)
    bad, act, prev = _cast(bad, prec), _cast(act, prec), _cast(prev, prec)
    env = pkg.PDEenv(setup, B=B, dtype=dt, y0=bad, autoreset=False)
    term = torch.full((B, setup.reward_len), 7.0, dtype=dt, device="cuda:0")
    env.set_terminal_out(term)
    env.action.copy_(_act(env, prev, dt))
    env(_act(env, act, dt))
    torch.cuda.synchronize()
    want, worst, ok = [], {}, True
    for b in range(B):
        with np.errstate(all="ignore"):
            p_ref = ks.prepare_action(cfg, act[b][None])
            y_ref = kc.oracle_step(ks, cfg, case, bad[b], _np(env.p[b]))
            y_new = _np(env.y[b])
            r_ref = ks.reward_function(cfg, y_new, act[b][None], (act[b] - prev[b])[None])
        want.append(kc.want_done(case, y_ref, r_ref))
        ok &= _err(worst, "p", _np(env.p[b]), p_ref, kc.tol_p(prec, p_ref))
        if b == 4:
            assert np.isnan(y_ref).any() and np.isnan(y_new).any()
            continue
        assert np.isfinite(y_ref).all() and np.isfinite(y_new).all()
        ty = kc.tol_y(prec, case, y_ref)
        if b == 0 and c.integrator == "cnab2":
            ty = kc.tol_y(prec, case, np.array([kc.BLOWUP_PATCH]))
        ok &= _err(worst, {0: "y_partner_of_patched", 1: "y_patched"}.get(b, "y_tame"), y_new, y_ref, ty)
        ts, tr = _sense_bounds(prec, case, g, y_new)
        ok &= _err(worst, "state_patched" if b == 1 else "state", _jl(env.state[b]), ks.featurize(cfg, y_new, None), ts)
        ok &= _err(worst, "reward_patched" if b == 1 else "reward", _np(env.reward[b]), r_ref, tr)
        if b == 1:
            assert np.abs(y_ref).max() > 1.2 * 30 and np.abs(y_new).max() > 1.2 * 30
    print(f"[ks-geometry blow-up {case} {prec}] (worst, bound):", worst)
    assert want == ([False] * B if c.check_max_value == "off" else [False, True, False, False, True])     # the oracle's verdict
    assert env.done.tolist() == want
    exp_term = torch.tensor(want, dtype=dt, device="cuda:0")[:, None].expand(B, setup.reward_len)
    assert torch.equal(term, exp_term), term
    assert ok, worst
    env.close()


# ------------------------------------------------------------------ d. rollouts
def _actor_params(ns, H, seed):
    rng = np.random.default_rng(seed)
    dims = [ns, H, 1]
    P = []
    for i in range(2):
        lim = np.sqrt(6.0 / (dims[i] + dims[i + 1]))
        P += [rng.uniform(-lim, lim, (dims[i + 1], dims[i])).astype(np.float32), rng.uniform(-0.1, 0.1, dims[i + 1]).astype(np.float32)]
    return dims, P


def _launches(env, label):
    ms, n = C.c_double(), C.c_int()
    env.lib.pdec_sync(env.handle)
    assert env.lib.pdec_prof_get(env.handle, label.encode(), C.byref(ms), C.byref(n)) == 0
    return n.value


def _rollout_body(pkg, monkeypatch, case, prec, engine=None):
    """the body of test_rollout_equals_the_step_loop_or_is_not_served (engine: the one a switch selects instead of the grid's own;
    its transform buffers enter the restated shape rule)"""
    monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", "1")
    L = pkg._lib
    dt, T, noise, seed = _dt(prec), 6, 0.3, 99
    c = kc.CASES[case]
    setup, cfg, g = _row(pkg, case, prec)
    if engine:
        g = kc.with_engine(g, case, prec, engine)
    served = kc.rollout_served(g, case, prec)
    ns, A = setup.state_shape
    y0 = _cast(kc.inputs(case, B, seed=3)[0], prec)
    env = pkg.PDEenv(setup, B=B, dtype=dt, y0=y0, autoreset=False)
    # the library's own verdict on the shape (all but the parameters' dtype): one member of B trajectories
    dims, P = _actor_params(g["S"] if c.mono else ns, kc.roll_h(case), 11)
    probe = pkg.HipMLP(dims, ["relu", "tanh"], P, dtype=torch.float32, max_cols=B * A)
    q = pkg.PDEenv(setup, B=B, dtype=dt, y0=y0, autoreset=False)
    L.check(q.lib.pdec_prof_reset(q.handle))
    L.check(q.lib.pdec_prof_enable(q.handle, 1))
    handles, got = (L.Handle * 1)(int(getattr(probe.handle, "value", probe.handle))), C.c_int(-1)
    rsum = torch.zeros((B, setup.reward_len), dtype=dt, device="cuda:0")
    L.check(q.lib.pdec_rollout_members(q.handle, handles, 1, B, 1, L.ptr(q.y), L.ptr(q.state), L.ptr(q.action), 1.0, 0, L.ptr(rsum),
                                       None, None, None, None, None, None, C.byref(got)))
    torch.cuda.synchronize()
    assert bool(got.value) is served, (case, prec, got.value)
    assert _launches(q, "ks_rollout_members") == (1 if served else 0)
    L.check(q.lib.pdec_prof_enable(q.handle, 0))
    if not served:
        assert _same(q.y, env.y) and float(rsum.abs().max()) == 0.0               # nothing was enqueued
    q.close()
    if c.mono:
        assert not served
        env.close()
        return
    actor = pkg.HipMLP(dims, ["relu", "tanh"], P, dtype=dt, max_cols=B * A)
    ref_env = pkg.PDEenv(setup, B=B, dtype=dt, y0=y0, autoreset=False)
    cols, rows, rsum, off = B * A, [], torch.zeros_like(ref_env.reward), 0
    for t in range(T):
        a = torch.empty(ref_env._ashape, dtype=dt, device="cuda:0")
        L.check(ref_env.lib.pdec_policy_act_rng(actor.handle, L.ptr(ref_env.state), cols, noise, 1.0, 1, seed, off, L.ptr(a)))
        off += (cols + 3) // 4
        ref_env(a)
        rsum += ref_env.reward
        rows.append((ref_env.y.clone(), ref_env.p.clone(), ref_env.action.clone(), ref_env.reward.clone()))
    L.check(env.lib.pdec_prof_reset(env.handle))
    L.check(env.lib.pdec_prof_enable(env.handle, 1))
    out = env.rollout(actor, T, act_noise=noise, act_limit=1.0, learning=True, seed=seed, offset=0, log=True)
    torch.cuda.synchronize()
    fused = "ks_env_step" if c.integrator == "cnab2" else "ksfd_env_step"
    one, steps = _launches(env, "ks_rollout"), _launches(env, fused)
    L.check(env.lib.pdec_prof_enable(env.handle, 0))
    assert (one, steps) == ((1, 0) if served else (0, T)), (one, steps, served)
    assert out["done_step"].tolist() == [-1] * B and int(out["done_any"].sum()) == 0 and env.steps == T
    assert bool(torch.isfinite(out["y"]).all()) and float(out["action"].abs().max()) <= 1.0
    assert not _same(out["action"][0], out["action"][1])
    if served:
        sc = 1e-6 if prec == "f64" else 1.0          # fp64: 2e-12 / 2e-11
        worst, ok = {}, True
        d = lambda x, y: _np(x) - _np(y)
        ok &= _err(worst, "action0", d(out["action"][0], rows[0][2]), 0, 2e-6 * sc)       # same state, same noise element for element
        for k, x, y in (("y_end", env.y, ref_env.y), ("state_end", env.state, ref_env.state), ("action_end", env.action, ref_env.action),
                        ("reward_sum", out["reward_sum"], rsum)):
            ok &= _err(worst, k, d(x, y), 0, 2e-5 * sc)
        for t in range(T):
            ok &= _err(worst, "y", d(out["y"][t], rows[t][0]), 0, 2e-5 * sc)
            ok &= _err(worst, "p", d(out["p"][t], rows[t][1]), 0, 2e-4 * sc)
            ok &= _err(worst, "action", d(out["action"][t], rows[t][2]), 0, 2e-5 * sc)
            ok &= _err(worst, "reward", d(out["reward"][t], rows[t][3]), 0, 2e-5 * sc)
        print(f"[ks-geometry rollout {case} {prec}{' ' + engine if engine else ''}] H = {kc.roll_h(case)} (worst, bound):", worst)
        assert ok, worst
    else:
        assert _same(env.y, ref_env.y) and _same(env.state, ref_env.state) and _same(env.action, ref_env.action)
        assert _same(out["reward_sum"], rsum)
        for t in range(T):
            for k, name in enumerate(("y", "p", "action", "reward")):
                assert _same(out[name][t], rows[t][k]), (t, name)
    env.close(), ref_env.close()


@pytest.mark.parametrize("case,prec", ROWS, ids=IDS)
def test_rollout_equals_the_step_loop_or_is_not_served(pkg, monkeypatch, case, prec):
    """ks_rollout_kernel on every row the restated ks_rollout_shape_ok serves: 6 steps with learning = True, noise 0.3, against the
    per-step loop pdec_policy_act_rng -> (env)(action) of the same Philox stream -- logged rows, reward_sum and done_step, with
    test_rollout_equals_step_by_step_loop's bounds.  With odd A one column pair of the policy loop straddles the two packed
    trajectories and its noise element shares a Box-Muller pair across them.  A row that is not served (temporal stack, "reward"
    check, mono, finite differences, more than 64 KiB) must be refused by the library as well: pdec_rollout_members reports
    served = 0 and enqueues nothing, and the per-actuator rows then run as the enqueued step loop, bit for bit."""
    _rollout_body(pkg, monkeypatch, case, prec)


@pytest.mark.parametrize("switch,case,prec", SWITCH_ROWS, ids=SWITCH_IDS)
def test_rollout_under_the_engine_switches(pkg, monkeypatch, switch, case, prec):
    """test_rollout_equals_the_step_loop_or_is_not_served with the engine of the switch: ks_rollout_kernel<T, FftR4 | FftGeneric>
    where the larger transform buffers leave the launch under 64 KiB (perm_oddA_256 in fp32), the step loop on that engine
    elsewhere -- and the library's verdict must be the restated one either way"""
    monkeypatch.setenv(switch, "1")
    _rollout_body(pkg, monkeypatch, case, prec, engine=SWITCHES[switch])


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_member_rollout_with_odd_a_equals_the_solo_rollouts(pkg, monkeypatch, prec):
    """one greedy member-form launch (pkg.evaluate_actors: M = 3 actors, n_inits = 3 -- the odd pair) on perm_oddA_256: every
    member's rows bit for bit those of its solo rollout, as the README states"""
    monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", "1")
    case, dt, M, K, T = "perm_oddA_256", _dt(prec), 3, 3, 6
    setup, cfg, g = _row(pkg, case, prec)
    ns, A = setup.state_shape
    y0 = to_dev(_cast(kc.inputs(case, K, seed=5)[0], prec), dt)
    actors = []
    for m in range(M):
        dims, P = _actor_params(ns, kc.roll_h(case), 100 + m)
        actors.append(pkg.HipMLP(dims, ["relu", "tanh"], P, dtype=torch.float32, max_cols=K * A))
    res = pkg.evaluate_actors(setup, actors, y0=y0, dtype=dt, steps=T, log=True)
    assert res["one_launch"] is True and res["workgroups"] == M * ((K + 1) // 2)
    assert res["y"].shape[:3] == (T, M, K) and bool((res["done_step"] == -1).all())
    for m, actor in enumerate(actors):
        env = pkg.PDEenv(setup, B=K, dtype=dt, y0=y0, autoreset=False)
        solo = env.rollout(actor.clone(dtype=dt, max_cols=K * A), T, learning=False, log=True)
        torch.cuda.synchronize()
        for k in ("y", "p", "action", "reward"):
            assert _same(res[k][:, m], solo[k]), (m, k)
        assert _same(res["reward_sum"][m], solo["reward_sum"]) and torch.equal(res["done_step"][m], solo["done_step"]), m
        assert bool(torch.isfinite(solo["y"]).all()) and float(solo["action"].abs().max()) > 1e-3
        env.close()
    assert not _same(res["action"][:, 0], res["action"][:, 1])         # the members differ


# ------------------------------------------------------------------ e. reward partials
@pytest.mark.parametrize("case", ["perm_oddA_256", "fd_perm_256"])
def test_reward_partials_are_the_sums_of_the_devices_rewards(pkg, case):
    """pdec_env_set_reward_partials_out, fp32: one partial per work-group (CNAB2: a pair of trajectories, the last one alone;
    finite differences: one trajectory) = the sum of the rewards that work-group wrote"""
    L = pkg._lib
    prec, dt = "f32", torch.float32
    setup, cfg, g = _row(pkg, case, prec)
    y0, act, prev = kc.inputs(case, B)
    env = pkg.PDEenv(setup, B=B, dtype=dt, y0=_cast(y0, prec), autoreset=False)
    n = C.c_int(0)
    part = torch.full((B,), 7.0, dtype=torch.float32, device="cuda:0")
    L.check(env.lib.pdec_env_set_reward_partials_out(env.handle, L.ptr(part), C.byref(n)))
    pair = kc.CASES[case].integrator == "cnab2"
    assert n.value == ((B + 1) // 2 if pair else B)
    env.action.copy_(_act(env, _cast(prev, prec), dt))
    env(_act(env, _cast(act[0], prec), dt))
    torch.cuda.synchronize()
    r = _np(env.reward)
    groups = [list(range(2 * w, min(2 * w + 2, B))) for w in range(n.value)] if pair else [[b] for b in range(B)]
    # a thread adds the rewards it wrote in fp32 (actuator a = tid, tid + nt, ... of each trajectory of its work-group: k terms,
    # k - 1 additions), the 64 lanes of a wave are summed by a 6-level xor tree, the waves in order (nw - 1 additions): every
    # reward passes through at most k - 1 + 6 + nw - 1 roundings, so |partial - sum r| <= depth u sum |r| (1.01: higher orders)
    nt, A = g["nthreads"], g["A"]
    k = len(groups[0]) * -(-A // nt)
    depth = (k - 1) + 6 + (nt // 64 - 1)
    worst = {}
    for w, bs in enumerate(groups):
        assert _err(worst, "partial", float(part[w]), r[bs].sum(), 1.01 * depth * kc.UNIT["f32"] * np.abs(r[bs]).sum()), (w, worst)
    print(f"[ks-geometry reward partials {case} f32] depth {depth} (worst, bound):", worst)
    assert part[n.value:].tolist() == [7.0] * (B - n.value)
    L.check(env.lib.pdec_env_set_reward_partials_out(env.handle, None, None))
    env.close()


# ------------------------------------------------------------------ limits reported, not launched
def test_a2s_out_of_range_is_refused_by_pdec_env_create(pkg):
    """reward_traj / reward_pair read dots[a2s[a]] and gsum[a2s[a]] unwrapped: pdec_env_create requires 0 <= a2s[a] < S of every
    setup -- per-actuator and mono, spectral and finite-difference -- before it allocates or launches anything"""
    from oracle import ks
    lib = pkg._lib.init(0)
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    for case in ("irregular_256", "mono_256", "fd_midpoint_100"):
        setup, cfg, g = _row(pkg, case, "f64")
        G, Ga, a2s = setup.tables()
        for where, bad in ((0, -1), (len(a2s) - 1, g["S"])):
            t = a2s.copy()
            t[where] = bad
            ecfg = setup.env_cfg(1, pkg._lib.dtype_code(torch.float64))
            h = pkg._lib.Handle()
            rc = lib.pdec_env_create(C.byref(h), C.byref(ecfg), G.ctypes.data_as(pd), Ga.ctypes.data_as(pd), t.ctypes.data_as(pi))
            assert rc != 0, (case, where, bad)
            with pytest.raises(pkg.PdecError, match=r"a2s.*out of range"):
                pkg._lib.check(rc)
        pkg.PDEenv(setup, B=1, dtype=torch.float64).close()          # the row's own table is accepted
