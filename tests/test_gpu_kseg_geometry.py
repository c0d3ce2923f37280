"""The 1-D Keller-Segel kernels (csrc/kseg.hip: kseg_env_step_kernel<T, 0 | 1 | 2>, kseg_rollout_kernel<T, MEM, NT>; csrc/env.hip: sense_kernel,
and the band tables pdec_env_create builds) against oracle/keller_segel.py over the geometries of kseg_geometry_cases.py -- the
work-group sizes 64 .. 1024, overlapping actuator boxes, window wrap, permuted actuators, the fmap gather with two species, deep
temporal stacks, one sense_dots group, punishments, the midpoint integrator, all three blow-up tests and both member forms of the
persistent rollout.  test_kseg_geometry_table.py proves without a GPU that each row reaches what it is there for.

Tolerances.  fp64 (device and oracle run the same fixed-step scheme): p 1e-12, state 1e-12, reward 1e-9 (test_env_step_fused),
rhs 1e-9 max(1, |ref|) (test_gpu_kseg.py), y after a control step 1e-11 max(1, |ref|) (test_gpu_kseg2d.py, same stencil), closed
loops 1e-9 (test_reference_trained_keller_segel_actor_closed_loop).  fp32: y 5e-5 and p 1e-5 absolute (test_gpu_kseg.py); the
others from the format, with u = 2^-24 and |y| <= ymax:
  rhs     8 u (4 ymax / dx^2) (1 + 5.6 ymax): a second difference is three products and two sums of terms <= 2 ymax / dx^2, and
          the chemotaxis term multiplies its error by 5.6 u_cell
  state   8 u (5 ymax / 4): a box sum of five cells, scaled by 1/4
  reward  8 u (3.1 + 6 ymax 1.5 / 800): the punishments (<= 0.3 + 0.7 * 4) and 2 |d| delta(d) / 800 with |d| <= 1.5
State and reward of the fused step are compared at the DEVICE's new field (as test_env_step_fused does for the state), so the
integrator's rounding does not enter them."""
import ctypes as C

import numpy as np
import pytest

import kseg_geometry_cases as kc
from util import to_dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U32 = 2.0 ** -24
CASES = list(kc.CASES)
PRECS = ["f64", "f32"]


def _dt(prec):
    return torch.float64 if prec == "f64" else torch.float32


def _mem(y):   # Julia [.., 2, nx] -> memory [.., nx, 2]
    return np.ascontiguousarray(np.swapaxes(y, -1, -2))


def _jl(t):    # device [.., nx, 2] or [.., A, ns] -> Julia-shaped float64 host array
    return np.swapaxes(t.detach().cpu().numpy().astype(np.float64), -1, -2)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _tols(prec, cfg, ymax):
    if prec == "f64":
        return dict(p=1e-12, state=1e-12, reward=1e-9, rhs=lambda ref: 1e-9 * max(1.0, np.abs(ref).max()),
                    y=lambda ref: 1e-11 * max(1.0, np.abs(ref).max()))
    return dict(p=1e-5, state=8 * U32 * 5 * ymax / 4, reward=8 * U32 * (3.1 + 6 * ymax * 1.5 / 800),
                rhs=lambda ref: 8 * U32 * (4 * ymax / cfg.dx ** 2) * (1 + 5.6 * ymax), y=lambda ref: 5e-5)


def _cast(a, prec):
    """the values the device sees: fp32 inputs are rounded once, the oracle then runs in fp64 FROM those values"""
    return np.asarray(a, dtype=np.float32).astype(np.float64) if prec == "f32" else np.asarray(a, dtype=np.float64)


def _bits(t):
    t = t.contiguous()
    return t.view({8: torch.int64, 4: torch.int32}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _err(worst, key, dev, ref, tol):
    e = float(np.abs(dev - ref).max())
    worst[key] = max(worst.get(key, (0.0, tol))[0], e), tol
    return e <= tol


# ------------------------------------------------------------------ a. the pieces through the C ABI
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", CASES)
def test_pieces_match_the_oracle(pkg, case, prec):
    from oracle import keller_segel as kg
    dt, B = _dt(prec), 5
    setup, cfg = kc.build(pkg, kg, case)
    y0, act, prev = kc.inputs(case, B)
    y0, a0, a1 = _cast(y0, prec), _cast(prev, prec), _cast(act[0], prec)
    tol = _tols(prec, cfg, float(np.abs(y0).max()) + 0.1)
    env = pkg.PDEenv(setup, B=B, dtype=dt, autoreset=False)
    yd, a0d, a1d = to_dev(_mem(y0), dt), to_dev(a0, dt).reshape(env._ashape), to_dev(a1, dt).reshape(env._ashape)
    p_dev = env.prepare_action(a1d)
    rhs_dev = env.rhs(yd, p_dev)
    y1_dev, flags = env.do_step(yd, p_dev)
    st0_dev = env.featurize(yd)
    st1_dev = env.featurize(y1_dev, st0_dev)
    r_dev = env.reward_function(y1_dev, a1d, a0d)
    torch.cuda.synchronize()
    assert flags.tolist() == [0] * B
    worst, ok = {}, True
    for b in range(B):
        p_ref = kg.prepare_action(cfg, a1[b][None])
        ok &= _err(worst, "p", _np(p_dev[b]), p_ref, tol["p"])
        p_in = _np(p_dev[b])                                             # downstream pieces: the oracle at the device's own inputs
        ref = kg.f(cfg, y0[b], p_in)
        ok &= _err(worst, "rhs", _jl(rhs_dev[b]), ref, tol["rhs"](ref))
        ref = kc.oracle_step(kg, cfg, case, y0[b], p_in)
        assert np.isfinite(ref).all()
        ok &= _err(worst, "y", _jl(y1_dev[b]), ref, tol["y"](ref))
        s0 = kg.featurize(cfg, y0[b], None)
        ok &= _err(worst, "state0", _jl(st0_dev[b]), s0, tol["state"])
        y1 = _jl(y1_dev[b])
        ok &= _err(worst, "state1", _jl(st1_dev[b]), kg.featurize(cfg, y1, _jl(st0_dev[b])), tol["state"])
        ok &= _err(worst, "reward", _np(r_dev[b]), kg.reward_function(cfg, y1, a1[b][None], (a1[b] - a0[b])[None]), tol["reward"])
    print(f"[kseg-geometry pieces {case} {prec}] (worst, bound):", worst)
    assert ok, worst
    env.close()


# ------------------------------------------------------------------ b. the fused step, three control steps
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", CASES)
def test_fused_step_matches_the_oracle_and_the_pieces(pkg, case, prec):
    from oracle import keller_segel as kg
    dt, B = _dt(prec), 3
    c = kc.CASES[case]
    setup, cfg = kc.build(pkg, kg, case)
    y0, act, prev = kc.inputs(case, B)
    y0, act, prev = _cast(y0, prec), _cast(act, prec), _cast(prev, prec)
    tol = _tols(prec, cfg, float(np.abs(y0).max()) + 0.5)
    env = pkg.PDEenv(setup, B=B, dtype=dt, y0=_mem(y0), autoreset=False)
    pieces = pkg.PDEenv(setup, B=B, dtype=dt, autoreset=False)
    term = torch.full((B, setup.n_actuators), 7.0, dtype=dt, device="cuda:0")
    env.set_terminal_out(term)
    env.action.copy_(to_dev(prev, dt).reshape(env._ashape))
    worst, ok = {}, True
    for b in range(B):
        ok &= _err(worst, "state_reset", _jl(env.state[b]), kg.featurize(cfg, y0[b], None), tol["state"])
    a_prev = prev
    for t in range(act.shape[0]):
        y_in, st_in = env.y.clone(), env.state.clone()
        a_dev = to_dev(act[t], dt).reshape(env._ashape)
        ap_dev = to_dev(a_prev, dt).reshape(env._ashape)
        env(a_dev)
        torch.cuda.synchronize()
        assert env.done.tolist() == [False] * B and float(term.abs().max()) == 0.0        # tame rows (test_kseg_geometry_table.py)
        # the same step composed of the stand-alone pieces, at the same inputs
        p_pc = pieces.prepare_action(a_dev)
        y_pc, _ = pieces.do_step(y_in, p_pc)
        st_pc = pieces.featurize(y_pc, st_in)
        r_pc = pieces.reward_function(y_pc, a_dev, ap_dev)
        torch.cuda.synchronize()
        for b in range(B):
            yb, sb = _jl(y_in[b]), _jl(st_in[b])
            p_ref = kg.prepare_action(cfg, act[t][b][None])
            ok &= _err(worst, "p", _np(env.p[b]), p_ref, tol["p"])
            y_ref = kc.oracle_step(kg, cfg, case, yb, _np(env.p[b]))
            assert np.isfinite(y_ref).all() and np.abs(y_ref).max() < 2.0
            ok &= _err(worst, "y", _jl(env.y[b]), y_ref, tol["y"](y_ref))
            y_new = _jl(env.y[b])
            ok &= _err(worst, "state", _jl(env.state[b]), kg.featurize(cfg, y_new, sb), tol["state"])
            r_ref = kg.reward_function(cfg, y_new, act[t][b][None], (act[t][b] - a_prev[b])[None])
            ok &= _err(worst, "reward", _np(env.reward[b]), r_ref, tol["reward"])
            assert kc.blown(r_ref if c.check_max_value == "reward" else y_new, c.max_value) is False
            ok &= _err(worst, "p_vs_pieces", _np(env.p[b]), _np(p_pc[b]), tol["p"])
            ok &= _err(worst, "y_vs_pieces", _jl(env.y[b]), _jl(y_pc[b]), tol["y"](y_ref))
            ok &= _err(worst, "state_vs_pieces", _jl(env.state[b]), _jl(st_pc[b]), tol["state"] + 1.25 * tol["y"](y_ref))
            ok &= _err(worst, "reward_vs_pieces", _np(env.reward[b]), _np(r_pc[b]), tol["reward"] + tol["y"](y_ref))
        a_prev = act[t]
    print(f"[kseg-geometry fused {case} {prec}] (worst, bound):", worst)
    assert ok, worst
    if c.temporal_steps > 1:       # the stack really shifted: the oldest block is the newest block of two steps ago
        fresh = c.window_size * 2
        assert not _same(env.state[:, :, :fresh], env.state[:, :, fresh:2 * fresh])
    env.close(), pieces.close()


# ------------------------------------------------------------------ c. blow-up handling
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("check", ["y", "reward", "off"])
@pytest.mark.parametrize("case", kc.BLOWUP)
def test_blowup_flags_and_untouched_neighbours(pkg, case, check, prec):
    """B = 5 with trajectory 1 patched past max_value and one NaN cell in trajectory 3 (ordinary data: the fields are plain
    numbers to every kernel): done and the per-column terminal rows are what the oracle's field / reward say under each
    check_max_value, and trajectories 0, 2, 4 come out bit for bit as from the batch without the two"""
    from oracle import keller_segel as kg
    dt, B = _dt(prec), 5
    mv = kc.BLOWUP_REWARD_MAX if check == "reward" else 20.0
    setup, cfg = kc.build(pkg, kg, case, check_max_value=check, max_value=mv)
    y0, bad, act, prev = kc.blowup_inputs(case, B)
    bad, act, prev = _cast(bad, prec), _cast(act, prec), _cast(prev, prec)
    want = []
    for b in range(B):
        with np.errstate(all="ignore"):
            y = kc.oracle_step(kg, cfg, case, bad[b], kg.prepare_action(cfg, act[b][None]))
            r = kg.reward_function(cfg, y, act[b][None], (act[b] - prev[b])[None])
        want.append(False if check == "off" else kc.blown(r if check == "reward" else y, mv))
    if check != "off":
        assert want == [False, True, False, True, False]          # both sides of the bound present, on the oracle's numbers
    out = {}
    for name, fields in (("tame", _cast(y0, prec)), ("bad", bad)):
        env = pkg.PDEenv(setup, B=B, dtype=dt, y0=_mem(fields), autoreset=False)
        term = torch.full((B, setup.n_actuators), 7.0, dtype=dt, device="cuda:0")
        env.set_terminal_out(term)
        env.action.copy_(to_dev(prev, dt).reshape(env._ashape))
        env(to_dev(act, dt).reshape(env._ashape))
        torch.cuda.synchronize()
        out[name] = dict(y=env.y.clone(), p=env.p.clone(), state=env.state.clone(), reward=env.reward.clone(),
                         done=env.done.tolist(), term=term.clone())
        env.close()
    assert out["tame"]["done"] == [False] * B and float(out["tame"]["term"].abs().max()) == 0.0
    assert out["bad"]["done"] == want
    exp_term = torch.tensor(want, dtype=dt, device="cuda:0")[:, None].expand(B, setup.n_actuators)
    assert torch.equal(out["bad"]["term"], exp_term), out["bad"]["term"]
    for k in ("y", "p", "state", "reward"):
        assert _same(out["bad"][k][[0, 2, 4]], out["tame"][k][[0, 2, 4]]), k
    assert bool(torch.isnan(out["bad"]["y"][3]).any()) and bool(torch.isfinite(out["bad"]["y"][1]).all())
    assert float(out["bad"]["y"][1].abs().max()) > 1.2 * 20.0


# ------------------------------------------------------------------ d. rollouts
def _actor_params(ns, seed):
    rng = np.random.default_rng(seed)
    dims = [ns, kc.ROLL_H, 1]
    P = []
    for i in range(2):
        lim = np.sqrt(6.0 / (dims[i] + dims[i + 1]))
        P += [rng.uniform(-lim, lim, (dims[i + 1], dims[i])).astype(np.float32), rng.uniform(-0.1, 0.1, dims[i + 1]).astype(np.float32)]
    return dims, P


def _oracle_closed_loop(cfg, case, P, y0, T, ft):
    """T steps of actor -> prepare_action -> integrator -> reward -> featurize in the oracle, every array of type `ft`
    (np.float32: the oracle's own routines on float32 tables, weights and fields -- the rounding level of the scheme)"""
    import copy
    from oracle import keller_segel as kg, nn
    c = kc.CASES[case]
    assert c.integrator == "rk4"
    cf = copy.copy(cfg)
    cf.gaussians, cf.gaussians_actuators = cfg.gaussians.astype(ft), cfg.gaussians_actuators.astype(ft)
    Pf = [p.astype(ft) for p in P]
    A = len(c.actuators_to_sensors)
    y = y0.astype(ft)
    state, a_prev, ret, h = kg.featurize(cf, y, None), np.zeros((1, A), dtype=ft), np.zeros(A, dtype=ft), cfg.dt / c.substeps
    rows = dict(action=[], p=[], y=[], reward=[])
    for t in range(T):
        a = np.clip(nn.forward(Pf, [nn.RELU, nn.TANH], state), -1, 1).astype(ft)
        p = kg.prepare_action(cf, a).astype(ft)
        for _ in range(c.substeps):
            y = kg.rk4_step(cf, y, p, h)
        r = kg.reward_function(cf, y, a, a - a_prev)
        state, a_prev, ret = kg.featurize(cf, y, state), a, ret + r
        assert y.dtype == ft and state.dtype == ft and r.dtype == ft and a.dtype == ft
        for k, v in zip(("action", "p", "y", "reward"), (a[0], p, y, r)):
            rows[k].append(v)
    out = {k: np.stack(v) for k, v in rows.items()}
    out.update(state=state, ret=ret)
    return out


def _launches(env, label):
    ms, n = C.c_double(), C.c_int()
    env.lib.pdec_sync(env.handle)
    assert env.lib.pdec_prof_get(env.handle, label.encode(), C.byref(ms), C.byref(n)) == 0
    return n.value


def _served(pkg, case, prec):
    """does the persistent launch take this row (kseg_rollout_lds restated, held against the source's figures by
    test_kseg_geometry_table.py); the library's own launch labels are asked as well where a handle is at hand"""
    from oracle import keller_segel as kg
    c = kc.CASES[case]
    setup, _ = kc.build(pkg, kg, case)
    g = kc.geometry(*setup.tables(), case)
    return kc.rollout_served(g, 8 if prec == "f64" else 4, c.check_max_value), g


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", kc.ROLLOUT)
def test_rollout_greedy_follows_the_oracle_and_learning_the_step_loop(pkg, monkeypatch, case, prec):
    """env.rollout in its solo form (kseg_rollout_kernel<T, false, 1024> where kseg_rollout_lds <= 64 KiB, the enqueued step loop
    where not): greedy against oracle.nn + the oracle environment (fp64, 1e-9), greedy and learning = True against the
    step-by-step loop pdec_policy_act_rng -> (env)(action) of the same Philox stream (the persistent launch sums the actor's
    layers in another order than the acting kernel: fp64 2e-12 actions / 2e-11 fields, fp32 2e-6 / 2e-5, p ten times that --
    test_rollout_equals_step_by_step_loop's figures; bit for bit where the step loop serves)"""
    from oracle import keller_segel as kg
    monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", "1")
    L = pkg._lib
    dt, B, T = _dt(prec), 3, 5
    served, g = _served(pkg, case, prec)
    setup, cfg = kc.build(pkg, kg, case)
    ns, A = setup.state_shape
    y0 = _cast(kc.inputs(case, B, seed=3)[0], prec)
    dims, P = _actor_params(ns, 11)
    actor = pkg.HipMLP(dims, ["relu", "tanh"], P, dtype=dt, max_cols=B * A)
    P64 = [p.astype(np.float64) for p in P]
    cols = B * A
    for learning, noise, seed in ((False, 0.0, 0), (True, 0.3, 99)):
        ref_env = pkg.PDEenv(setup, B=B, dtype=dt, y0=_mem(y0), autoreset=False)
        env = pkg.PDEenv(setup, B=B, dtype=dt, y0=_mem(y0), autoreset=False)
        rows, rsum, off = [], torch.zeros_like(ref_env.reward), 0
        for t in range(T):
            a = torch.empty(ref_env._ashape, dtype=dt, device="cuda:0")
            L.check(ref_env.lib.pdec_policy_act_rng(actor.handle, L.ptr(ref_env.state), cols, noise, 1.0, int(learning), seed, off, L.ptr(a)))
            off += (cols + 3) // 4
            ref_env(a)
            rsum += ref_env.reward
            rows.append((ref_env.y.clone(), ref_env.p.clone(), ref_env.action.clone(), ref_env.reward.clone()))
        L.check(env.lib.pdec_prof_reset(env.handle))
        L.check(env.lib.pdec_prof_enable(env.handle, 1))
        out = env.rollout(actor, T, act_noise=noise, act_limit=1.0, learning=learning, seed=seed, offset=0, log=True)
        torch.cuda.synchronize()
        one, steps = _launches(env, "kseg_rollout"), _launches(env, "kseg_env_step")
        L.check(env.lib.pdec_prof_enable(env.handle, 0))
        assert (one, steps) == ((1, 0) if served else (0, T)), (one, steps, served)
        assert out["done_step"].tolist() == [-1] * B and env.steps == T
        if served:
            sc = 1e-6 if prec == "f64" else 1.0
            close = lambda x, y, tol: float((x - y).abs().max()) <= tol * sc
            assert close(out["action"][0], rows[0][2], 2e-6)
            assert close(env.y, ref_env.y, 2e-5) and close(env.state, ref_env.state, 2e-5) and close(env.action, ref_env.action, 2e-5)
            assert close(out["reward_sum"], rsum, 2e-5)
            for t in range(T):
                assert close(out["y"][t], rows[t][0], 2e-5) and close(out["p"][t], rows[t][1], 2e-4), t
                assert close(out["action"][t], rows[t][2], 2e-5) and close(out["reward"][t], rows[t][3], 2e-5), t
        else:
            assert _same(env.y, ref_env.y) and _same(env.state, ref_env.state) and _same(env.action, ref_env.action)
            assert _same(out["reward_sum"], rsum)
            for t in range(T):
                for k, name in enumerate(("y", "p", "action", "reward")):
                    assert _same(out[name][t], rows[t][k]), (t, name)
        if learning:       # the noise is there and the clamp has work to do
            assert not _same(out["action"][0], greedy_first) and float(out["action"].abs().max()) <= 1.0
        else:
            greedy_first = out["action"][0].clone()
        if not learning:
            # the oracle's closed loop: fp64 to 1e-9; fp32 to 4 x the rounding level of the scheme itself, which is the oracle's
            # own routines run in float32 on the host (inputs, tables and weights cast) against the fp64 loop, per quantity
            worst, level = {}, {}
            for b in range(B):
                ref = _oracle_closed_loop(cfg, case, P, y0[b], T, np.float64)
                if prec == "f32":
                    r32 = _oracle_closed_loop(cfg, case, P, y0[b], T, np.float32)
                    for k in ref:
                        level[k] = max(level.get(k, 0.0), float(np.abs(r32[k].astype(np.float64) - ref[k]).max()))
                dev = dict(action=_np(out["action"][:, b, :, 0]), p=_np(out["p"][:, b]), y=_jl(out["y"][:, b]),
                           reward=_np(out["reward"][:, b]), state=_jl(env.state[b]), ret=_np(out["reward_sum"][b]))
                for k in ref:
                    worst[k] = max(worst.get(k, 0.0), float(np.abs(dev[k] - ref[k]).max()))
                assert np.isfinite(ref["y"]).all() and np.abs(ref["y"]).max() < 2.0 and np.abs(ref["action"]).max() > 1e-3
            bound = {k: 1e-9 for k in worst} if prec == "f64" else {k: 4 * v for k, v in level.items()}
            print(f"[kseg-geometry rollout {case} {prec}] deviation from the oracle's closed loop:", worst, "bound:", bound,
                  "float32 level of the oracle:", level)
            assert all(worst[k] <= bound[k] for k in worst), (worst, bound)
        env.close(), ref_env.close()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", kc.ROLLOUT)
def test_member_rollout_equals_the_solo_rollouts(pkg, monkeypatch, case, prec):
    """pkg.evaluate_actors (pdec_rollout_members: kseg_rollout_kernel<T, true, 256> up to 256 threads, <T, true, 1024> above) --
    every member's rows bit for bit those of its solo rollout, as test_gpu_population_eval.py asks at the shipped geometry;
    where the persistent form does not serve (1024 cells, 100 actuators, fp64) one_launch is False and the rows are the solo
    rollouts' all the same"""
    from oracle import keller_segel as kg
    monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", "1")
    dt, M, K, T = _dt(prec), 3, 3, 5
    served, g = _served(pkg, case, prec)
    setup, cfg = kc.build(pkg, kg, case)
    ns, A = setup.state_shape
    y0 = to_dev(_mem(kc.inputs(case, K, seed=5)[0]), dt)
    actors = []
    for m in range(M):
        dims, P = _actor_params(ns, 100 + m)
        actors.append(pkg.HipMLP(dims, ["relu", "tanh"], P, dtype=torch.float32, max_cols=K * A))
    res = pkg.evaluate_actors(setup, actors, y0=y0, dtype=dt, steps=T, log=True)
    assert res["one_launch"] is served
    assert res["workgroups"] == (M * K if served else None)
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
    # the launch itself, by the library's own label: pdec_rollout_members on an environment of this test, profiled.  The label
    # "kseg_rollout_members" is kseg_rollout_launch's member branch, which picks kseg_rollout_kernel<T, true, 256> up to 256
    # threads and <T, true, 1024> above (csrc/kseg.hip); a kernel trace of this test names both instantiations
    L = pkg._lib
    env = pkg.PDEenv(setup, B=M * K, dtype=dt, y0=y0.repeat(M, 1, 1), autoreset=False)
    L.check(env.lib.pdec_prof_reset(env.handle))
    L.check(env.lib.pdec_prof_enable(env.handle, 1))
    handles = (L.Handle * M)(*[int(getattr(a.handle, "value", a.handle)) for a in actors])
    rsum = torch.zeros((M * K, A), dtype=dt, device="cuda:0")
    log_y = torch.empty((T,) + env._yshape, dtype=dt, device="cuda:0")
    got = C.c_int(0)
    L.check(env.lib.pdec_rollout_members(env.handle, handles, M, K, T, L.ptr(env.y), L.ptr(env.state), L.ptr(env.action), 1.0, 0,
                                         L.ptr(rsum), L.ptr(log_y), None, None, None, None, None, C.byref(got)))
    torch.cuda.synchronize()
    assert bool(got.value) is served
    assert (_launches(env, "kseg_rollout_members"), _launches(env, "kseg_rollout"), _launches(env, "kseg_env_step")) == \
        ((1, 0, 0) if served else (0, 0, 0))
    L.check(env.lib.pdec_prof_enable(env.handle, 0))
    if served:
        assert _same(log_y.view((T, M, K) + tuple(log_y.shape[2:])), res["y"]) and _same(rsum.view(M, K, A), res["reward_sum"])
        assert g["nthreads"] == {"wrap_nx100": 128, "fmap_w3_nx100": 128, "roll_nx320": 320, "nx1024": 1024}[case]
    env.close()
    assert not _same(res["action"][:, 0], res["action"][:, 1])         # the members differ


# ------------------------------------------------------------------ sense_dots' 8-row unrolled body
@pytest.mark.parametrize("prec", PRECS)
def test_wide_boxes_reach_the_unrolled_sense_body(pkg, prec):
    """21-cell boxes (kc.build_wide: one sense_dots group of 21 band rows = two unrolled passes of 8 and a tail of 5, in the step
    kernel and in the stand-alone closures): featurize and reward alone, and two fused steps, against the oracle built with the
    same half window.  fp32 bounds as in the module docstring with 21 cells per box instead of 5 (|d| <= 21 * 0.3)."""
    from oracle import keller_segel as kg
    dt, B = _dt(prec), 3
    setup, cfg = kc.build_wide(pkg, kg)
    y0, act, prev = kc.inputs(kc.WIDE, B)
    y0, act, prev = _cast(y0, prec), _cast(act, prec), _cast(prev, prec)
    ymax = float(np.abs(y0).max()) + 0.5
    tol = _tols(prec, cfg, ymax)
    if prec == "f32":
        tol.update(state=8 * U32 * 21 * ymax / 4, reward=8 * U32 * (3.1 + 2 * 6.3 * 21 * ymax / 800))
    env = pkg.PDEenv(setup, B=B, dtype=dt, y0=_mem(y0), autoreset=False)
    env.action.copy_(to_dev(prev, dt).reshape(env._ashape))
    worst, ok = {}, True
    st0 = env.featurize(to_dev(_mem(y0), dt))
    r0 = env.reward_function(to_dev(_mem(y0), dt), to_dev(act[0], dt).reshape(env._ashape), to_dev(prev, dt).reshape(env._ashape))
    torch.cuda.synchronize()
    for b in range(B):
        ok &= _err(worst, "featurize", _jl(st0[b]), kg.featurize(cfg, y0[b], None), tol["state"])
        ok &= _err(worst, "reward_fn", _np(r0[b]), kg.reward_function(cfg, y0[b], act[0][b][None], (act[0][b] - prev[b])[None]), tol["reward"])
        ok &= _err(worst, "state_reset", _jl(env.state[b]), kg.featurize(cfg, y0[b], None), tol["state"])
    a_prev = prev
    for t in range(2):
        y_in, st_in = env.y.clone(), env.state.clone()
        env(to_dev(act[t], dt).reshape(env._ashape))
        torch.cuda.synchronize()
        assert env.done.tolist() == [False] * B
        for b in range(B):
            ok &= _err(worst, "p", _np(env.p[b]), kg.prepare_action(cfg, act[t][b][None]), tol["p"])
            y_ref = kg.do_step(cfg, _jl(y_in[b]), _np(env.p[b]), 32)
            ok &= _err(worst, "y", _jl(env.y[b]), y_ref, tol["y"](y_ref))
            y_new = _jl(env.y[b])
            ok &= _err(worst, "state", _jl(env.state[b]), kg.featurize(cfg, y_new, _jl(st_in[b])), tol["state"])
            ok &= _err(worst, "reward", _np(env.reward[b]), kg.reward_function(cfg, y_new, act[t][b][None], (act[t][b] - a_prev[b])[None]), tol["reward"])
        a_prev = act[t]
    print(f"[kseg-geometry wide boxes {prec}] (worst, bound):", worst)
    assert ok, worst
    env.close()


# ------------------------------------------------------------------ e. limits reported, not launched
def test_grid_limits_are_refused_at_creation(pkg):
    from oracle import keller_segel as kg
    big = pkg.KellerSegelSetup(nx=1025, Lx=102.5, sensor_positions=np.arange(3, 1024, 5), actuators_to_sensors=np.arange(3, 19))
    with pytest.raises(pkg.PdecError, match=r"N=1025 too large for the one-cell-per-thread"):
        pkg.PDEenv(big, B=1, dtype=torch.float64)
    # nx = 3 holds no 5-cell box, so no setup exists for it: the configuration struct goes to pdec_env_create directly
    small = pkg.KellerSegelSetup(nx=8, Lx=0.8, sensor_positions=[3, 4, 5, 6], actuators_to_sensors=[1, 2, 3, 4])
    lib = pkg._lib.init(0)
    cfg = small.env_cfg(1, pkg._lib.dtype_code(torch.float64))
    cfg.N = 3
    G, Ga, a2s = np.ones((4, 3)), np.ones((4, 3)), np.arange(4, dtype=np.int32)
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    h = pkg._lib.Handle()
    rc = lib.pdec_env_create(C.byref(h), C.byref(cfg), G.ctypes.data_as(pd), Ga.ctypes.data_as(pd), a2s.ctypes.data_as(pi))
    assert rc != 0
    with pytest.raises(pkg.PdecError, match=r"bad sizes B=1 N=3 "):
        pkg._lib.check(rc)
    # ... and the smallest grid the table runs is accepted
    pkg.PDEenv(small, B=1, dtype=torch.float64).close()
