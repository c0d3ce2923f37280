"""The 2-D Keller-Segel kernels (csrc/kseg2d.hip: kseg2d_rk4_kernel<T, 1 | 2, 0 | 1 | 2>, kseg2d_actuate_kernel,
kseg2d_boxsum_kernel, kseg2d_feat_kernel, kseg2d_terminal_kernel, the split batch of k2_integrate, and pdec_env_autoreset on the
2-D layout) against oracle/keller_segel2d.py over the geometries of kseg2d_geometry_cases.py -- one tile and ragged last tiles in
both precisions, the XCD-aware tile order with a tile count that does not divide 8, both second passes of the box-sum loops,
boxes clipped by the domain edge, other windows and stacks, punishments, all three blow-up tests, the two-sub-step variant, the
split batch with a ragged tile and the fp32 gather kernels.  test_kseg2d_geometry_table.py proves without a GPU that each row
reaches what it is there for.

Tolerances are the project's own.  fp64: p 1e-13, y / reward / state 1e-11 max(1, |ref|) (test_env_step_fused), rhs
1e-11 max |ref| (test_rhs_matches_oracle).  fp32: p 1e-5 (test_env_step_at_the_benchmarked_size_matches_oracle), y / reward /
state 2e-5 max(1, |ref|) (TOL_K2, tests/pipeline_ref.py), rhs per cell 4 * 2^-24 * mag, mag = the oracle's f with every term
replaced by its absolute value (kc.mag): one rounding per operation of k2_rhs_pair sums to about one unit of that scale, the
factor 4 is margin for the contraction into FMAs.  fp32 inputs are rounded to fp32 first and the oracle runs in fp64 FROM those
values; every control step is compared from the device's own previous field."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import kseg2d_geometry_cases as kc
from util import to_dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U32 = 2.0 ** -24
ROWS = [(case, prec) for case in kc.CASES for prec in kc.CASES[case].precs]
PRECS = ["f64", "f32"]


def _dt(prec):
    return torch.float64 if prec == "f64" else torch.float32


def _mem(y):        # host [.., 2, ny, nx] -> memory [.., ny, nx, 2]
    return np.ascontiguousarray(np.moveaxis(y, -3, -1))


def _host(t):       # memory [.., ny, nx, 2] -> host [.., 2, ny, nx]
    return np.moveaxis(t.detach().cpu().numpy().astype(np.float64), -1, -3)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _cast(a, prec):
    """the values the device sees: fp32 inputs are rounded once, the oracle then runs in fp64 FROM those values"""
    return np.asarray(a, dtype=np.float32).astype(np.float64) if prec == "f32" else np.asarray(a, dtype=np.float64)


def _bits(t):
    t = t.contiguous()
    return t.view({8: torch.int64, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _tol(prec):
    return dict(p=1e-13, rel=1e-11) if prec == "f64" else dict(p=1e-5, rel=2e-5)


def _rel(worst, key, dev, ref, rel):
    """max |dev - ref| / max(1, max |ref|) against `rel`; keeps the largest figure per key"""
    e = float(np.abs(dev - ref).max()) / max(1.0, float(np.abs(ref).max()))
    worst[key] = max(worst.get(key, 0.0), e)
    return e <= rel


def _abs(worst, key, dev, ref, tol):
    e = float(np.abs(dev - ref).max())
    worst[key] = max(worst.get(key, 0.0), e)
    return e <= tol


def _act(env, a, dt):
    return to_dev(a, dt).reshape(env._ashape)


def _oracle_step(k2, cfg, y, a, a_prev, st_prev):
    p = k2.prepare_action(cfg, a)
    with np.errstate(all="ignore"):
        y1 = k2.do_step(cfg, y, p)
        r = k2.reward_function(cfg, y1, a, a - a_prev)
        st = k2.featurize(cfg, y1, st_prev)
    return p, y1, r, st


# ------------------------------------------------------------------ a. the right-hand side, both precisions
@pytest.mark.parametrize("case,prec", ROWS)
def test_rhs_matches_the_oracle(pkg, case, prec):
    """kseg2d_rk4_kernel<T, 1, 1>.  Largest fp32 ratio |got - ref| / (2^-24 mag) measured per row: DESIGN.md"""
    from oracle import keller_segel2d as k2
    c, dt = kc.CASES[case], _dt(prec)
    setup, cfg = kc.build(pkg, k2, case)
    y0, act, _ = kc.inputs(case)
    y0, a = _cast(y0, prec), _cast(act[0], prec)
    env = pkg.PDEenv(setup, B=c.B, dtype=dt, autoreset=False)
    p_dev = env.prepare_action(_act(env, a, dt))
    out = _host(env.rhs(to_dev(_mem(y0), dt), p_dev))
    p_in = _np(p_dev)
    worst, ok = {}, True
    for b in kc.picks(case):
        ok &= _abs(worst, "p", p_in[b], k2.prepare_action(cfg, a[b]), _tol(prec)["p"])
        ref = k2.f(cfg, y0[b], p_in[b])                          # the oracle at the device's own forcing
        assert np.isfinite(ref).all() and np.isfinite(out[b]).all()
        if prec == "f64":
            e = float(np.abs(out[b] - ref).max() / (1e-11 * np.abs(ref).max()))
            worst["rhs / (1e-11 max|ref|)"] = max(worst.get("rhs / (1e-11 max|ref|)", 0.0), e)
            ok &= e <= 1.0
        else:
            ratio = np.abs(out[b] - ref) / (U32 * kc.mag(cfg, y0[b], p_in[b]))
            worst["rhs / (2^-24 mag)"] = max(worst.get("rhs / (2^-24 mag)", 0.0), float(ratio.max()))
            ok &= bool((ratio <= 4.0).all())
    print(f"[kseg2d-geometry rhs {case} {prec}] worst:", worst)
    assert ok, worst
    env.close()


# ------------------------------------------------------------------ b. do_step, the closures and the fused step
@pytest.mark.parametrize("case,prec", ROWS)
def test_fused_step_and_closures_match_the_oracle(pkg, case, prec):
    """three control steps of (env)(action) from kc.inputs: p, y, reward and state of every step and every trajectory of the row
    (of a split row: kc.picks) against the oracle, each step from the device's own previous field; do_step, prepare_action,
    featurize (reset form and with the previous state) and reward_function alone on the same fields"""
    from oracle import keller_segel2d as k2
    c, dt, tol = kc.CASES[case], _dt(prec), _tol(prec)
    setup, cfg = kc.build(pkg, k2, case)
    y0, act, prev = kc.inputs(case)
    y0, act, prev = _cast(y0, prec), _cast(act, prec), _cast(prev, prec)
    B, A = c.B, cfg.A
    env = pkg.PDEenv(setup, B=B, dtype=dt, y0=_mem(y0), action0=_act_shape(prev, B, A), autoreset=False)
    pieces = pkg.PDEenv(setup, B=B, dtype=dt, autoreset=False)
    term = torch.full((B, A), 7.0, dtype=dt, device="cuda:0")
    env.set_terminal_out(term)
    picks = kc.picks(case)
    worst, ok = {}, True
    st0 = pieces.featurize(to_dev(_mem(y0), dt), None)
    for b in picks:
        ref = k2.featurize(cfg, y0[b], None)
        ok &= _rel(worst, "state_reset", _np(env.state[b]).T, ref, tol["rel"])
        ok &= _rel(worst, "featurize_reset", _np(st0[b]).T, ref, tol["rel"])
    a_prev = prev
    for t in range(act.shape[0]):
        y_in, st_in = env.y.clone(), env.state.clone()
        a_dev, ap_dev = _act(env, act[t], dt), _act(env, a_prev, dt)
        env(a_dev)
        p_pc = pieces.prepare_action(a_dev)
        y_pc, flags = pieces.do_step(y_in, p_pc)
        st_pc = pieces.featurize(y_pc, st_in)
        r_pc = pieces.reward_function(y_pc, a_dev, ap_dev)
        torch.cuda.synchronize()
        assert env.done.tolist() == [False] * B and int(flags.abs().sum()) == 0 and float(term.abs().max()) == 0.0
        y_in_h, y_new, y_pc_h = _host(y_in), _host(env.y), _host(y_pc)
        for b in picks:
            sb = _np(st_in[b]).T
            p_ref, y_ref, r_ref, st_ref = _oracle_step(k2, cfg, y_in_h[b], act[t][b], a_prev[b], sb)
            assert np.isfinite(y_ref).all() and np.abs(y_ref).max() < 2.0
            ok &= _abs(worst, "p", _np(env.p[b]), p_ref, tol["p"])
            ok &= _rel(worst, "y", y_new[b], y_ref, tol["rel"])
            ok &= _rel(worst, "reward", _np(env.reward[b]), r_ref, tol["rel"])
            ok &= _rel(worst, "state", _np(env.state[b]).T, st_ref, tol["rel"])
            # the stand-alone closures: do_step at the field p, the sensing closures at the field do_step made
            ok &= _abs(worst, "prepare_action", _np(p_pc[b]), p_ref, tol["p"])
            ok &= _rel(worst, "do_step", y_pc_h[b], k2.do_step(cfg, y_in_h[b], _np(p_pc[b])), tol["rel"])
            ok &= _rel(worst, "featurize", _np(st_pc[b]).T, k2.featurize(cfg, y_pc_h[b], sb), tol["rel"])
            ok &= _rel(worst, "reward_function", _np(r_pc[b]),
                       k2.reward_function(cfg, y_pc_h[b], act[t][b], act[t][b] - a_prev[b]), tol["rel"])
        a_prev = act[t]
    print(f"[kseg2d-geometry fused {case} {prec}] worst (bound {tol}):", worst)
    assert ok, worst
    if c.temporal_steps > 1:       # the stack really shifted: the second block is the first block of the step before
        fresh = 2 * c.window_size ** 2
        assert _same(env.state[:, :, fresh:2 * fresh], st_in[:, :, :fresh]) and not _same(env.state[:, :, :fresh], st_in[:, :, :fresh])
    env.close(), pieces.close()


def _act_shape(a, B, A):
    return np.ascontiguousarray(a).reshape(B, A, 1)


# ------------------------------------------------------------------ c. the two-sub-step variant
def _nsub2_env(pkg, monkeypatch, setup, **kw):
    """PDEC_KSEG2D_NSUB2 is read by pdec_kseg2d_env_create: set around the environment's creation only"""
    monkeypatch.setenv("PDEC_KSEG2D_NSUB2", "1")
    try:
        return pkg.PDEenv(setup, **kw)
    finally:
        monkeypatch.delenv("PDEC_KSEG2D_NSUB2")


@pytest.mark.parametrize("K", [3, 4, 5])
@pytest.mark.parametrize("case", kc.NSUB2)
def test_two_substep_variant_matches_the_oracle(pkg, monkeypatch, case, K):
    """kseg2d_rk4_kernel<float, 2, 0> (halo 8, an 80 x 80 region) with the single sub-step launch that ends an odd K
    (kc.nsub2_launches: 2 + 1, 2 + 2, 2 + 2 + 1): do_step and one fused step against the oracle at the fp32 bound.  (The launch
    list itself is not observable: the library times the whole sub-step loop under one label.)"""
    from oracle import keller_segel2d as k2
    c, dt, tol, prec = kc.CASES[case], torch.float32, _tol("f32"), "f32"
    setup, cfg = kc.build(pkg, k2, case, substeps=K)
    y0, act, prev = kc.inputs(case, steps=1)
    y0, a, prev = _cast(y0, prec), _cast(act[0], prec), _cast(prev, prec)
    B, A = c.B, cfg.A
    env = _nsub2_env(pkg, monkeypatch, setup, B=B, dtype=dt, y0=_mem(y0), action0=_act_shape(prev, B, A), autoreset=False)
    assert "PDEC_KSEG2D_NSUB2" not in os.environ and env.n_part_streams == 0
    st_in = env.state.clone()
    p_dev = env.prepare_action(_act(env, a, dt))
    y_pc, flags = env.do_step(to_dev(_mem(y0), dt), p_dev)
    env(_act(env, a, dt))
    torch.cuda.synchronize()
    assert env.done.tolist() == [False] * B and int(flags.abs().sum()) == 0
    worst, ok = {}, True
    y_new, y_pc_h = _host(env.y), _host(y_pc)
    for b in range(B):
        p_ref, y_ref, r_ref, st_ref = _oracle_step(k2, cfg, y0[b], a[b], prev[b], _np(st_in[b]).T)
        assert np.isfinite(y_ref).all()
        ok &= _abs(worst, "p", _np(env.p[b]), p_ref, tol["p"])
        ok &= _rel(worst, "do_step", y_pc_h[b], k2.do_step(cfg, y0[b], _np(p_dev[b])), tol["rel"])
        ok &= _rel(worst, "y", y_new[b], y_ref, tol["rel"])
        ok &= _rel(worst, "reward", _np(env.reward[b]), r_ref, tol["rel"])
        ok &= _rel(worst, "state", _np(env.state[b]).T, st_ref, tol["rel"])
    print(f"[kseg2d-geometry nsub2 {case} K={K}] worst (bound {tol}):", worst)
    assert ok, worst
    env.close()


# ------------------------------------------------------------------ d. blow-up handling
def _blowup_run(pkg, setup, fields, act, prev, dt, autoreset):
    B, A = fields.shape[0], setup.n_actuators
    env = pkg.PDEenv(setup, B=B, dtype=dt, y0=_mem(fields), action0=_act_shape(prev, B, A), autoreset=autoreset)
    term = torch.full((B, A), 7.0, dtype=dt, device="cuda:0")
    env.set_terminal_out(term)
    state0 = env.state.clone()
    env(_act(env, act, dt))
    torch.cuda.synchronize()
    out = dict(y=env.y.clone(), p=env.p.clone(), state=env.state.clone(), reward=env.reward.clone(), action=env.action.clone(),
               done=env.done.tolist(), term=term.clone(), y0=env.y0.clone(), state0=state0, action0=env.action0.clone())
    env.close()
    return out


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", kc.BLOWUP + ["nocheck_68x65"])
def test_blowup_flags_terminal_columns_and_autoreset(pkg, case, prec):
    """kc.blowup_inputs (B = 5: trajectory 1 patched past max_value, one NaN cell in trajectory 3): `done` is the oracle's
    predicate not all(|x| <= max_value) per trajectory -- x the field, or the rewards under check_max_value = "reward" -- the
    terminal columns follow it, the untouched trajectories meet the oracle, "off" raises nothing; with autoreset the raised
    trajectories come back as their initial images bit for bit with finite rewards and the others are unchanged"""
    from oracle import keller_segel2d as k2
    c, dt, tol, B = kc.CASES[case], _dt(prec), _tol(prec), kc.BLOWUP_B
    setup, cfg = kc.build(pkg, k2, case)
    _, bad, act, prev = kc.blowup_inputs(case)
    bad, act, prev = _cast(bad, prec), _cast(act, prec), _cast(prev, prec)
    st0 = [k2.featurize(cfg, bad[b], None) for b in range(B)]
    refs, want = [], []
    for b in range(B):
        refs.append(_oracle_step(k2, cfg, bad[b], act[b], prev[b], st0[b]))
        x = refs[b][2] if c.check_max_value == "reward" else refs[b][1]
        want.append(False if c.check_max_value == "off" else kc.blown(x, c.max_value))
    assert want == ([False] * B if c.check_max_value == "off" else [False, True, False, True, False])
    out = _blowup_run(pkg, setup, bad, act, prev, dt, autoreset=False)
    assert out["done"] == want
    exp_term = torch.tensor(want, dtype=dt, device="cuda:0")[:, None].expand(B, cfg.A)
    assert torch.equal(out["term"], exp_term), out["term"]
    worst, ok = {}, True
    y_new = _host(out["y"])
    for b in (0, 2, 4):                                     # the untouched trajectories still meet the oracle
        p_ref, y_ref, r_ref, st_ref = refs[b]
        ok &= _abs(worst, "p", _np(out["p"][b]), p_ref, tol["p"])
        ok &= _rel(worst, "y", y_new[b], y_ref, tol["rel"])
        ok &= _rel(worst, "reward", _np(out["reward"][b]), r_ref, tol["rel"])
        ok &= _rel(worst, "state", _np(out["state"][b]).T, st_ref, tol["rel"])
    # the patched one too: finite, past the bound, and the oracle's field (the patch is ordinary data to the kernel)
    ok &= _rel(worst, "y_patched", y_new[1], refs[1][1], tol["rel"])
    assert bool(torch.isfinite(out["y"][1]).all()) and float(out["y"][1].abs().max()) > 1.2 * 20.0
    assert bool(torch.isnan(out["y"][3]).any())
    print(f"[kseg2d-geometry blowup {case} {prec}] worst (bound {tol}):", worst)
    assert ok, worst
    # ---- the same step with autoreset
    rst = _blowup_run(pkg, setup, bad, act, prev, dt, autoreset=True)
    assert rst["done"] == want and torch.equal(rst["term"], exp_term)
    assert _same(rst["y0"], to_dev(_mem(bad), dt)) and _same(rst["action0"], to_dev(_act_shape(prev, B, cfg.A), dt))
    for b in range(B):
        if want[b]:
            assert _same(rst["y"][b], rst["y0"][b]) and _same(rst["state"][b], rst["state0"][b]), b
            assert _same(rst["action"][b], rst["action0"][b]) and bool(torch.isfinite(rst["reward"][b]).all()), b
        else:
            for k in ("y", "state", "action", "reward"):
                assert _same(rst[k][b], out[k][b]), (b, k)
    assert _same(rst["p"], out["p"])


# ------------------------------------------------------------------ e. the split batch
@pytest.mark.parametrize("case", list(kc.SPLIT))
def test_split_batch_matches_the_oracle_and_the_unsplit_path(pkg, case):
    """k2_integrate with np >= 2 (fp32): the parts' offsets into `done`, the fields and the forcing, on a grid with a ragged tile.
    One fused step and one do_step: the first, a middle and the last trajectory of each part against the oracle, everything bit
    for bit against the same environment with part_streams=[] (the unsplit path); then the blow-up patch on the last trajectory
    of part 0, the first of part 1 and the last of the batch: `done` and do_step's flags are raised on exactly those three"""
    from oracle import keller_segel2d as k2
    c, dt, tol, prec = kc.CASES[case], torch.float32, _tol("f32"), "f32"
    setup, cfg = kc.build(pkg, k2, case)
    assert c.substeps == 3
    y0, act, prev = kc.inputs(case, steps=1)
    y0, a, prev = _cast(y0, prec), _cast(act[0], prec), _cast(prev, prec)
    B, A = c.B, cfg.A
    patched = kc.split_patched(case)
    bad = y0.copy()
    for b in patched:
        kc.patch(bad, b)
    runs = {}
    for name, fields in (("tame", y0), ("bad", bad)):
        for split in (True, False):
            env = pkg.PDEenv(setup, B=B, dtype=dt, y0=_mem(fields), action0=_act_shape(prev, B, A), autoreset=False,
                             **({} if split else dict(part_streams=[])))
            assert env.n_part_streams == (kc.SPLIT[case] if split else 0)
            term = torch.full((B, A), 7.0, dtype=dt, device="cuda:0")
            env.set_terminal_out(term)
            st_in = env.state.clone()
            y_pc, flags = env.do_step(env.y, env.prepare_action(_act(env, a, dt)))
            env(_act(env, a, dt))
            torch.cuda.synchronize()
            runs[name, split] = dict(y=env.y.clone(), p=env.p.clone(), state=env.state.clone(), reward=env.reward.clone(),
                                     done=env.done.clone(), term=term, st_in=st_in, y_pc=y_pc, flags=flags.clone())
            env.close()
        s, u = runs[name, True], runs[name, False]
        for k in ("y", "p", "state", "reward", "done", "term", "y_pc", "flags"):
            assert _same(s[k], u[k]), (name, k)
    tame, worst, ok = runs["tame", True], {}, True
    assert int(tame["done"].sum()) == 0 and int(tame["flags"].abs().sum()) == 0 and float(tame["term"].abs().max()) == 0.0
    for b in kc.picks(case):
        p_ref, y_ref, r_ref, st_ref = _oracle_step(k2, cfg, y0[b], a[b], prev[b], _np(tame["st_in"][b]).T)
        assert np.isfinite(y_ref).all()
        ok &= _abs(worst, "p", _np(tame["p"][b]), p_ref, tol["p"])
        ok &= _rel(worst, "y", _host(tame["y"][b]), y_ref, tol["rel"])
        ok &= _rel(worst, "do_step", _host(tame["y_pc"][b]), k2.do_step(cfg, y0[b], _np(tame["p"][b])), tol["rel"])
        ok &= _rel(worst, "reward", _np(tame["reward"][b]), r_ref, tol["rel"])
        ok &= _rel(worst, "state", _np(tame["state"][b]).T, st_ref, tol["rel"])
    print(f"[kseg2d-geometry split {case}] worst (bound {tol}):", worst)
    assert ok, worst
    b_ = runs["bad", True]
    assert torch.nonzero(b_["done"]).flatten().tolist() == patched
    assert torch.nonzero(b_["flags"]).flatten().tolist() == patched
    assert torch.nonzero(b_["term"][:, 0]).flatten().tolist() == patched and bool((b_["term"] == b_["term"][:, :1]).all())
    for b in patched:
        with np.errstate(all="ignore"):
            y_ref = k2.do_step(cfg, bad[b], k2.prepare_action(cfg, a[b]))
        assert np.isfinite(y_ref).all() and kc.blown(y_ref, c.max_value)
        ok &= _rel(worst, "y_patched", _host(b_["y"][b]), y_ref, tol["rel"])
    assert ok, worst
    keep = [b for b in range(B) if b not in patched]
    assert _same(b_["y"][keep], tame["y"][keep]) and _same(b_["reward"][keep], tame["reward"][keep])


# ------------------------------------------------------------------ f. the fp32 gather kernels
def test_fp32_gather_kernels_match_the_oracle(pkg, tmp_path):
    """kseg2d_rk4_kernel<float, 1, 2> and <float, 2, 2> (the forcing taken from the action table) run only under
    PDEC_KSEG2D_GATHER=1, which the library reads once per process: one fresh child process (kseg2d_gather_child.py) runs the
    fused step of kc.GATHER in fp32 as the rows stand and with the two-sub-step variant at K = 5, and writes its deviations
    from the oracle; no retry, a non-zero exit fails the test"""
    out = tmp_path / "gather.json"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kseg2d_gather_child.py")
    env = {k: v for k, v in os.environ.items() if k not in ("PDEC_KSEG2D_NSUB2", "PDEC_KSEG2D_SPLIT")}
    env["PDEC_KSEG2D_GATHER"] = "1"
    r = subprocess.run([sys.executable, child, str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    res = json.loads(out.read_text())
    tol = _tol("f32")
    assert res["gather_env"] == "1" and sorted(res["runs"]) == sorted(f"{c} {v}" for c in kc.GATHER for v in ("nsub1 K=3", "nsub2 K=5"))
    print("[kseg2d-geometry gather] worst per run:", res["runs"])
    for name, w in res["runs"].items():
        assert w["done"] == 0 and w["finite"], (name, w)
        assert w["p"] <= tol["p"] and w["y"] <= tol["rel"] and w["reward"] <= tol["rel"] and w["state"] <= tol["rel"], (name, w)
