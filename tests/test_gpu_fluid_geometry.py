"""The 2-D fluid kernels (csrc/fluid_lds.hip, fluid_wave.hip, fluid_sense.hip) against oracle/fluid.py over the geometries of fluid_geometry_cases.py, in fp64 and fp32:
the LDS-tile kernels with 8, 4 and 2 lines per tile (radix-5 stages among them, and the fall-through of a grid that asks for the
fused integrator and has no wave plan), the fused integrator on un-padded grids (self-mirrored Nyquist line), with K = 1 and
K = 3 and with several x-pass tiles per workgroup, do_step on the half-wave plans and with the persistent x-pass at n = 512,
sensing and actuation with other windows, ragged 16 x 16 blocks, a window wider than the sensor grid and a box as long as the
ring, and the three documented switches, each value in a process of its own (fluid_geometry_child.py).
test_fluid_geometry_table.py proves without a GPU that each row reaches what it is there for; here every environment's dispatch
is first held to the table's restatement through the library's own pdec_debug_fluid_plan.

Tolerances are the project's own (fluid_geometry_cases.TOL), relative to max |reference| (state and reward: to max(1, |ref|)).
fp64: rhs and do_step 1e-11, closures 1e-12, env step 1e-11.  fp32: rhs 2e-6, do_step 5e-6, env step / state / reward 1e-5, forcing
1e-6.  Inputs are exact in single precision, the oracle runs in fp64 from those values; a control step after the first is
compared from the device's own previous field.  Measured errors per row: DESIGN.md 3.3."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fluid_geometry_cases as fc
import fluid_geometry_child as dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fluid_geometry_child.py")


def _rows(what):
    return [(case, prec) for case, c in fc.CASES.items() if what in c.run for prec in fc.PRECS]


def _rel(a, ref, floor=0.0):
    return float(np.abs(a - ref).max()) / max(floor, float(np.abs(ref).max()))


def _env(pkg, case, prec, **kw):
    """the row's environment, its dispatch held to the table first"""
    from oracle import fluid
    assert not [k for k in fc.ENV_NAMES if k in os.environ], "the in-process rows need the fluid switches unset"
    c = fc.CASES[case]
    r = fc.reference(pkg, fluid, case)
    env = pkg.PDEenv(r["setup"], B=c.B, dtype=dev.torch_dtype(torch, prec), autoreset=False, **kw)
    got, want = dev.device_plan(pkg, env), fc.plan(case, prec)
    assert got == want, (case, prec, dict(zip(fc.PLAN_FIELDS, got)), dict(zip(fc.PLAN_FIELDS, want)))
    return c, r, env


def _report(tag, case, prec, worst, tol):
    print(f"[fluid-geometry {tag} {case} {prec}] " + ", ".join(f"{k} {v:.2e} (<= {tol[k]:.0e})" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= tol[k]}
    assert not bad, ("numeric", case, prec, bad)


# ------------------------------------------------------------------ a. the right-hand side
@pytest.mark.parametrize("case,prec", _rows("rhs"))
def test_rhs_matches_the_oracle(pkg, case, prec):
    c, r, env = _env(pkg, case, prec)
    out, untouched = dev.device_rhs(torch, env, r["y"], r["p"], env.dtype)
    assert untouched and np.isfinite(out).all()
    _report("rhs", case, prec, dict(rhs=max(_rel(out[b], r["rhs"][b]) for b in range(c.B))), fc.TOL[prec])
    env.close()


# ------------------------------------------------------------------ b. do_step
@pytest.mark.parametrize("case,prec", _rows("step"))
def test_do_step_matches_the_oracle(pkg, case, prec):
    """K RK4 sub-steps (FluidSetup.jl:163-172) by the integrator the row reaches: the plain loop over the LDS-tile or the wave
    kernels, or fluid_integrate_wave; input untouched, flags zero"""
    c, r, env = _env(pkg, case, prec)
    out, flags, untouched = dev.device_step(torch, env, r["y"], r["p"], env.dtype)
    assert untouched and flags == [0] * c.B and np.isfinite(out).all()
    _report("do_step", case, prec, dict(step=max(_rel(out[b], r["step"][b]) for b in range(c.B))), fc.TOL[prec])
    env.close()


# ------------------------------------------------------------------ c. closures and the fused env step
@pytest.mark.parametrize("case,prec", _rows("env"))
def test_closures_and_env_step_match_the_oracle(pkg, case, prec):
    """featurize at reset, prepare_action, then tsteps fused (env)(action) (src/PDEenv.jl:195-241): y, p, reward, state, the done
    flags and the stand-alone reward_function"""
    from oracle import fluid
    c = fc.CASES[case]
    A = c.spa ** 2
    r = fc.reference(pkg, fluid, case)
    c, r, env = _env(pkg, case, prec, y0=r["y"], action0=np.ascontiguousarray(r["a_prev"].reshape(c.B, A, 1)))
    cfg, dt, tol = r["cfg"], env.dtype, fc.TOL[prec]
    np64 = lambda t: t.detach().cpu().numpy().astype(np.float64)
    act = lambda a: dev.to_dev(torch, a.reshape(c.B, A, 1), dt)
    worst = dict(closure=0.0, forcing=0.0, env=0.0)
    for b in range(c.B):
        worst["closure"] = max(worst["closure"], _rel(np64(env.state[b]).T, r["feat0"][b], 1.0))
    pa = dev.jul(env.prepare_action(act(r["acts"][0])))
    for b in range(c.B):
        worst["forcing"] = max(worst["forcing"], _rel(pa[b], r["steps"][0]["pa"][b]))
    y_prev, st_prev, a_prev = r["y"], None, r["a_prev"]
    for t in range(c.tsteps):
        a = r["acts"][t]
        env(act(a))
        y_dev, p_dev, rew, st = dev.jul(env.y), dev.jul(env.p), np64(env.reward), np64(env.state)
        assert np.isfinite(y_dev).all() and np.isfinite(rew).all() and np.isfinite(st).all()
        done = env._done_flags.cpu().tolist()
        alone = np64(env.reward_function())
        for b in range(c.B):
            if t == 0:
                s = {k: v[b] for k, v in r["steps"][0].items()}
            else:               # from the device's own previous field and state
                p_ref = fluid.prepare_action(cfg, a[b])
                y_ref = fluid.do_step(cfg, y_prev[b], p_ref, c.K)
                s = dict(pa=p_ref, y=y_ref, reward=fluid.reward_function(cfg, y_ref, a[b], a[b] - a_prev[b]),
                         state=fluid.featurize(cfg, y_ref, st_prev[b].T))
            worst["forcing"] = max(worst["forcing"], _rel(p_dev[b], s["pa"]))
            worst["env"] = max(worst["env"], _rel(y_dev[b], s["y"]), _rel(rew[b], s["reward"], 1.0), _rel(st[b].T, s["state"], 1.0))
            assert st[b].T.shape == s["state"].shape == (fc.geometry(case, prec)["ns"], A)
            assert not done[b] and not (np.abs(s["reward"]) > r["setup"].max_value).any()      # check_max_value = "reward"
        assert np.abs(alone - rew).max() <= (1e-14 if prec == "f64" else 1e-6) * max(1.0, np.abs(rew).max())
        y_prev, st_prev, a_prev = y_dev, st, a
    _report("env", case, prec, worst, tol)
    env.close()


# ------------------------------------------------------------------ d. the documented switches, one process per value
@pytest.mark.parametrize("var,value", fc.SWITCHES)
def test_switch_rows_match_the_oracle(pkg, tmp_path, var, value):
    """PDEC_FLUID_K2P=0: fluid_k2w_kernel<T,2,3,4,6> and <T,4,3,4,6>; PDEC_FLUID_FUSE=1: fluid_k31w_kernel<T,4,3,6> and <T,4,2,6>;
    PDEC_FLUID_FUSE=0: the plain loop at n = 256; PDEC_FLUID_LDS_FFT=1: the LDS-tile kernels at the wave lengths (TL 16, 8, 4).
    The child's plan, rhs and do_step against the table and the oracle; under PDEC_FLUID_K2P=0 the right-hand side also equals
    this process's (fluid_k2p_kernel) bit for bit wherever csrc/fluid_wave.hip states that of W2 (fluid_geometry_cases.K2P_VS_K2W)."""
    from oracle import fluid
    rows = fc.switch_rows(var, value)
    assert rows
    refs = {row: fc.reference(pkg, fluid, row) for row in rows}
    for row in rows:
        np.save(tmp_path / f"{row}_y.npy", refs[row]["y"])
        np.save(tmp_path / f"{row}_p.npy", refs[row]["p"])
    env = {k: v for k, v in os.environ.items() if k not in fc.ENV_NAMES}
    env[var] = value
    # a 512 x 512 setup, four environments and a dozen launches: seconds; the limit covers a cold start of the runtime
    proc = subprocess.run([sys.executable, CHILD, str(tmp_path)], env=env, timeout=240, capture_output=True, text=True)
    assert proc.returncode == 0, (proc.returncode, proc.stdout[-2000:], proc.stderr[-4000:])
    with open(tmp_path / "meta.json") as fh:
        meta = json.load(fh)
    assert meta["env"] == {var: value}
    for row in rows:
        c, r = fc.SWITCH_CASES[row], refs[row]
        for prec in fc.PRECS:
            m = meta["rows"][f"{row} {prec}"]
            want = fc.plan(row, prec)
            assert m["plan"] == want, (row, prec, dict(zip(fc.PLAN_FIELDS, m["plan"])), dict(zip(fc.PLAN_FIELDS, want)))
            worst = {}
            if "rhs" in c.run:
                out = np.load(tmp_path / f"{row}_{prec}_rhs.npy")
                assert m["rhs_input_untouched"] and np.isfinite(out).all()
                worst["rhs"] = max(_rel(out[b], r["rhs"][b]) for b in range(c.B))
                if (row, prec) in fc.K2P_VS_K2W:
                    dt = dev.torch_dtype(torch, prec)
                    here = pkg.PDEenv(r["setup"], B=c.B, dtype=dt, autoreset=False)
                    plan = dict(zip(fc.PLAN_FIELDS, dev.device_plan(pkg, here)))
                    assert plan["k2p"] == 1 and fc.geometry(row, prec, env={})["k2p"] == 1
                    mine, _ = dev.device_rhs(torch, here, r["y"], r["p"], dt)
                    here.close()
                    diff = float(np.abs(mine - out).max()) / float(np.abs(out).max())
                    print(f"[fluid-geometry switch {row} {prec}] K2p against K2w: max difference {diff:.2e} of max |rhs|")
                    assert diff <= fc.K2P_VS_K2W[row, prec], ("numeric", row, prec, diff)
                    if fc.K2P_VS_K2W[row, prec] == 0.0:
                        assert np.array_equal(mine, out), ("numeric", row, prec)
            if "step" in c.run:
                out = np.load(tmp_path / f"{row}_{prec}_step.npy")
                assert m["step_input_untouched"] and m["flags"] == [0] * c.B and np.isfinite(out).all()
                worst["step"] = max(_rel(out[b], r["step"][b]) for b in range(c.B))
            _report(f"switch {var}={value}", row, prec, worst, fc.TOL[prec])
