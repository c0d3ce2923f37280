"""The table of test_gpu_ks_disturbance.py (ks_disturbance_cases.py) held against oracle/ks.py, without a GPU: the inputs stay tame
under every amplitude of the table, and the mistakes the per-trajectory disturbance invites -- the two amplitudes of a packed pair
swapped (a neighbour's amplitude where a work-group holds one trajectory), the batch's mean amplitude for everyone -- move ONE
control step of the oracle by a stated multiple of the GPU test's fp32 bound, so that test cannot pass on them."""
import numpy as np
import pytest

import ks_disturbance_cases as dc
import ks_geometry_cases as kc
from oracle import ks


@pytest.fixture(scope="module")
def built(pkg):
    out = {}
    for case in dc.TABLE_ROWS:
        mu = dc.amplitudes(case)
        setup, cfgs = dc.configs(pkg, ks, case, list(mu) + [mu.mean()])
        out[case] = (setup, cfgs[:-1], cfgs[-1])         # (the row's setup, one config per trajectory, the one at the batch's mean)
    return out


def _step(case, cfg, y, a):
    return kc.oracle_step(ks, cfg, case, y, ks.prepare_action(cfg, a[None]))


def test_the_table_is_what_the_gpu_test_needs():
    assert set(dc.STEP_ROWS) <= set(kc.CASES) and not any(kc.CASES[c].mono for c in dc.TABLE_ROWS)
    kinds = {kc.CASES[c].integrator for c in dc.STEP_ROWS}
    assert kinds == {"cnab2", "rk4_fd", "midpoint_fd"}
    assert {kc.engine(kc.CASES[c].nx) for c in dc.STEP_ROWS if kc.CASES[c].integrator == "cnab2"} == \
        {"FftWave256", "FftFixed192", "FftGeneric", "FftWave1024"}
    assert kc.n_actuators("perm_oddA_256") % 2 == 1
    fd = [c for c in dc.STEP_ROWS if kc.CASES[c].integrator != "cnab2"]
    assert {kc.nthreads(kc.CASES[c].nx, kc.CASES[c].integrator) == 64 for c in fd} == {True, False}     # the one-wave kernel and the general one
    for case in dc.STEP_ROWS:
        mu, B = dc.amplitudes(case), dc.batch(case)
        assert B % 2 == 1 and B == (3 if kc.CASES[case].nx == 1024 else 5)       # the last trajectory is alone in its work-group
        assert all(abs(mu[a] - mu[b]) >= 0.1 - 1e-15 for a, b in dc.pairs(case)) and len(dc.pairs(case)) == B // 2
        assert abs(mu[B - 1] - mu.mean()) >= 0.05 - 1e-15 and len(set(mu.tolist())) == B
    assert 0.0 in dc.MU and min(dc.MU) < 0 < max(dc.MU)
    assert 0 < dc.ROLL_FROM < dc.ROLL_T <= 8 and dc.STEPS <= 8


@pytest.mark.parametrize("case", dc.TABLE_ROWS)
def test_inputs_stay_tame_under_every_amplitude(built, case):
    """free-running in the oracle for the longest run of the GPU test (ROLL_T steps: the step tests' STEPS actions, then zero
    actions, as the uncontrolled prefix of the rollouts has them), every trajectory at its own amplitude"""
    setup, cfgs, _ = built[case]
    B = dc.batch(case)
    y0, act, prev = kc.inputs(case, B, steps=dc.STEPS)
    for b in range(B):
        y = y0[b]
        for t in range(dc.ROLL_T):
            a = act[t, b] if t < dc.STEPS else np.zeros_like(prev[b])
            y = _step(case, cfgs[b], y, a)
            assert np.isfinite(y).all() and np.abs(y).max() < 6.0, (b, t, float(np.abs(y).max()))
        assert np.abs(y).max() < 0.5 * kc.CASES[case].max_value


@pytest.mark.parametrize("case", dc.TABLE_ROWS)
def test_a_mistaken_amplitude_moves_one_step_by_many_bounds(built, case):
    setup, cfgs, mean_cfg = built[case]
    c = kc.CASES[case]
    B, mu = dc.batch(case), dc.amplitudes(case)
    need = dc.MIN_BOUNDS[c.integrator]
    y0, act, prev = kc.inputs(case, B, steps=1)
    ref = [_step(case, cfgs[b], y0[b], act[0, b]) for b in range(B)]
    bound = [kc.tol_y("f32", case, r) for r in ref]
    worst = {}
    # the two amplitudes of a pair swapped
    for a, b in dc.pairs(case):
        for me, other in ((a, b), (b, a)):
            moved = float(np.abs(_step(case, cfgs[other], y0[me], act[0, me]) - ref[me]).max())
            worst["swap"] = min(worst.get("swap", np.inf), moved / bound[me])
            assert moved >= need * bound[me], (me, other, moved, bound[me])
            assert moved >= 1e6 * kc.tol_y("f64", case, ref[me])
    # the batch's mean amplitude for everyone: every trajectory whose own amplitude is not the mean moves, in proportion
    most = 0.0
    for b in range(B):
        moved = float(np.abs(_step(case, mean_cfg, y0[b], act[0, b]) - ref[b]).max())
        off = abs(mu[b] - mu.mean())
        most = max(most, moved / bound[b])
        if off < 1e-12:             # (trajectory 0 carries the mean itself)
            assert moved < 1e-12
            continue
        worst["mean"] = min(worst.get("mean", np.inf), moved / bound[b] / (off / 0.1))
        assert moved >= need * bound[b] * (off / 0.1), (b, moved, bound[b], off)
    assert most >= need, most
    # the lone last trajectory with its neighbour's amplitude (the empty half of its pair must not bring one in)
    moved = float(np.abs(_step(case, cfgs[B - 2], y0[B - 1], act[0, B - 1]) - ref[B - 1]).max())
    assert moved >= need * bound[B - 1], (moved, bound[B - 1])
    print(f"[ks-disturbance table {case}] movement in fp32 bounds per 0.1 of amplitude, least:", worst,
          "max |y|", float(max(np.abs(r).max() for r in ref)))
