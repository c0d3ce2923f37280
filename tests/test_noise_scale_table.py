"""The table of test_gpu_noise_scale.py (noise_scale_cases.py) held without a GPU and without the library: every row reaches the
kernel it names under the routing rules of DESIGN.md section 3.2 as the table restates them, the rows cover what the per-trajectory
exploration amplitude can get wrong, no element of any row can reach the clamp, and the Python layer has the setters and the binding
with their host-side checks."""
import math

import numpy as np
import pytest

import noise_scale_cases as nc


@pytest.mark.parametrize("name", sorted(nc.ROWS))
def test_row_reaches_its_kernel(name):
    r = nc.ROWS[name]
    assert nc.route(r) == r.kernel, f"{name}: the routing rules send it to {nc.route(r)}, the table names {r.kernel}"
    assert nc.entries(r) * r.cpe == nc.cols(r)


def test_the_table_covers_the_seams():
    R = nc.ROWS
    kernels = {r.kernel for r in R.values()}
    assert {"policy_act_fused_kernel<2>", "policy_act_fused_kernel<1>", "policy_act2_kernel<2,2>", "policy_act2_kernel<1,5>",
            "small_act_kernel", "generic"} == kernels
    # fused 3-layer: two full 64-column blocks and a ragged one, entries that straddle 16-column tiles and block edges
    r = R["fused3_mta2"]
    assert nc.cols(r) == 135 and nc.cols(r) // 64 == 2 and nc.cols(r) % 64 not in (0,) and 16 % r.cpe != 0 and 64 % r.cpe != 0
    # fused 2-layer: past the 256-state threshold, entries straddling tiles
    for n in ("fused2_kb2", "fused2_kb5"):
        assert nc.cols(R[n]) == 259 >= 256 and 16 % R[n].cpe != 0
    # one step outside the fused predicate
    assert R["generic_f32"].dims[1] == nc.FUSED3_ACT_MAX_H + 1 and {R["generic_f32"].net_dtype, R["generic_f64"].net_dtype} == {"f32", "f64"}
    # the few-column kernel: the reference's mixed types, fp32, and two outputs with one noise row
    assert (R["small_f64_f32"].state_dtype, R["small_f64_f32"].net_dtype, R["small_f64_f32"].B) == ("f64", "f32", 1)
    assert R["small_memory"].dims[-1] == 2 and R["small_memory"].noise_rows == 1
    # cols_per_entry: A everywhere but one row with 1 and one with 2 A
    other = {n: r.cpe for n, r in R.items() if r.cpe != r.A}
    assert other == {"fused3_cpe1": 1, "fused3_cpe2A": 2 * R["fused3_cpe2A"].A}
    assert nc.GLUE_ROW in R and R[nc.GLUE_ROW].B == 1 and nc.CLAMP_ROW in R
    # the rollouts: an odd batch (a lone last trajectory) on KS
    assert nc.KS_ROLL[1] % 2 == 1 and nc.KS_ROLL[1] >= 3
    # amplitudes: three distinct levels, one of them 0, none above 2; neighbouring entries differ
    for lv in (nc.LEVELS, nc.ROLL_LEVELS):
        assert len(set(lv)) == 3 and 0.0 in lv and max(lv) <= 2.0 and min(lv) >= 0.0
    m = nc.mixed(7)
    assert all(m[i] != m[i + 1] for i in range(6)) and 0.0 < nc.EQUAL <= 2.0 and 0.0 < nc.ROLL_EQUAL <= 2.0


def test_no_element_can_reach_the_clamp():
    """u = (w + 0.5) 2^-32 >= 2^-33, so the Box-Muller radius is at most sqrt(2 * 33 ln 2) < 6.8; the outputs are tanh-bounded"""
    assert abs(nc.max_normal() - math.sqrt(-2.0 * math.log(0.5 / 4294967296.0))) < 1e-14 and nc.max_normal() < 6.8
    for r in nc.ROWS.values():
        assert r.acts[-1] == nc.TANH
    worst = nc.no_clamp_bound(nc.LEVELS + (nc.EQUAL,) + nc.ROLL_LEVELS + (nc.ROLL_EQUAL,))
    assert worst < 14.6 < nc.ACT_LIMIT
    # and the host restatement of the stream stays under that radius
    from oracle import rng
    assert np.abs(rng.randn(nc.SEED, nc.OFFSET, 4096)).max() < nc.max_normal()


def test_draw_tolerance_is_the_stated_one():
    g, s, z = np.array([0.5]), 2.0, np.array([-3.0])
    assert nc.draw_tolerance(g, s, z, "f32")[0] == 3 * 2.0 ** -24 * 6.5 + 2e-12
    assert nc.draw_tolerance(g, s, z, "f64")[0] == 3 * 2.0 ** -53 * 6.5 + 2e-12
    assert nc.draw_tolerance(g, 0.0, z, "f64")[0] == 3 * 2.0 ** -53 * 0.5


def test_python_layer_has_the_setters_and_checks_host_input(pkg):
    """no library, no GPU: the binding's signature, the three setters, and the refusals of host arrays (raised before anything
    touches the device)"""
    import ctypes as C
    sig = pkg._lib.SIGNATURES["pdec_mlp_set_noise_scale"]
    assert len(sig) == 4 and sig[2] is C.c_int64 and sig[3] is C.c_int
    assert callable(pkg.CustomDDPGPolicy.set_noise_scale) and callable(pkg.TrainPipeline.set_noise_scale)
    assert callable(pkg.HipMLP.set_noise_scale)
    import inspect
    assert "noise_scale" in inspect.signature(pkg.TrainPipeline.__init__).parameters
    assert "noise_scale" in inspect.signature(pkg.PDEenv.rollout).parameters
    assert inspect.signature(pkg.CustomDDPGPolicy.set_noise_scale).parameters["cols_per_entry"].default is None
    from importlib import import_module
    buf = import_module(pkg.__name__ + ".agent").noise_scale_buffer
    with pytest.raises(ValueError, match=r"entry 1 is -0\.5 \(1 of 3"):
        buf([0.1, -0.5, 0.2], 3, "cpu", "who")
    with pytest.raises(ValueError, match=r"entry 2 is nan"):
        buf(np.array([0.1, 0.5, np.nan]), 3, "cpu", "who")
    with pytest.raises(ValueError, match=r"entry 0 is inf"):
        buf([np.inf, 0.5, 0.0], None, "cpu", "who")
    with pytest.raises(ValueError, match=r"who: expected 3 amplitudes in a 1-D array, got shape \(4,\)"):
        buf(np.zeros(4), 3, "cpu", "who")
    with pytest.raises(ValueError, match=r"expected 3 amplitudes in a 1-D array, got shape \(3, 1\)"):
        buf(np.zeros((3, 1)), 3, "cpu", "who")
    with pytest.raises(ValueError, match=r"expected >= 1 amplitudes"):
        buf(np.zeros(0), None, "cpu", "who")
    ok = buf([0.0, 0.5, 2.0], 3, "cpu", "who")
    assert ok.dtype.is_floating_point and ok.element_size() == 8 and ok.tolist() == [0.0, 0.5, 2.0]
