"""The table of test_gpu_noise_color.py (noise_color_cases.py) held without a GPU and without the library: colour does not change
which kernel a row reaches, the {a, b} rows keep the stationary variance at 1, the fp64 model at a = 0 is the white draw exactly,
its variance over a long series is 1 at every correlation of the table, and the C ABI and the Python layer have the entry."""
import os
import re

import numpy as np
import pytest

import noise_color_cases as cc
import noise_scale_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(cc.ROWS))
def test_colour_does_not_change_the_route(name):
    r = cc.ROWS[name]
    assert cc.ROWS is nc.ROWS and cc.route(r) == r.kernel
    assert cc.entries(r) * r.cpe == cc.cols(r) and cc.counters(r) * 4 >= cc.cols(r) * r.dims[-1] > (cc.counters(r) - 1) * 4


def test_ab_rows_have_unit_stationary_variance(pkg):
    a = cc.corr(7)
    assert a.tolist() == [0.9, 0.0, 0.5, 0.9, 0.0, 0.5, 0.9] and all(a[i] != a[i + 1] for i in range(6))
    from importlib import import_module
    host = import_module(pkg.__name__ + ".agent").noise_corr_ab
    for ab in (cc.ab_of(a), host(a, 7, "who"), host(0.8, 3, "who")):
        assert ab.dtype == np.float64 and ab.shape[1] == 2 and ab.flags.c_contiguous
        assert (np.abs(ab[:, 0] ** 2 + ab[:, 1] ** 2 - 1.0) <= 2.0 ** -52).all()            # 1 ulp of 1
        assert ((ab[:, 0] >= 0) & (ab[:, 0] < 1) & (ab[:, 1] > 0) & (ab[:, 1] <= 1)).all()
    assert np.array_equal(cc.ab_of(a), host(a, None, "who")) and cc.ab_of([0.0])[0].tolist() == [0.0, 1.0]
    for bad, n, msg in (([0.5, 1.0], None, r"entry 1 is 1\.0 \(1 of 2"), ([-0.1], None, r"entry 0 is -0\.1"),
                        ([np.nan, 0.2], 2, "entry 0 is nan"), (1.5, 3, r"entry 0 is 1\.5"),
                        (np.zeros((2, 1)), None, r"got shape \(2, 1\)"), (np.zeros(4), 3, r"who: expected a scalar or 3 ")):
        with pytest.raises(ValueError, match=msg):
            host(bad, n, "who")
    assert pkg.corr_from_time(2.0, 0.5) == np.exp(-0.25) and pkg.corr_from_time(3.0, 0.0) == 1.0
    with pytest.raises(ValueError, match="tau > 0"):
        pkg.corr_from_time(0.0, 1.0)


def test_the_model_at_zero_correlation_is_the_white_draw():
    from oracle import rng
    z = np.stack([rng.randn(cc.SEED, cc.OFFSET + 3 * t, 12).reshape(6, 2) for t in range(cc.STEPS)])
    x0 = np.random.default_rng(0).uniform(-1, 1, (6, 2))
    xs = cc.model(x0, np.repeat(cc.ab_of([0.0]), 6, axis=0), z)
    assert np.array_equal(xs.view(np.uint64), z.view(np.uint64))
    # noise rows: the rows beyond them keep x0
    xs = cc.model(x0, np.repeat(cc.ab_of([0.5]), 6, axis=0), z, noise_rows=1)
    assert np.array_equal(xs[-1][:, 1], x0[:, 1]) and not np.array_equal(xs[-1][:, 0], x0[:, 0])


VAR_COLS = 64


@pytest.mark.parametrize("a", cc.CORR)
def test_stationary_variance_is_one(a):
    """4 000 steps of the host restatement of the stream, from x0 = 0: b = sqrt(1 - a^2) keeps act_noise and the scale array at
    their meaning at every correlation.  The mean of x^2 over N steps of ONE AR(1) series has the standard deviation
    sqrt(2 (1 + a^2) / ((1 - a^2) N)) = 0.069 at a = 0.9, N = 4000: more than the 5 % asked for.  So the model runs 64 columns
    side by side, as an acting call does (step t draws its 64 normals at counter OFFSET + 16 t), which brings the deviation to
    0.069 / 8 < 0.9 % and 5 % to more than five of them; 31 columns would give four."""
    from oracle import rng
    assert VAR_COLS >= (4 * np.sqrt(2 * 1.81 / (0.19 * 4000)) / 0.05) ** 2
    z = np.stack([rng.randn(cc.SEED, cc.OFFSET + (VAR_COLS // 4) * t, VAR_COLS) for t in range(0, 4000, 500)])
    whole = rng.randn(cc.SEED, cc.OFFSET, 4000 * VAR_COLS).reshape(4000, VAR_COLS, 1)
    assert np.array_equal(whole[::500, :, 0], z)                      # the per-step numbering of the acting calls
    xs = cc.model(np.zeros((VAR_COLS, 1)), np.repeat(cc.ab_of([a]), VAR_COLS, axis=0), whole)
    var = float(np.mean(xs * xs))
    print(f"[noise-color a = {a}] variance over 4000 steps x {VAR_COLS} columns: {var:.4f}")
    assert abs(var - 1.0) <= 0.05


def test_state_tolerance_is_the_stated_one():
    M = cc.max_normal()
    assert cc.state_tolerance(0, 0.9) == 0.0
    assert cc.state_tolerance(1, 0.0) == 1e-12 + 2 * cc.U * M
    b = np.sqrt(1 - 0.81)
    e1 = 1e-12 * b + 2 * cc.U * (0.9 + b) * M
    assert cc.state_tolerance(2, 0.9) == 0.9 * e1 + e1
    assert cc.action_tolerance(np.array([0.5]), 2.0, np.array([-3.0]), "f32", 1e-11)[0] == 3 * 2.0 ** -24 * 6.5 + 2e-12 + 2e-11


def test_the_entry_is_declared_and_bound(pkg):
    import ctypes as C
    import inspect
    with open(os.path.join(ROOT, "include", "pdeconv.h")) as f:
        header = f.read()
    assert re.search(r"int pdec_mlp_set_noise_color\(pdec_handle actor, double\* state_dev, const double\* ab_dev, int64_t n, "
                     r"int cols_per_entry\);", header)
    sig = pkg._lib.SIGNATURES["pdec_mlp_set_noise_color"]
    assert len(sig) == 5 and sig[3] is C.c_int64 and sig[4] is C.c_int
    assert callable(pkg.HipMLP.set_noise_color) and callable(pkg.CustomDDPGPolicy.set_noise_corr)
    assert callable(pkg.CustomDDPGPolicy.reset_noise_state) and callable(pkg.TrainPipeline.set_noise_corr)
    assert inspect.signature(pkg.TrainPipeline.__init__).parameters["noise_corr"].default is None
    assert inspect.signature(pkg.CustomDDPGPolicy.set_noise_corr).parameters["cols_per_entry"].default is None
