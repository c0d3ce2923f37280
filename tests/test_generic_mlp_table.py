"""The case table of test_gpu_generic_mlp.py (generic_mlp_cases.py) against what it claims, with the tile constants read out of
csrc/mlp.hip and the fp64 oracle (oracle/nn.py) as the only arithmetic.  Runs without a GPU: the edges are all there, every row's
data is usable (few ReLU kinks, no all-zero gradient array, every fp32 DDPG row outside the fused predicates) and the tolerances
of the GPU test are sound -- the same reference evaluated in numpy float32 stays ten times inside them."""
import sys

import numpy as np
import pytest

import fused_shape_cases as fc
import generic_mlp_cases as gc
from oracle import nn

NET_RUNS = [(name, cols) for name, (_, _, cc) in gc.NETS.items() for cols in cc]
DDPG_RUNS = [(name, quirk) for name in gc.DDPG for quirk in gc.QUIRKS]


def relerr(a, b):
    return np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max() / max(1e-30, np.abs(b).max())


def test_constants_are_the_ones_the_table_was_written_for():
    assert gc.read_constants() == (64, 64, 16, 512)
    assert (gc.I, gc.R, gc.T) == (nn.IDENT, nn.RELU, nn.TANH)


def test_table_imports_without_torch_or_numpy():
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); import generic_mlp_cases as gc; "
            "assert 'torch' not in sys.modules and 'numpy' not in sys.modules; print(len(gc.NETS), len(gc.DDPG))") % gc.os.path.dirname(gc.__file__)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == [str(len(gc.NETS)), str(len(gc.DDPG))]


def test_rows_are_well_formed():
    for name, (dims, acts, cols) in gc.NETS.items():
        assert len(dims) == len(acts) + 1 and 1 <= len(acts) <= 8 and min(dims) >= 1 and min(cols) >= 1, name
        assert set(acts) <= {gc.I, gc.R, gc.T}
        assert max(cols) == cols[0], name                  # the handle is made for the first count
    for name, (da, aa, dc, ac, prec, Bu) in gc.DDPG.items():
        assert len(da) == len(aa) + 1 and len(dc) == len(ac) + 1 and prec in ("f32", "f64") and Bu >= 1, name
        assert dc[0] == da[0] + da[-1] and dc[-1] == 1 and name.startswith(prec), name
    assert len(gc.NETS) == 13 and len(gc.DDPG) == 6 and len(gc.F64_DDPG) == 3


def test_tile_and_split_edges_are_all_there():
    gm, gn, gk, kc = gc.read_constants()
    widths = {1, gk - 1, gk, gk + 1, gm - 1, gm, gm + 1, 2 * gm, 2 * gm + 1}
    assert widths == {1, 15, 16, 17, 63, 64, 65, 128, 129}
    ins = {d for dims, _, _ in gc.NETS.values() for d in dims[:-1]}
    outs = {d for dims, _, _ in gc.NETS.values() for d in dims[1:]}
    assert widths <= ins and widths <= outs
    cols = {c for _, _, cc in gc.NETS.values() for c in cc}
    assert {1, gk - 1, gk, gk + 1, gn - 1, gn, gn + 1, kc - 1, kc, kc + 1, 2 * kc, 2 * kc + 1} <= cols
    assert {1, 15, 16, 17, 63, 64, 65, 511, 512, 513, 1024, 1025} <= cols
    hidden = {a for _, acts, _ in gc.NETS.values() for a in acts[:-1]}
    last = {acts[-1] for _, acts, _ in gc.NETS.values()}
    assert hidden == last == {gc.I, gc.R, gc.T}
    assert {1, 2, 3, 5, 8} <= {len(acts) for _, acts, _ in gc.NETS.values()}
    assert any(d == 1 for dims, _, _ in gc.NETS.values() for d in dims[1:-1])           # a width-1 layer in the middle
    assert any(len(cc) > 1 and cc[1] < cc[0] for _, _, cc in gc.NETS.values())          # a smaller count behind a larger one
    # the DDPG rows: a last dW chunk of ONE column, an exact multiple of the chunk, one block's stride 256 from both sides
    bus = {v[5] for v in gc.DDPG.values()}
    assert {1, 255, 257, kc, kc + 1, 2 * kc + 1} <= bus
    assert any(v[0][-1] == 2 and v[5] % 2 == 1 for v in gc.DDPG.values())               # na = 2 at an odd batch


@pytest.mark.parametrize("name", [n for n, v in gc.DDPG.items() if v[4] == "f32"])
def test_f32_ddpg_rows_are_outside_both_fused_predicates(name):
    k = fc.read_constants()
    assert gc.outside_fused(name, k)
    da, aa = gc.DDPG[name][:2]
    assert da[-1] != 1 or len(aa) > 3                      # by the number of actions or of layers: no table row names them
    # the helper does say "inside" for the pairs the fused families serve
    gc.DDPG["_probe"] = ([3, 16, 16, 1], [gc.R, gc.R, gc.T], [4, 140, 140, 1], [gc.R, gc.R, gc.I], "f32", 200)
    try:
        assert not gc.outside_fused("_probe", k)
    finally:
        del gc.DDPG["_probe"]


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name,cols", NET_RUNS)
def test_network_rows_have_few_kinks_and_live_gradients(name, cols, prec):
    dims, acts, _ = gc.NETS[name]
    P = gc.net_params(name, prec)
    x, dy, replaced = gc.net_data(name, cols, prec, P)
    assert x.shape == (dims[0], cols) and dy.shape == (dims[-1], cols) and x.dtype == gc.np_dtype(prec)
    assert replaced < gc.KINK_CAP * cols, (name, cols, replaced)
    assert not gc.kinked_columns(P, acts, x).any()
    y, g, dx = gc.net_reference(P, acts, x, dy)
    assert all(np.abs(a).max() > 0 for a in g) and np.abs(dx).max() > 0 and np.abs(y).max() > 0


@pytest.mark.parametrize("name,quirk", DDPG_RUNS)
def test_ddpg_rows_have_few_kinks_and_live_gradients(name, quirk):
    da, aa, dc, ac, prec, Bu = gc.DDPG[name]
    case = gc.ddpg_case(name, quirk)
    assert case["replaced"] < gc.KINK_CAP * Bu, (name, quirk, case["replaced"])
    s, a = case["batch"][:2]
    assert not gc.ddpg_kinked_columns(case["P"][0], case["P"][1], aa, ac, s, a).any()
    out, out2 = gc.ddpg_reference(name, quirk, case)
    assert all(np.abs(g).max() > 0 for g in out["gC"]) and all(np.abs(g).max() > 0 for g in out2["gA"])
    assert all(x.dtype == gc.np_dtype(prec) for x in case["batch"])


@pytest.mark.parametrize("name,quirk", [(n, q) for n in gc.F64_DDPG for q in gc.QUIRKS])
def test_few_entries_sit_where_adam_is_ill_conditioned(name, quirk):
    """the parameter comparison behind pdec_ddpg_update may leave out entries with an almost-zero gradient: at most 0.1 % of an
    array -- counted here on the reference alone, so the cap is known to hold before anything runs on a GPU"""
    _, _, masks = gc.ddpg_reference_updates(name, quirk)
    for net in masks:
        for m in net:
            assert int(m.sum()) <= int(gc.SMALL_GRAD_CAP * m.size), (name, quirk, m.shape, int(m.sum()))


def test_fp32_tolerances_are_sound():
    """the fp64 reference against ITSELF evaluated in numpy float32 on the same rounded values: an honest fp32 evaluation stays at
    least ten times inside the tolerances the GPU test applies"""
    worst = {"forward": 0.0, "dx": 0.0, "grad": 0.0}
    for name, cols in NET_RUNS:
        _, acts, _ = gc.NETS[name]
        P = gc.net_params(name, "f32")
        x, dy, _ = gc.net_data(name, cols, "f32", P)
        y, g, dx = gc.net_reference(P, acts, x, dy)
        y32, zs, as_ = nn.forward(P, acts, x, keep=True)
        g32, dx32 = nn.backward(P, acts, zs, as_, dy)
        assert y32.dtype == np.float32 and dx32.dtype == np.float32
        worst["forward"] = max(worst["forward"], relerr(y32, y))
        worst["dx"] = max(worst["dx"], relerr(dx32, dx))
        worst["grad"] = max([worst["grad"]] + [relerr(a, b) for a, b in zip(g32, g)])
    for name, quirk in DDPG_RUNS:
        da, aa, dc, ac, prec, Bu = gc.DDPG[name]
        if prec != "f32":
            continue
        case = gc.ddpg_case(name, quirk)
        out, out2 = gc.ddpg_reference(name, quirk, case)
        PA, PC, PAt, PCt = case["P"]
        s, a, r, t, sn = case["batch"]
        o32 = nn.ddpg_losses_and_grads(PA, PC, PAt, PCt, aa, ac, s, a, r, t, sn, np.float32(gc.GAMMA), bool(quirk))
        o32b = nn.actor_grads(PA, PC, aa, ac, s)
        worst["grad"] = max([worst["grad"]] + [relerr(x, y) for x, y in zip(o32["gC"] + o32b["gA"], out["gC"] + out2["gA"])])
    print("float32 evaluation of the reference, worst relative error:", worst)
    assert worst["forward"] <= gc.TOL["f32"]["forward"] / 10
    assert worst["dx"] <= gc.TOL["f32"]["grad"] / 10
    assert worst["grad"] <= gc.TOL["f32"]["grad"] / 10
