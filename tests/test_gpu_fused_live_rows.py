"""The fused 3-layer DDPG passes issue no MFMA on a k-step or a tile whose operands are zero by construction (csrc/fused3_layers.hpp,
LiveRows): the first layers run ceil(K0 / 4) of their four k-steps, and a last hidden tile that holds only the bias row of the
gradient image (H a multiple of 16) is zero without a product.  Every skipped instruction added exact zeros, so nothing may move:

  1. bitwise       two identical sets of handles run three batched updates and one fused acting call, one set with
                   PDEC_FUSED_FULL_ROWS=1 (every MFMA of the padded extents, the form before) and one without.  All four networks'
                   parameters, both ADAM moment sets, both flat gradient buffers, the losses and the actions are compared with
                   array_equal / torch.equal, which hold -0 == +0: the one difference a skipped add of zero can make.
  2. oracle        the rows this file adds go through the fp64-oracle gradient check of test_gpu_fused_shapes.py, its helper and its
                   tolerances.

Rows: every fused 3-layer row of fused_shape_cases.CASES up to 1000 columns, and the edges of the new counts (EXTRA below)."""
import ctypes as C

import numpy as np
import pytest

import fused_shape_cases as fc
from test_gpu_fused_shapes import Rig, _check_gradients
from test_gpu_grads import read_grads
from util import to_dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# (layers, ns, actor hidden, critic hidden, Bu, grad_scale, pair, act) as in fused_shape_cases.CASES
EXTRA = {
    "live_ns4_a16_c31_bu17": (3, 4, 16, 31, 17, 1.0, "<2,2>", "<2>"),        # critic K0 = 5: two live k-steps beside the actor's one
    "live_ns8_a15_c128_bu63": (3, 8, 15, 128, 63, 0.5, "<9,1>", "<1>"),      # actor two, critic three; the critic's ninth tile dead
    "live_ns12_a16_c16_bu15": (3, 12, 16, 16, 15, 1.0, "<2,2>", "<2>"),      # actor three, critic four; both second tiles dead
    "live_ns3_a17_c143_bu64": (3, 3, 17, 143, 64, 1.0, "<9,2>", "<2>"),      # the second actor tile has exactly one live row
    "live_ns3_a16_c140_bu129": (3, 3, 16, 140, 129, 1.0, "<9,2>", "<2>"),    # the flagship pair, two workgroups
}
SHARED = [k for k in fc.FUSED if fc.CASES[k][0] == 3 and fc.CASES[k][4] <= 1000]
ROWS = SHARED + list(EXTRA)


@pytest.fixture
def table(monkeypatch):
    """the rows of EXTRA sit in fused_shape_cases.CASES for the length of one test (Rig looks its row up there)"""
    for k, v in EXTRA.items():
        monkeypatch.setitem(fc.CASES, k, v)


def test_rows_are_the_ones_the_counts_need():
    assert len(SHARED) == 8
    rows = [fc.CASES[k] for k in SHARED] + list(EXTRA.values())
    kt = lambda K0: -(-K0 // 4)
    assert {(kt(r[1]), kt(r[1] + 1)) for r in rows} >= {(1, 1), (1, 2), (2, 2), (2, 3), (3, 4), (4, 4)}
    assert {r[2] for r in rows} >= {1, 15, 16, 17, 31} and {r[3] for r in rows} >= {16, 31, 128, 140, 143}
    k = fc.read_constants()
    for name, r in EXTRA.items():
        assert fc.rule(*r[:4], k) == r[6:], name


def _adam(net):
    n = net.num_params
    m, v, bp = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.float32), (C.c_double * 2)()
    assert net.lib.pdec_adam_get_state(net.handle, m.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), bp) == 0
    return m, v, np.array([bp[0], bp[1]])


def _snapshot(rig, i):
    """everything an update leaves behind on handle set i"""
    A, Cn, At, Ct = rig.nets(i)
    out = {f"{who} array {j}": p for who, net in (("actor", A), ("critic", Cn), ("target actor", At), ("target critic", Ct))
           for j, p in enumerate(net.params())}
    for who, net in (("actor", A), ("critic", Cn)):
        out[f"{who} ADAM m"], out[f"{who} ADAM v"], out[f"{who} beta powers"] = _adam(net)
        out[f"{who} gradient buffer"] = read_grads(rig.pkg, net)
    return out


@pytest.mark.parametrize("quirk", [1, 0])
@pytest.mark.parametrize("case", ROWS)
def test_live_rows_are_bit_identical_to_the_full_form(pkg, table, monkeypatch, case, quirk):
    rig = Rig(pkg, case, quirk, sets=2)
    rig.assert_routes()
    Bu = rig.Bu
    state = rig.rng.standard_normal((rig.ns, fc.ACT_COLS)).astype(np.float32)
    dstate = to_dev(state.T, torch.float32)
    losses = [torch.zeros(2, dtype=torch.float32, device="cuda:0") for _ in range(2)]

    def both(f):
        """f(0) with the full form, f(1) with the live counts"""
        monkeypatch.setenv("PDEC_FUSED_FULL_ROWS", "1")
        a = f(0)
        monkeypatch.delenv("PDEC_FUSED_FULL_ROWS")
        return a, f(1)
    a0, a1 = both(lambda i: rig.act(dstate, fc.ACT_COLS, i))         # (publishes the image of the initial parameters)
    assert np.array_equal(a0, a1)
    moved = 0.0
    for it in range(3):
        dv = rig.dev(rig.batch(Bu, safe=False))
        both(lambda i: rig.update_async(dv, Bu, i, losses=losses[i]))
        torch.cuda.synchronize()
        assert torch.equal(losses[0], losses[1]), (case, it, losses)
        full, live = _snapshot(rig, 0), _snapshot(rig, 1)
        for name in full:
            assert np.array_equal(full[name], live[name]), f"{case} quirk={quirk}: update {it}, {name} differs from the full form"
        assert all(np.isfinite(v).all() for v in live.values())
        moved = max(moved, np.abs(live["actor gradient buffer"]).max() * np.abs(live["critic gradient buffer"]).max())
    assert moved > 0
    b0, b1 = both(lambda i: rig.act(dstate, fc.ACT_COLS, i))
    assert np.array_equal(b0, b1)
    assert np.abs(b1 - a1).max() >= 1e-4          # the updates moved the actor: the acting kernel read the new image


@pytest.mark.parametrize("quirk", [1, 0])
@pytest.mark.parametrize("case", list(EXTRA))
def test_new_rows_match_the_oracle(pkg, table, case, quirk):
    """every gradient array of one update, both losses and the norm ratio, as test_gradients_match_the_oracle checks its rows"""
    rig = Rig(pkg, case, quirk)
    rig.assert_routes()
    batch = rig.batch(rig.Bu, safe=True)
    gC, gA, lv = rig.grads(rig.dev(batch), rig.Bu)
    _check_gradients(rig, gC, gA, lv, batch)
