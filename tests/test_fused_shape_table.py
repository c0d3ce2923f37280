"""The case table of test_gpu_fused_shapes.py against a plain-Python restatement of the shape rules of the fused DDPG passes
(fused_shape_cases.py), with the constants and instantiation lists read out of the .hip sources.  Runs without a GPU: it keeps
the table honest where nothing can be launched, and fails when a tile count joins a predicate without a case."""
import sys

import pytest

import fused_shape_cases as fc


@pytest.fixture(scope="module")
def k():
    return fc.read_constants()


def test_constants_are_the_ones_the_table_was_written_for(k):
    assert (k["KXP"], k["K2MAX"], k["FCOLS"], k["CPWMAX"]) == (16, 6, 128, 4)
    assert k["T3"] == [(9, 2), (9, 1), (2, 2), (2, 1)] and k["A3"] == [2, 1]
    assert k["T2"] == [(22, 2), (22, 1), (9, 2), (9, 1)] and k["A2"] == [2, 1] and k["KB2"] == [2, 5, 6]
    assert (k["ACT2_MIN_COLS"], k["APPLY2_MIN_BU"], k["ACT3_MAX_H"]) == (256, 64, 31)
    assert (k["LDP"], k["LDQ"]) == (72, 40)


def test_table_imports_without_torch_or_the_library():
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); import fused_shape_cases as fc; "
            "assert 'torch' not in sys.modules and 'numpy' not in sys.modules; print(len(fc.CASES))") % fc.os.path.dirname(fc.__file__)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert int(out.stdout) == len(fc.CASES)


@pytest.mark.parametrize("case", list(fc.CASES))
def test_every_row_names_what_the_rules_pick(k, case):
    layers, ns, ha, hc, Bu, scale, pair, act = fc.CASES[case]
    assert fc.rule(layers, ns, ha, hc, k) == (pair, act)
    assert (case in fc.OUTSIDE) == (pair is None) == case.startswith("o")
    assert Bu >= 1 and scale > 0


def test_rows_reach_every_instantiation_and_nothing_else(k):
    pairs, acts = fc.all_names(k)
    assert len(pairs) == 4 + 12 and len(acts) == 2 + 6
    got = [fc.kernel_names(c) for c in fc.FUSED]
    assert {(g[0], g[1]) for g in got} == pairs
    assert {g[2] for g in got} == acts


def test_width_and_row_edges_are_all_there():
    rows = [fc.CASES[c] for c in fc.FUSED]
    l3 = [r for r in rows if r[0] == 3]
    l2 = [r for r in rows if r[0] == 2]
    assert {128, 143, 16, 31} <= {r[3] for r in l3} and {336, 351, 128, 143} <= {r[3] for r in l2}
    assert {1, 15, 16, 31} <= {r[2] for r in l3} and {1, 15, 16, 31} <= {r[2] for r in l2}
    assert {1, 14} <= {r[1] for r in l3}
    assert {6, 7, 14, 15, 16, 30, 31, 39, 40, 46} <= {r[1] for r in l2}
    for fam in (l3, l2):
        assert {1, 15, 17, 127, 129, 63, 64} <= {r[4] for r in fam}
    assert (3, 14, 15, 143) in {r[:4] for r in l3} and (2, 46, 31, 351) in {r[:4] for r in l2}
    out = [fc.CASES[c] for c in fc.OUTSIDE]
    assert {127, 144, 32} <= {r[3] for r in out if r[0] == 3} and {335, 352, 127, 144} <= {r[3] for r in out if r[0] == 2}
    assert {3, 2} == {r[0] for r in out if r[2] == 32}
    assert (3, 15) in {r[:2] for r in out} and (2, 47) in {r[:2] for r in out}


def test_batch_edges_of_both_grid_rules(k):
    """3-layer: the batch-mean reward becomes its own launch above 256 FCOLS columns; 2-layer: grid2_of deals tiles above 256
    chunks -- the figures the table's comment states"""
    l3 = {fc.CASES[c][4] for c in fc.FUSED if fc.CASES[c][0] == 3}
    assert {256 * k["FCOLS"], 256 * k["FCOLS"] + 1} <= l3
    l2 = {fc.CASES[c][4] for c in fc.FUSED if fc.CASES[c][0] == 2}
    assert {32789, 32835, 65536} <= l2
    assert fc.grid2_rule(32768, k) == (256, 8, 8, 16)             # the last batch of the one-chunk-per-workgroup regime
    assert fc.grid2_rule(32789, k) == (228, 9, 7, 5)
    assert fc.grid2_rule(32835, k) == (229, 9, 1, 3)
    assert fc.grid2_rule(65536, k) == (256, 16, 16, 16)
    assert fc.grid2_rule(100352, k) == (251, 25, 22, 16)          # config C4 (test_gpu_grads.py)


def test_lds_rule_of_the_two_layer_passes(k):
    """the dynamic LDS of every 2-layer row stays within the 160 KiB of a CU (64 KiB for the acting kernel's launch), and the
    rule reproduces the bytes that pdec_debug_batched_update_route reported for the corner row before the layouts became
    Critic2Lds / Actor2Lds / Act2Lds: ddpg2_critic_kernel<22,2,6> 148 384, ddpg2_actor_kernel<22,2,6> 107 200,
    policy_act2_kernel<2,6> 6 928"""
    for case, (layers, ns, ha, hc, _, _, pair, act) in fc.CASES.items():
        if layers != 2:
            continue
        if pair is not None:
            critic, actor, _ = fc.lds2_rule(ns, ha, hc, k)
            assert 0 < critic <= 160 * 1024 and 0 < actor <= 160 * 1024, (case, critic, actor)
        if act is not None:
            assert 0 < fc.lds2_rule(ns, ha, hc, k)[2] <= 64 * 1024, case
    for case in ("l2_ns46_a31_c351_bu32789", "l2_ns46_a31_c351_bu65536"):
        _, ns, ha, hc = fc.CASES[case][:4]
        assert fc.lds2_rule(ns, ha, hc, k) == (148384, 107200, 6928)
