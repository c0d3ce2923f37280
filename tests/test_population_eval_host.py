"""Host side of the one-launch population evaluation (population.py: member_workgroups, score_members; the C ABI of
pdec_rollout_members in include/pdeconv.h, its ctypes and Julia bindings).  No GPU needed."""
import importlib
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pop(pkg):
    return importlib.import_module(pkg.__name__ + ".population")


def test_workgroup_map_covers_every_trajectory_once_and_never_pairs_two_members(pkg):
    """the map the KS member kernel uses (workgroup -> member, pair, first trajectory, has a second one): for all M, K <= 5
    every trajectory of B = M K is served exactly once, both trajectories of a workgroup belong to its member, and member m's
    workgroups are the pairs a solo launch on K trajectories makes"""
    mw = _pop(pkg).member_workgroups
    for M in range(1, 6):
        for K in range(1, 6):
            wgs = mw(M, K)
            assert len(wgs) == M * ((K + 1) // 2)
            seen = []
            for w, (m, pair, b0, has1) in enumerate(wgs):
                assert (m, pair) == divmod(w, (K + 1) // 2)
                served = [b0] + ([b0 + 1] if has1 else [])
                assert all(b // K == m for b in served), (M, K, w)
                seen += served
            assert sorted(seen) == list(range(M * K)), (M, K)
            solo = [(pair, b0, has1) for _, pair, b0, has1 in mw(1, K)]
            for m in range(M):
                assert [(pair, b0 - m * K, has1) for mm, pair, b0, has1 in wgs if mm == m] == solo


def test_score_and_order_rule(pkg):
    sm = _pop(pkg).score_members
    er = np.array([[-3.0, -5.0], [-1.0, -2.0], [-4.0, -4.0], [-1.0, -2.0], [-0.5, np.nan], [-0.1, -0.1]])
    ds = np.full((6, 2), -1)
    ds[5, 1] = 17                                     # the best-looking member blew up in one of its trajectories
    score, order = sm(er, ds)
    assert np.array_equal(score[:4], [-4.0, -1.5, -4.0, -1.5]) and np.isnan(score[4]) and np.isnan(score[5])
    assert order == [1, 3, 0, 2, 4, 5]                # best first, ties by index, NaN last (by index)
    score, order = sm(np.array([[np.inf], [-2.0]]), np.full((2, 1), -1))
    assert np.isnan(score[0]) and order == [1, 0]
    score, order = sm(np.full((3, 4), np.nan), np.zeros((3, 4), dtype=np.int32))
    assert np.isnan(score).all() and order == [0, 1, 2]
    # a blow-up at step 0 counts (done_step = 0), -1 does not
    score, order = sm(np.array([[-1.0], [-2.0]]), np.array([[0], [-1]]))
    assert np.isnan(score[0]) and score[1] == -2.0 and order == [1, 0]


def test_rollout_members_is_declared_bound_and_exported(pkg):
    """pdec_rollout_members: declared in include/pdeconv.h, bound by ctypes with as many arguments, bound in
    julia/PDEenvHIP.jl with matching arity (type tuple and actual arguments), named in INTEGRATION.md, exported by the library"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdeconv.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+pdec_rollout_members\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)
    assert m, "pdec_rollout_members is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 18 and args[0] == "pdec_handle env" and args[1] == "const pdec_handle* actors" and args[-1] == "int* served"
    assert len(pkg._lib.SIGNATURES["pdec_rollout_members"]) == len(args)
    jl = open(os.path.join(ROOT, "julia", "PDEenvHIP.jl")).read()
    call = re.search(r"ccall\(\(:pdec_rollout_members, LIB\),\s*Cint,\s*\((.*?)\),\s*(.*?)\)\)", jl, flags=re.S)
    assert call, "julia/PDEenvHIP.jl does not bind pdec_rollout_members"
    assert len([a for a in call.group(1).replace("\n", " ").split(",") if a.strip()]) == len(args)
    assert len([a for a in call.group(2).replace("\n", " ").split(",") if a.strip()]) == len(args)
    assert "pdec_rollout_members" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    import ctypes
    assert hasattr(ctypes.CDLL(pkg._lib.LIB_PATH), "pdec_rollout_members")
    assert callable(pkg.evaluate_actors) and callable(pkg.Population.evaluate)
