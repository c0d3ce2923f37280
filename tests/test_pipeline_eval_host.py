"""The host restatement of the pipeline's evaluation numbers and best rule (pipeline_eval_ref.py, which the GPU tests share) and
the package's own eval_score, held against population.score_members on hand-made arrays.  The values are dyadic, so every sum
is exact whatever its order and the restatement's ordered sums must equal score_members' NumPy means bit for bit."""
import importlib

import numpy as np
import pytest

from pipeline_eval_ref import best_rule, restate_eval


@pytest.fixture(scope="module")
def mods():
    return (importlib.import_module("distributedconvrl-pde-control_amd.population"),
            importlib.import_module("distributedconvrl-pde-control_amd.pipeline"))


CASES = {
    "plain": (np.array([[-1.0, -2.0, -0.5, -0.5], [-4.0, 0.0, -2.0, -2.0], [0.25, -0.25, -8.0, 0.0]]), np.array([-1, -1, -1])),
    "raised_flag": (np.array([[-1.0, -2.0], [-4.0, 0.0], [0.5, -0.5]]), np.array([-1, 0, -1])),
    "late_flag": (np.array([[-1.0, -2.0], [-4.0, 0.0]]), np.array([16, -1])),
    "nan_return": (np.array([[-1.0, np.nan], [-4.0, 0.0]]), np.array([-1, -1])),
    "inf_return": (np.array([[-1.0, -np.inf], [-4.0, 0.0]]), np.array([-1, -1])),
    "k1": (np.array([[-3.0, -1.0, -2.0, -2.0]]), np.array([-1])),
    "k1_flag": (np.array([[-3.0, -1.0]]), np.array([3])),
    "fp32": (np.array([[-1.5, -2.25], [-0.125, 0.0]], dtype=np.float32), np.array([-1, -1], dtype=np.int32)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_follows_score_members(mods, name):
    population, pipeline = mods
    rs, ds = CASES[name]
    ret, blew, score = restate_eval(rs, ds)
    want_ret = rs.astype(np.float64).mean(axis=1)
    assert np.array_equal(ret, want_ret, equal_nan=True)
    assert np.array_equal(blew, ds >= 0)
    want, order = population.score_members(want_ret[None, :], ds[None, :])
    assert np.array_equal(np.array([score]), want, equal_nan=True)
    assert np.isnan(score) == (name in ("raised_flag", "late_flag", "nan_return", "inf_return", "k1_flag"))
    # the package's own host statement (the zero-action baseline goes through it)
    r2, b2, s2 = pipeline.eval_score(rs, ds)
    assert np.array_equal(r2, ret, equal_nan=True) and np.array_equal(b2, blew)
    assert np.array_equal(np.array([s2]), np.array([score]), equal_nan=True)


def test_ordered_sums():
    """values whose sum depends on the order: the restatement adds in index order"""
    rs = np.array([[1e16, 1.0, -1e16, 1.0]])
    ret, _, score = restate_eval(rs, np.array([-1]))
    assert ret[0] == ((((0.0 + 1e16) + 1.0) - 1e16) + 1.0) / 4.0 == 0.25
    assert score == 0.25


def test_best_rule():
    nan = float("nan")
    # ties go to the later evaluation (>=), ineligible and NaN evaluations are skipped, a NaN does not block later ones
    assert best_rule([2, 4, 6, 8], [-1.0, -3.0, -1.0, -2.0], 0) == (-1.0, 6)
    assert best_rule([2, 4, 6, 8], [-1.0, -3.0, -1.0, -2.0], 7) == (-2.0, 8)
    assert best_rule([2, 4, 6, 8], [0.0, -3.0, nan, -2.0], 3) == (-2.0, 8)
    assert best_rule([2, 4, 6], [0.0, nan, -5.0], 3) == (-5.0, 6)
    assert best_rule([1, 2], [nan, nan], 0) == (-1e6, 0)
    assert best_rule([1, 2], [-1.0, -2.0], 3) == (-1e6, 0)
    assert best_rule([], [], 0) == (-1e6, 0)
    # the hand-made scores above against score_members' own NaN handling: a NaN-scored member ranks last, never first
    population = importlib.import_module("distributedconvrl-pde-control_amd.population")
    er = np.array([[0.0, 0.0], [-3.0, -3.0], [nan, 0.0], [-2.0, -2.0]])
    score, order = population.score_members(er, np.full((4, 2), -1))
    assert order[-1] == 2 and np.isnan(score[2])
    assert best_rule([1, 2, 3, 4], score, 0)[1] == 1 + order[0]
