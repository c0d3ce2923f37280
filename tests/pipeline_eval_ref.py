"""Host restatement of TrainPipeline's greedy held-out evaluation (pipeline.py module docstring, csrc/ledger.hip) in NumPy, shared
by the GPU tests: the numbers of one evaluation from a rollout's reward_sum / done_step, and the best-by-evaluation rule."""
import numpy as np


def restate_eval(reward_sum, done_step):
    """(ret [K] float64, blew [K] bool, score): ret_b = (sum over a, in index order, of the fp64 values reward_sum[b][a]) / R;
    blew_b = done_step[b] >= 0 (population.score_members' predicate); score = (sum over b in index order of ret_b) / K, NaN
    when any blew_b is set or any ret_b is not finite"""
    rs = np.asarray(reward_sum)
    K, R = rs.shape
    ret = np.zeros(K, dtype=np.float64)
    for b in range(K):
        s = np.float64(0.0)
        for a in range(R):
            s = s + np.float64(rs[b, a])
        ret[b] = s / np.float64(R)
    blew = np.asarray(done_step).reshape(K) >= 0
    t = np.float64(0.0)
    for b in range(K):
        t = t + ret[b]
    if blew.any() or not np.isfinite(ret).all():
        return ret, blew, float("nan")
    return ret, blew, float(t / np.float64(K))


def best_rule(episodes, scores, min_best_episode):
    """(bestreward, bestepisode) of PDEhook's rule (src/PDEhook.jl:65-76) on evaluation scores: an evaluation at an episode
    >= min_best_episode whose score is not NaN and >= every earlier such score becomes the best; (-1e6, 0) before any choice"""
    best, best_e, top = -1e6, 0, -np.inf
    for e, s in zip(episodes, scores):
        if int(e) >= int(min_best_episode) and not np.isnan(s) and s >= top:
            top = best = float(s)
            best_e = int(e)
    return best, best_e
