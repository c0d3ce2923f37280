"""The fp64 restatement of the grouped reward broadcast (tests/reward_group_ref.py) against oracle.nn: one group spanning
the batch is the reference's whole-batch broadcast, groups of one column the diagonal TD target, and any grouping the mean
of the reference's loss over its minibatches.  CPU only."""
import numpy as np
import pytest

from oracle import nn
from reward_group_ref import group_index, group_members, grouped_losses_and_grads


def _problem(seed, Bu, ns=3):
    rng = np.random.default_rng(seed)
    da, aa = nn.layer_sizes(ns, 1, 1.6, True, False)
    dc, ac = nn.layer_sizes(ns, 1, 2.0, False, False)
    nets = [nn.glorot_uniform(rng, d, np.float64) for d in (da, dc, da, dc)]
    for P in nets:
        for i in range(1, len(P), 2):
            P[i] = rng.standard_normal(P[i].shape) * 0.1
    s, sn = rng.standard_normal((ns, Bu)), rng.standard_normal((ns, Bu))
    a = rng.uniform(-1, 1, (1, Bu))
    r = -rng.uniform(0, 1, Bu)
    t = (rng.uniform(0, 1, Bu) < 0.2).astype(np.float64)
    return nets, aa, ac, s, a, r, t, sn


def _close(x, y, tol=1e-12):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return np.abs(x - y).max() <= tol * max(1.0, np.abs(y).max())


def test_group_index_is_l_strided():
    # L = A: actuator a of g consecutive trajectories (c = b A + a)
    A, g = 4, 3
    idx = group_index(2 * g * A, g, A)
    assert list(idx[:g * A]) == [0, 1, 2, 3] * 3
    assert list(idx[g * A:]) == [4, 5, 6, 7] * 3
    assert group_members(12, 3, 4)[1].tolist() == [1, 5, 9]
    assert group_members(6, 3, 1).tolist() == [[0, 1, 2], [3, 4, 5]]


@pytest.mark.parametrize("Bu", [12, 30])
def test_one_group_is_the_whole_batch_broadcast(Bu):
    (A, C, At, Ct), aa, ac, s, a, r, t, sn = _problem(1 + Bu, Bu)
    got = grouped_losses_and_grads(A, C, At, Ct, aa, ac, s, a, r, t, sn, 0.99, Bu, 1)
    want = nn.ddpg_losses_and_grads(A, C, At, Ct, aa, ac, s, a, r, t, sn, 0.99, quirk=True)
    assert _close(got["critic_loss"], want["critic_loss"])
    for x, y in zip(got["gC"], want["gC"]):
        assert _close(x, y)


@pytest.mark.parametrize("L", [1, 3])
def test_groups_of_one_are_the_diagonal_target(L):
    Bu = 24
    (A, C, At, Ct), aa, ac, s, a, r, t, sn = _problem(5, Bu)
    got = grouped_losses_and_grads(A, C, At, Ct, aa, ac, s, a, r, t, sn, 0.99, 1, L)
    want = nn.ddpg_losses_and_grads(A, C, At, Ct, aa, ac, s, a, r, t, sn, 0.99, quirk=False)
    assert _close(got["critic_loss"], want["critic_loss"])
    for x, y in zip(got["gC"], want["gC"]):
        assert _close(x, y)


@pytest.mark.parametrize("g,L", [(3, 1), (3, 4), (2, 3)])
def test_groups_are_the_mean_of_reference_minibatch_updates(g, L):
    """loss and gradient = mean over the groups of the reference's own update on each group's g columns"""
    Bu = 36
    (A, C, At, Ct), aa, ac, s, a, r, t, sn = _problem(7 + g + L, Bu)
    got = grouped_losses_and_grads(A, C, At, Ct, aa, ac, s, a, r, t, sn, 0.99, g, L)
    per = []
    for cols in group_members(Bu, g, L):
        per.append(nn.ddpg_losses_and_grads(A, C, At, Ct, aa, ac, s[:, cols], a[:, cols], r[cols], t[cols], sn[:, cols],
                                            0.99, quirk=True))
    assert len(per) == Bu // g
    assert _close(got["critic_loss"], np.mean([p["critic_loss"] for p in per]))
    for i, x in enumerate(got["gC"]):
        assert _close(x, np.mean([p["gC"][i] for p in per], axis=0))
    # and it is neither of the two existing readings
    whole = nn.ddpg_losses_and_grads(A, C, At, Ct, aa, ac, s, a, r, t, sn, 0.99, quirk=True)
    diag = nn.ddpg_losses_and_grads(A, C, At, Ct, aa, ac, s, a, r, t, sn, 0.99, quirk=False)
    assert not _close(got["gC"][0], whole["gC"][0], 1e-6) and not _close(got["gC"][0], diag["gC"][0], 1e-6)
