"""fp64 restatement of the grouped reward broadcast (include/pdeconv.h, pdec_ddpg_set_reward_groups), built on oracle.nn.
Test infrastructure, host only.

The reference's critic target r .+ y .* (1 .- t) .* qt (src/PDEagent.jl:388) broadcasts the 1 x Bu reward row against the
Bu-vector of targets, so every sample of a minibatch sees the minibatch's mean reward.  Read at batch scale, an update of
Bu columns is the mean of Bu / g such minibatch losses: column c belongs to group (c / (g L)) L + c % L, and with
d = gamma (1 - t) qt - q and r_bar(c) the mean reward of c's group
    loss = mean(d^2) + 2 mean_c(d_c r_bar(c)) + mean(r^2),    dL/dq_c = -(2 / Bu) (r_bar(c) + d_c)."""
import numpy as np

from oracle import nn


def group_index(Bu, g, L=1):
    """group of every column c: (c // (g L)) L + c % L"""
    c = np.arange(Bu)
    return (c // (g * L)) * L + c % L


def group_members(Bu, g, L=1):
    """[Bu / g, g] column indices of each group, members in ascending order"""
    idx = group_index(Bu, g, L)
    order = np.argsort(idx, kind="stable")
    return order.reshape(-1, g)


def group_mean_reward(r, g, L=1):
    """r_bar(c) for every column, fp64"""
    r = np.asarray(r, dtype=np.float64)
    idx = group_index(r.size, g, L)
    return (np.bincount(idx, weights=r) / np.bincount(idx))[idx]


def grouped_losses_and_grads(A, C, At, Ct, acts_a, acts_c, s, a, r, t, snext, gamma, g, L=1):
    """critic loss and gradient of one update under reward groups (g, L); arrays as oracle.nn.ddpg_losses_and_grads
    (s, snext [ns, Bu]; a [na, Bu]; r, t [Bu]).  Returns dict(critic_loss, gC, q, qt, dq, rbar)."""
    dt = s.dtype
    Bu = s.shape[1]
    assert Bu % (g * L) == 0, (Bu, g, L)
    anext = nn.forward(At, acts_a, snext)
    qt = nn.forward(Ct, acts_c, np.concatenate([snext, anext])).reshape(-1)
    d = dt.type(gamma) * (1 - t.astype(dt)) * qt
    q, zs, as_ = nn.forward(C, acts_c, np.concatenate([s, a]), keep=True)
    q = q.reshape(-1)
    d = d - q
    rbar = group_mean_reward(r, g, L).astype(dt)
    r64, d64 = r.astype(np.float64), d.astype(np.float64)
    closs = dt.type(np.mean(d64 * d64) + 2.0 * np.mean(d64 * rbar) + np.mean(r64 * r64))
    dq = -(2.0 / Bu) * (rbar + d)
    gC, _ = nn.backward(C, acts_c, zs, as_, dq[None, :].astype(dt))
    return dict(critic_loss=closs, gC=gC, q=q, qt=qt, dq=dq, rbar=rbar)


def critic_grad_of_dq(C, acts_c, s, a, dq):
    """dL/dtheta of the critic for a given dL/dq row (closed-form differences of the gradient)"""
    _, zs, as_ = nn.forward(C, acts_c, np.concatenate([s, a]), keep=True)
    gC, _ = nn.backward(C, acts_c, zs, as_, np.asarray(dq, dtype=s.dtype)[None, :])
    return gC
