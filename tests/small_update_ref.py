"""fp64 reference checks of ONE launch of the small DDPG update (pdec_ddpg_update_small / _rng: `loops` minibatch
updates of the reference's update!, src/PDEagent.jl:363-418), built on oracle.nn.  Test infrastructure, host only.

A launch is judged from the learner state before and after it -- a `Snap`: the four networks' parameters (Flux layout),
the behaviour networks' ADAM moments and beta powers -- read back from the device (teacher forcing: the reference of an
update starts from the state the kernel actually had, so legitimate fp32 rounding never compounds).  Two kinds of launch
have closed forms:
  * loops == 1, real learning rates: gradients, ADAM step, Polyak, beta powers, losses of the one update; the actor's
    reference gradient is taken through the critic the launch produced (`after`), so a critic ADAM step that rounds
    differently near g ~ 0 cannot show up as an actor error -- the critic's own step is checked on its own;
  * any loops, eta_actor = eta_critic = 0: the parameters stay put, so m, v, the beta powers and (rho < 1) the targets
    after L loops are sums over the L per-minibatch fp64 gradients, and every loop's slots and gradient count.

check_launch() returns the list of what is wrong (empty: the launch is right) and, given a dict `worst`, keeps in it the
largest error of every check as a fraction of its tolerance.  Tolerances: fp32 gradients <= 1e-4 relative
per tensor against fp64.

Batched updates (tests/pipeline_ref.py) add two things: reward groups (`group` = (g, L), tests/reward_group_ref.py) and
ReLU kinks (`kinks=True`).  At thousands of columns some pre-activations lie within fp32 rounding of 0, and the kernel may
legitimately take the other branch there; the bound of every gradient entry then widens by the |terms| those units carry,
and only by them."""
import copy
from dataclasses import dataclass, field

import numpy as np

from oracle import nn
import reward_group_ref as rg

B1, B2, EPS = 0.9, 0.999, 1e-8
TOL_G = 1e-4          # fp32 gradient vs fp64, relative to the tensor's largest entry
COND = 1e-5           # fp32 rounding of a sum of up to a few hundred terms, relative to the sum of their magnitudes


@dataclass
class Snap:
    """learner state around a launch; lists are Flux-layout fp32 arrays [W1, b1, W2, b2, ...]"""
    A: list
    C: list
    At: list
    Ct: list
    mA: list
    vA: list
    mC: list
    vC: list
    bpA: np.ndarray = field(default_factory=lambda: np.array([B1, B2]))
    bpC: np.ndarray = field(default_factory=lambda: np.array([B1, B2]))
    losses: tuple = (np.nan, np.nan)       # (critic loss, actor loss) of the launch's last update

    def copy(self):
        return copy.deepcopy(self)


def fresh_snap(A, C, At, Ct):
    z = lambda P: [np.zeros_like(p) for p in P]
    return Snap([p.copy() for p in A], [p.copy() for p in C], [p.copy() for p in At], [p.copy() for p in Ct],
                z(A), z(A), z(C), z(C))


def minibatches(S, Aa, R, T, slots):
    """the launch's minibatches from the replay traces (S [slot, ns], Aa [slot, na], R / T [slot]) and the slot table
    [3, loops, Bu] (rows: s/a, r/t, s' slots) -> list of (s, a, r, t, s') in the oracle's [features, Bu] layout"""
    return [(S[slots[0, k]].T, Aa[slots[0, k]].T, R[slots[1, k]], T[slots[1, k]], S[slots[2, k]].T)
            for k in range(slots.shape[1])]


def _f64(P):
    return [np.asarray(p, dtype=np.float64) for p in P]


def _abs_backward(params, acts, zs, as_, dy, amb=None, amb_on=True):
    """nn.backward with every factor replaced by its magnitude: per gradient entry the sum of |terms| an fp32 evaluation
    rounds, i.e. the scale of its rounding error when the terms cancel (returns grads, |dx|).  amb: per layer, the units
    whose ReLU branch fp32 may take either way (_ambiguous); they pass their |term| as if active (amb_on) or pass nothing"""
    grads = [None] * len(params)
    d = np.abs(dy)
    for li in reversed(range(len(acts))):
        g = np.abs(nn.act_grad(zs[li], as_[li + 1], acts[li]))
        if amb is not None and amb[li] is not None:
            g = np.maximum(g, amb[li]) if amb_on else g * (1 - amb[li])
        dz = d * g
        grads[2 * li] = dz @ np.abs(as_[li]).T
        grads[2 * li + 1] = dz.sum(axis=1)
        d = np.abs(params[2 * li]).T @ dz
    return grads, d


def _ambiguous(params, acts, zs, as_):
    """per layer: the ReLU units whose pre-activation lies within fp32 rounding of 0 (COND x the sum of the |terms| it
    adds), None for other activations"""
    out = []
    for li, kind in enumerate(acts):
        if kind != nn.RELU:
            out.append(None)
            continue
        zabs = np.abs(params[2 * li]) @ np.abs(as_[li]) + np.abs(params[2 * li + 1])[:, None]
        out.append((np.abs(zs[li]) <= COND * zabs).astype(np.float64))
    return out


def _bound(params, acts, zs, as_, dy, kinks, dy_kinks=None):
    """gradient magnitude bound in units of COND (see _check_net), |dx| and its kink-widened form; with kinks, every
    |term| that passes through an ambiguous unit (_ambiguous) -- active or not in fp64, fp32 may drop or add it -- is added
    whole, not scaled by COND: the sum with every ambiguous unit on less the sum with all of them off.  dy_kinks: the
    widened |dy| of a downstream kink bound (its extra terms count whole as well)"""
    grads, dx = _abs_backward(params, acts, zs, as_, dy)
    if not kinks:
        return grads, dx, dx
    amb = _ambiguous(params, acts, zs, as_)
    wide, dxw = _abs_backward(params, acts, zs, as_, dy if dy_kinks is None else dy_kinks, amb, True)
    off, _ = _abs_backward(params, acts, zs, as_, dy, amb, False)
    return [g + (w - o) / COND for g, w, o in zip(grads, wide, off)], dx, dxw


def critic_grad64(st, acts_a, acts_c, mb, gamma, quirk, group=None, kinks=False):
    """fp64 critic gradient, loss and gradient magnitude bound (_abs_backward) of one minibatch from the fp32 state `st`
    (gamma: the fp32 value the kernel uses; group: reward groups (g, L) of the broadcast, reward_group_ref)"""
    s, a, r, t, sn = (np.asarray(x, dtype=np.float64) for x in mb)
    g32 = float(np.float32(gamma))
    if group is not None:
        out = rg.grouped_losses_and_grads(_f64(st.A), _f64(st.C), _f64(st.At), _f64(st.Ct), acts_a, acts_c, s, a, r, t, sn,
                                          g32, *group)
        rabs = rg.group_mean_reward(np.abs(r), *group)
    else:
        out = nn.ddpg_losses_and_grads(_f64(st.A), _f64(st.C), _f64(st.At), _f64(st.Ct), acts_a, acts_c, s, a, r, t, sn,
                                       g32, bool(quirk))
        rabs = np.abs(r).mean() if quirk else np.abs(r)
    C = _f64(st.C)
    _, zs, as_ = nn.forward(C, acts_c, np.concatenate([s, a]), keep=True)
    ti = np.abs(g32 * (1 - t) * out["qt"])
    e = rabs + ti + np.abs(out["q"])
    return out["gC"], float(out["critic_loss"]), _bound(C, acts_c, zs, as_, (2.0 / s.shape[1]) * e[None, :], kinks)[0]


def actor_grad64(A, C, acts_a, acts_c, s, kinks=False):
    """fp64 actor gradient, loss and gradient magnitude bound through the critic C"""
    A, C, s = _f64(A), _f64(C), np.asarray(s, dtype=np.float64)
    out = nn.actor_grads(A, C, acts_a, acts_c, s)
    aout, zsa, asa = nn.forward(A, acts_a, s, keep=True)
    _, zs, as_ = nn.forward(C, acts_c, np.concatenate([s, aout]), keep=True)
    _, dx, dxw = _bound(C, acts_c, zs, as_, np.full((1, s.shape[1]), 1.0 / s.shape[1]), kinks)
    ns = s.shape[0]
    return out["gA"], float(out["actor_loss"]), _bound(A, acts_a, zsa, asa, dx[ns:], kinks, dxw[ns:])[0]


def relerr(x, ref):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(x - ref).max() / max(1e-30, np.abs(ref).max()))


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def _moments(m0, v0, grads, bounds):
    """Flux ADAM's moments after the gradients `grads` (one list per update), fp64, and how far fp32 gradients may move
    them: COND x the gradient magnitude bounds, carried through the same recurrences"""
    m, v = _f64(m0), _f64(v0)
    dm = [np.zeros_like(x) for x in m]
    dv = [np.zeros_like(x) for x in v]
    for g, b in zip(grads, bounds):
        m = [B1 * mi + (1 - B1) * gi for mi, gi in zip(m, g)]
        v = [B2 * vi + (1 - B2) * gi * gi for vi, gi in zip(v, g)]
        dm = [B1 * x + (1 - B1) * COND * bi for x, bi in zip(dm, b)]
        dv = [B2 * x + (1 - B2) * 2 * np.abs(gi) * COND * bi for x, gi, bi in zip(dv, g, b)]
    return m, v, dm, dv


def _keep(worst, key, ratio):
    if worst is not None:
        worst[key] = max(worst.get(key, 0.0), float(ratio))


def _over(x, ref, slack, tol):
    """entries of x off ref by more than tol x the tensor's largest |ref| + slack (elementwise); returns the worst ratio"""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float((np.abs(x - ref) / (tol * np.abs(ref).max() + slack + 1e-300)).max())


def _check_net(errs, tag, p0, p1, m0, v0, m1, v1, bp0, bp1, grads, bounds, eta, loops, worst=None):
    """one behaviour network: gradient (through m), m, v, ADAM step, beta powers.  Besides TOL_G of the tensor's largest
    entry, an entry may be off by COND x the sum of the |terms| its fp32 evaluation adds (where they cancel, the rounding
    of the terms, not the sum, sets the error) and by the fp32 rounding of the stored moments"""
    if loops == 1:
        # the gradient the kernel used, recovered from its moments: g = (m_new - b1 m_old) / (1 - b1)
        for i, (a, b, g, c) in enumerate(zip(m1, m0, grads[0], bounds[0])):
            gk = (np.asarray(a, np.float64) - B1 * np.asarray(b, np.float64)) / (1 - B1)
            e = _over(gk, g, COND * c + (_ulp(a) + B1 * _ulp(b)) / (1 - B1), TOL_G)
            _keep(worst, f"{tag} gradient", e)
            if e > 1:
                errs.append(f"{tag}: gradient of tensor {i} off by {e:.2f} x its tolerance (from m)")
    mr, vr, dm, dv = _moments(m0, v0, grads, bounds)
    for i in range(len(p0)):
        e = _over(m1[i], mr[i], dm[i] + 2 * _ulp(mr[i]), TOL_G)
        _keep(worst, f"{tag} m", e)
        if e > 1:
            errs.append(f"{tag}: m of tensor {i} off by {e:.2f} x its tolerance")
        e = _over(v1[i], vr[i], dv[i] + 2 * _ulp(vr[i]), 2 * TOL_G)      # v holds g^2: twice the gradient's relative error
        _keep(worst, f"{tag} v", e)
        if e > 1:
            errs.append(f"{tag}: v of tensor {i} off by {e:.2f} x its tolerance")
    # beta powers: advanced once per update, fp64, by repeated multiplication like Flux
    bp = np.array(bp0, dtype=np.float64)
    for _ in range(loops):
        bp = bp * np.array([B1, B2])
    if not np.array_equal(np.asarray(bp1, dtype=np.float64), bp):
        errs.append(f"{tag}: beta powers {list(bp1)} != {list(bp)}")
    # ADAM step from the kernel's own new moments (fp64), p_new = p_old - eta mhat / (sqrt(vhat) + eps):
    # within the rounding of p_new and 1e-5 of the step
    for i in range(len(p0)):
        if eta == 0:
            if not np.array_equal(p1[i], p0[i]):
                errs.append(f"{tag}: parameters of tensor {i} moved at eta = 0")
            continue
        mh = np.asarray(m1[i], np.float64) / (1 - bp0[0])
        vh = np.asarray(v1[i], np.float64) / (1 - bp0[1])
        d = mh / (np.sqrt(vh) + EPS) * eta
        ref = np.asarray(p0[i], np.float64) - d
        dev = np.abs(np.asarray(p1[i], np.float64) - ref)
        _keep(worst, f"{tag} ADAM step", (dev / (_ulp(ref) + 1e-5 * np.abs(d) + 1e-300)).max())
        bad = dev > _ulp(ref) + 1e-5 * np.abs(d)
        if bad.any():
            errs.append(f"{tag}: ADAM step of tensor {i} wrong at {int(bad.sum())} entries")


def _polyak32(dst, src, rho):
    """dest = rho dest + (1 - rho) src in fp32 with the products rounded, as the kernels compute it"""
    r32 = np.float32(rho)
    omr = np.float32(1) - r32
    return [(r32 * np.asarray(d, np.float32)) + (omr * np.asarray(s, np.float32)) for d, s in zip(dst, src)]


def _check_polyak(errs, tag, pt0, pt1, p1, rho, loops, worst=None):
    if np.float32(rho) == np.float32(1):
        for i, (a, b) in enumerate(zip(pt1, pt0)):
            _keep(worst, f"{tag} Polyak", 0.0 if np.array_equal(a, b) else np.inf)
            if not np.array_equal(a, b):
                errs.append(f"{tag}: frozen target (rho = 1) changed in tensor {i}")
        return
    ref = pt0
    for _ in range(loops):          # (src fixed: loops == 1 or eta == 0)
        ref = _polyak32(ref, p1, rho)
    for i in range(len(pt0)):
        dev = np.abs(np.asarray(pt1[i], np.float64) - ref[i])
        _keep(worst, f"{tag} Polyak", (dev / (4 * _ulp(ref[i]) + 1e-30)).max())
        bad = dev > 4 * _ulp(ref[i]) + 1e-30
        if bad.any():
            errs.append(f"{tag}: Polyak of tensor {i} wrong at {int(bad.sum())} entries")


def _check_loss(errs, tag, got, ref, worst=None):
    # a mean of O(1) squared / summed fp32 terms: gradient-level tolerance against the larger of |ref| and 1
    _keep(worst, tag, abs(float(got) - ref) / (TOL_G * max(1.0, abs(ref))))
    if not abs(float(got) - ref) <= TOL_G * max(1.0, abs(ref)):
        errs.append(f"{tag}: {got} vs fp64 {ref}")


def check_launch(before, after, mbs, acts_a, acts_c, gamma, rho, quirk, eta_a, eta_c, check_losses=True, group=None,
                 kinks=False, worst=None):
    """what is wrong with `after` as the result of one launch of len(mbs) updates on `before` (see the module doc)"""
    loops = len(mbs)
    assert loops == 1 or (eta_a == 0 and eta_c == 0), "closed forms: one update, or any number at eta = 0"
    errs = []
    gCs, gAs, bCs, bAs, cl, al = [], [], [], [], np.nan, np.nan
    cur = before.copy()
    for mb in mbs:
        g, cl, b = critic_grad64(cur, acts_a, acts_c, mb, gamma, quirk, group, kinks)
        gCs.append(g)
        bCs.append(b)
        g, al, b = actor_grad64(before.A, after.C, acts_a, acts_c, mb[0], kinks)     # through the critic the launch produced
        gAs.append(g)
        bAs.append(b)
        cur.At, cur.Ct = _polyak32(cur.At, before.A, rho), _polyak32(cur.Ct, before.C, rho)   # (eta = 0: the targets still move)
    _check_net(errs, "critic", before.C, after.C, before.mC, before.vC, after.mC, after.vC, before.bpC, after.bpC, gCs,
               bCs, eta_c, loops, worst)
    _check_net(errs, "actor", before.A, after.A, before.mA, before.vA, after.mA, after.vA, before.bpA, after.bpA, gAs,
               bAs, eta_a, loops, worst)
    _check_polyak(errs, "target critic", before.Ct, after.Ct, after.C, rho, loops, worst)
    _check_polyak(errs, "target actor", before.At, after.At, after.A, rho, loops, worst)
    if check_losses:
        _check_loss(errs, "critic loss", after.losses[0], cl, worst)
        _check_loss(errs, "actor loss", after.losses[1], al, worst)
    return errs
