"""Population-based selection: who takes over whom, and how the takers' hyper-parameters are perturbed (pure host logic;
Population.exploit applies a plan with Population.clone and set_hyper)."""
import numpy as np

PERTURBED = ("actor_lr", "critic_lr", "act_noise")      # what exploit's perturbation multiplies


def plan_exploit(score, order, frac=0.25):
    """[(dst, src), ...] of one exploit step on M members from an evaluation's `score` [M] (NaN: not rankable) and `order` (best
    first, NaN last, ties by index: score_members).  n = max(1, floor(frac M)), frac <= 0.5; the sources are the best n members
    of `order` with a finite score, the destinations the worst n of `order` followed by every NaN-scored member not among them
    (each group in `order`'s sequence); destination k takes source k mod n_sources.  Empty when no score is finite.  No member is
    both a source and a destination."""
    score = np.asarray(score, dtype=np.float64)
    order = [int(m) for m in order]
    M = len(order)
    if not 0.0 < frac <= 0.5:
        raise ValueError(f"plan_exploit: frac must lie in (0, 0.5] (got {frac!r})")
    if score.shape != (M,) or sorted(order) != list(range(M)):
        raise ValueError("plan_exploit: score [M] and order (a permutation of the M members) are needed")
    n = max(1, int(np.floor(frac * M)))
    sources = [m for m in order[:n] if np.isfinite(score[m])]
    if not sources:
        return []
    worst = order[M - n:]
    dests = [m for m in worst + [m for m in order[:M - n] if not np.isfinite(score[m])] if m not in sources]
    return [(d, sources[k % len(sources)]) for k, d in enumerate(dests)]


def perturb_factors(rng, n, lo, hi):
    """[n, len(PERTURBED)] factors of exploit's perturbation, each `lo` or `hi` with equal probability, from ONE draw of the
    numpy Generator `rng` (row k: destination k of the plan; columns: PERTURBED)"""
    pick = rng.integers(0, 2, size=(int(n), len(PERTURBED)))
    return np.where(pick == 0, float(lo), float(hi))
