"""NumPy model of the device telemetry (csrc/telemetry.hip; TrainPipeline(telemetry=N)): the row a step call and an update call
write, the ring's read-out, and the error bound of every column -- derived from the arithmetic, not measured.

Every input is promoted to float64, which is exact for fp32 and fp64 inputs.  Entries that are not finite are left out of sums and
maxima and counted; a difference is left out when either of its two entries is not finite.

Bounds.  Counts, minima, maxima, the two losses, the `step` / `update` numbers and the sentinel involve no rounding: exact.  A sum
of n doubles taken in ANY order differs from the exact sum by at most (n - 1) 2^-53 sum|term| (first order; Higham, Accuracy and
Stability of Numerical Algorithms, 4.2), and where the terms are squares each carries one more rounding of 2^-53 relative; the
device and this model each commit at most that, so their difference is held to n 2^-52 sum|term| absolute.  A mean is such a sum
divided by a count (one more rounding, 2^-53 relative, inside the same allowance for n >= 1): the bound divided by the count."""
import numpy as np

STEP_COLUMNS = ("step", "reward_mean", "reward_min", "reward_max", "reward_nonfinite", "action_mean", "action_abs_mean",
                "action_saturated", "state_abs_max", "state_nonfinite", "blown_up", "terminal")
UPDATE_COLUMNS = ("update", "critic_loss", "actor_loss", "actor_norm2", "critic_norm2", "actor_target_dist2", "critic_target_dist2",
                  "actor_step2", "critic_step2", "actor_abs_max", "critic_abs_max", "actor_nonfinite", "critic_nonfinite")
EPS = 2.0 ** -52


def _sum(terms):
    """(sum, bound) of a 1-D float64 array of finite terms"""
    t = np.asarray(terms, dtype=np.float64).reshape(-1)
    return float(t.sum()), t.size * EPS * float(np.abs(t).sum())


def step_row(s_out, act, rew, term, flags, act_limit, step=0):
    """(row, bound): dicts over STEP_COLUMNS.  s_out [cols, ns], act [cols, na], rew / term [cols], flags [B]"""
    s = np.asarray(s_out).astype(np.float64).reshape(-1)
    a = np.asarray(act).astype(np.float64)
    a = a.reshape(a.shape[0], -1)[:, 0]
    r = np.asarray(rew).astype(np.float64).reshape(-1)
    cols = r.size
    assert a.size == cols and np.asarray(term).size == cols
    fin = np.isfinite(r)
    row, tol = {}, {k: 0.0 for k in STEP_COLUMNS}
    row["step"] = float(step)
    n = int(fin.sum())
    if n:
        rs, rb = _sum(r[fin])
        row["reward_mean"], tol["reward_mean"] = rs / n, rb / n
        row["reward_min"], row["reward_max"] = float(r[fin].min()), float(r[fin].max())
    else:
        row["reward_mean"] = row["reward_min"] = row["reward_max"] = float("nan")
    row["reward_nonfinite"] = float(cols - n)
    asum, ab = _sum(a)
    row["action_mean"], tol["action_mean"] = asum / cols, ab / cols
    asum, ab = _sum(np.abs(a))
    row["action_abs_mean"], tol["action_abs_mean"] = asum / cols, ab / cols
    row["action_saturated"] = float((np.abs(a) >= float(act_limit)).sum())
    sf = np.isfinite(s)
    row["state_abs_max"] = float(np.abs(s[sf]).max()) if sf.any() else 0.0
    row["state_nonfinite"] = float((~sf).sum())
    row["blown_up"] = float((np.asarray(flags).reshape(-1) != 0).sum())
    row["terminal"] = float((np.asarray(term).reshape(-1) != 0).sum())
    return row, tol


def flat(params):
    """the flat float64 vector of a network given as an array or a list of per-layer arrays (any order: sums do not care)"""
    if isinstance(params, np.ndarray):
        return params.astype(np.float64).reshape(-1)
    return np.concatenate([np.asarray(p).astype(np.float64).reshape(-1) for p in params])


def _net(x, xt, xp):
    fin = np.isfinite(x)
    out, tol = {}, {}
    out["norm2"], tol["norm2"] = _sum(x[fin] * x[fin])
    both = fin & np.isfinite(xt)
    d = x[both] - xt[both]
    out["target_dist2"], tol["target_dist2"] = _sum(d * d)
    if xp is None:
        out["step2"], tol["step2"] = 0.0, 0.0
    else:
        both = fin & np.isfinite(xp)
        d = x[both] - xp[both]
        out["step2"], tol["step2"] = _sum(d * d)
    out["abs_max"], tol["abs_max"] = (float(np.abs(x[fin]).max()) if fin.any() else 0.0), 0.0
    out["nonfinite"], tol["nonfinite"] = float((~fin).sum()), 0.0
    return out, tol


def update_row(losses, A, C, At, Ct, A_prev=None, C_prev=None, update=0):
    """(row, bound): dicts over UPDATE_COLUMNS.  losses = (critic, actor); A_prev / C_prev None: the first call (step2 = 0)"""
    row, tol = {k: 0.0 for k in UPDATE_COLUMNS}, {k: 0.0 for k in UPDATE_COLUMNS}
    row["update"] = float(update)
    row["critic_loss"], row["actor_loss"] = float(losses[0]), float(losses[1])
    for name, x, xt, xp in (("actor", A, At, A_prev), ("critic", C, Ct, C_prev)):
        o, t = _net(flat(x), flat(xt), None if xp is None else flat(xp))
        for k in o:
            row[f"{name}_{k}"], tol[f"{name}_{k}"] = o[k], t[k]
    return row, tol


def step_nonfinite(row):
    return row["reward_nonfinite"] + row["state_nonfinite"] > 0


def update_nonfinite(row):
    return (not np.isfinite(row["critic_loss"]) or not np.isfinite(row["actor_loss"])
            or row["actor_nonfinite"] + row["critic_nonfinite"] > 0)


def ring(rows, capacity):
    """(the rows a ring of `capacity` still holds, oldest first; how many it has dropped)"""
    rows = list(rows)
    n = min(len(rows), int(capacity))
    return rows[len(rows) - n:], len(rows) - n


def mismatches(got, want, tol, columns, where=""):
    """the columns of one row (got: name -> value) that miss the model by more than the bound"""
    bad = []
    for k in columns:
        g, w, t = float(got[k]), float(want[k]), float(tol[k])
        ok = (np.isnan(g) and np.isnan(w)) or g == w or abs(g - w) <= t
        if not ok:
            bad.append(f"{where}{k}: got {g!r}, want {w!r} +- {t:.3g}")
    return bad
