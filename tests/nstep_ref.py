"""NumPy restatement of the n-step assembly (csrc/nstep.hip; include/pdeconv.h: pdec_nstep_step) -- test infrastructure, host only.
Ring-free: the model keeps the whole history and looks the window of step k up in it.

Rule, per column c, at step k with u = k - n + 1:
    m      = the smallest i in [0, n-1] with t_{u+i}[c] != 0, or n - 1 if there is none
    R[c]   = sum_{i=0..m} w_i r_{u+i}[c],  w_0 = 1, w_{i+1} = w_i gamma: float64, index order, a multiplication and an addition per
             term (NumPy's ufuncs never contract them), rounded once to the rows' dtype
    T[c]   = 1 if t_{u+m}[c] != 0 else 0
    state  = s_in_u[c], action = a_u[c]; next_state = s_out_k[c]
Rows before step 0 are zeros (what the device rings hold after creation); a caller ignores the windows that reach them."""
import numpy as np


def gamma_n(gamma, n):
    """w_n by the repeated multiplication of the rule"""
    w = 1.0
    for _ in range(int(n)):
        w = w * float(gamma)
    return w


def window_lengths(ts):
    """ts: [n][cols] terminal rows of one window, oldest first -> m [cols]"""
    ts = np.asarray(ts)
    n = ts.shape[0]
    hit = ts != 0
    return np.where(hit.any(axis=0), hit.argmax(axis=0), n - 1)


def window_return(rs, ts, gamma, dtype):
    """(R [cols] in dtype, T [cols] in dtype, m [cols]) of one window: rs, ts [n][cols], oldest first"""
    rs, ts = np.asarray(rs), np.asarray(ts)
    n, cols = rs.shape
    acc = np.zeros(cols, np.float64)
    alive = np.ones(cols, bool)
    T = np.zeros(cols, dtype)
    w = 1.0
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            term = w * rs[i].astype(np.float64)
            acc = np.where(alive, acc + term, acc)
            hit = alive & (ts[i] != 0)
            T[hit] = 1
            alive &= ~hit
            w = w * float(gamma)
        R = acc.astype(dtype)
    return R, T, window_lengths(ts)


class NStepModel:
    """feed the rows of step 0, 1, ... with push(); emit(k) is what step k's call writes"""

    def __init__(self, n, gamma):
        self.n, self.gamma = int(n), float(gamma)
        self.s, self.a, self.r, self.t = [], [], [], []

    def push(self, s, a, r, t):
        for lst, x in ((self.s, s), (self.a, a), (self.r, r), (self.t, t)):
            lst.append(np.array(x, copy=True))
        return self.emit(len(self.s) - 1)

    def _row(self, lst, i):
        return lst[i] if i >= 0 else np.zeros_like(lst[0])

    def emit(self, k):
        """dict(state, action, reward, terminal, m, start) of step k's batch"""
        u = k - self.n + 1
        rs = [self._row(self.r, i) for i in range(u, k + 1)]
        ts = [self._row(self.t, i) for i in range(u, k + 1)]
        R, T, m = window_return(rs, ts, self.gamma, self.r[0].dtype)
        return dict(state=self._row(self.s, u), action=self._row(self.a, u), reward=R, terminal=T, m=m, start=u)

    def ring(self):
        """the device rings after the last push: slot k mod n holds step k's row -> (S, A, R, T), each [n, ...]"""
        K = len(self.s)
        out = []
        for lst in (self.s, self.a, self.r, self.t):
            ring = np.zeros((self.n,) + lst[0].shape, lst[0].dtype)
            for k in range(max(0, K - self.n), K):
                ring[k % self.n] = lst[k]
            out.append(ring)
        return tuple(out)


def nstep_transition(trace, j, n, gamma):
    """the minibatch the update trains on when it reads the batch assembled at step j of a pipeline_ref.Trace: (state [cols, ns],
    action [cols, na], reward [cols], terminal [cols], next_state [cols, ns]) in the trace's dtype.  The window starts at
    j - n + 1 >= 0."""
    u = j - n + 1
    assert u >= 0, "the window reaches back before step 0"
    st = trace.steps
    R, T, _m = window_return([st[i].r for i in range(u, j + 1)], [st[i].t for i in range(u, j + 1)], gamma, st[j].r.dtype)
    return st[u].s_in, st[u].a, R, T, st[j].s_out


def first_update_steps(resets, n_steps, lag, n):
    """the steps k < n_steps that carry an update: k - lag >= F + n - 1, F the last restart at or before k"""
    starts = sorted(set(resets) | {0})
    return [k for k in range(n_steps) if k - lag >= max(t for t in starts if t <= k) + n - 1]
