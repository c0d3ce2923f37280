"""NumPy restatement of the episode clock (csrc/episode_clock.hip; include/pdeconv.h: pdec_epclock_step) -- test infrastructure,
host only.  Rule per trajectory b of one boundary call behind an env step, in this order (E = episode_steps, C = capacity):

  1. blew = flags[b] != 0; where blew, non-finite entries of reward row b become 0; other rows are left alone
  2. ret[b] += (sum_a (double) r[b][a]) / R, summed in a order, on the sanitised row
  3. clock[b]++, len[b]++, total[b]++; ends = blew or clock[b] == E
  4. not ended: action_prev_next[b] = action[b]; nothing else of b is written
  5. ended: terminal row b = 1; log slot count[b] % C <- (ret[b], len[b], blew, total[b]); count[b]++; ret[b] = 0;
     clock[b] = len[b] = 0; action_prev_next[b] = 0; y_next[b] <- the new field, state_next[b] <- its features in reset form

The new field of a restart is row b of a fixed (y0, state0) pair or, with random initial fields, row b of the draw at Philox
offset init_offset(n, r, W, B, nc) with n = count[b] after the increment."""
import numpy as np


def initial_clocks(B, E, stagger):
    """the clocks TrainPipeline(episodes="per_trajectory", stagger=...) starts from: floor(b E / B), or zeros"""
    return np.array([(b * E) // B if stagger else 0 for b in range(B)], dtype=np.int32)


def init_offset(n, rank, world, B, nc):
    """Philox offset of the draw that holds episode n of the B trajectories of rank `rank` of `world`; nc sine coefficients
    (one uniform each, four per counter) per trajectory.  Trajectory b takes the counters off + b ceil(nc / 4) onwards."""
    return (n * world + rank) * B * ((nc + 3) // 4)


class ClockModel:
    def __init__(self, B, E, capacity, clock0=None):
        self.B, self.E, self.C = int(B), int(E), int(capacity)
        self.count = np.zeros(B, dtype=np.int64)
        self.total = np.zeros(B, dtype=np.int64)
        self.slots = [dict() for _ in range(B)]            # slot -> (ret, len, blew, total, episode)
        self.clock0 = np.zeros(B, dtype=np.int32) if clock0 is None else np.asarray(clock0, dtype=np.int32).copy()
        self.set()

    def set(self, clock0=None):
        """pdec_epclock_set: the clocks to clock0 (None: the values given at construction), len and ret to 0"""
        if clock0 is not None:
            self.clock0 = np.asarray(clock0, dtype=np.int32).copy()
        self.clock = self.clock0.copy()
        self.len = np.zeros(self.B, dtype=np.int32)
        self.ret = np.zeros(self.B)

    def step(self, reward, flags):
        """rules 1 - 3 and the bookkeeping of 5.  reward [B, R] in the environment's dtype, flags [B].
        Returns (the sanitised reward, ended [B] bool, n [B]: count[b] after the increment where ended)"""
        r = np.array(reward, copy=True)
        blew = np.asarray(flags) != 0
        for b in np.nonzero(blew)[0]:
            row = r[b]
            row[~np.isfinite(row)] = 0
        s = np.zeros(self.B)
        with np.errstate(invalid="ignore", over="ignore"):
            for a in range(r.shape[1]):
                s = s + r[:, a].astype(np.float64)
            ret = self.ret + s / float(r.shape[1])
        self.clock += 1
        self.len += 1
        self.total += 1
        ended = blew | (self.clock == self.E)
        self.ret = np.where(ended, 0.0, ret)
        for b in np.nonzero(ended)[0]:
            n = int(self.count[b])
            self.slots[b][n % self.C] = (ret[b], int(self.len[b]), bool(blew[b]), int(self.total[b]), n)
            self.count[b] += 1
        self.clock[ended] = 0
        self.len[ended] = 0
        return r, ended, np.where(ended, self.count, 0)

    def finished(self):
        """what TrainPipeline.finished_episodes() returns: flat arrays sorted by (end_step, trajectory), and dropped"""
        rows = sorted((v[3], b, v[4], v[0], v[1], v[2]) for b in range(self.B) for v in self.slots[b].values())
        col = lambda i, dt: np.array([x[i] for x in rows], dtype=dt)
        return dict(trajectory=col(1, np.int64), episode=col(2, np.int64), ret=col(3, np.float64), length=col(4, np.int32),
                    blew_up=col(5, bool), end_step=col(0, np.int64), dropped=int(np.maximum(self.count - self.C, 0).sum()))

    def rings(self):
        """what pdec_epclock_read returns besides the counts: [B, C] arrays (slots never written: 0)"""
        ret, ln = np.zeros((self.B, self.C)), np.zeros((self.B, self.C), dtype=np.int32)
        blew, end = np.zeros((self.B, self.C), dtype=np.int32), np.zeros((self.B, self.C), dtype=np.int64)
        for b in range(self.B):
            for sl, v in self.slots[b].items():
                ret[b, sl], ln[b, sl], blew[b, sl], end[b, sl] = v[0], v[1], int(v[2]), v[3]
        return ret, ln, blew, end


def apply_rows(ended, terminal, action, action_prev_next, y_next, state_next, new_y, new_state):
    """rules 4 and 5 on host copies of the arrays (modified in place): new_y / new_state hold the restart rows of the ended
    trajectories at their own index b (other rows are not read)"""
    for b in range(len(ended)):
        if ended[b]:
            terminal[b] = 1
            action_prev_next[b] = 0
            y_next[b] = new_y[b]
            state_next[b] = new_state[b]
        else:
            action_prev_next[b] = action[b]
