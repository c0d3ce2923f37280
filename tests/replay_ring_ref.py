"""A plain model of the device replay (csrc/replay.hip: replay_push2_kernel, replay_push_rt_kernel, replay_sample_kernel; the same
pushes inside csrc/act.hip's step_glue_kernel; the slot table of csrc/small_args.hpp) that holds NO ring.  numpy only.

Four lists indexed by LOGICAL entry number -- state, action (one entry per pushed row) and reward, terminal -- and two counters,
n_sa and n_rt, that move as the host's do (agent.py: CircularArraySARTTrajectory).  What a physical trace must hold is derived
afterwards (`image`): physical row p holds the newest logical entry l with l % modulus == p, modulus = cap + stride for state /
action and cap for reward / terminal; a row never written keeps what it held before (zero, or the caller's sentinel).  pop_sa
lowers n_sa, and the next push writes over the popped entries: the later write wins, and a popped entry that nothing wrote over
is still in its row.

The halt flag follows replay.hip: None = none attached; once it is 1 nothing is pushed -- the host's counters still move, the
rows keep what they held (HOLE) -- ; the rt push of the step that ends the episode still happens and raises it; done[0] decides.

`batch` gathers s, a, r, t, s' from the logical lists (s' = logical lg + stride), `gather` from an image through physical slots as
a kernel does: that the two agree is the alignment claim of CircularArraySARTTrajectory's docstring (reference quirks).
The index draw is oracle.rng's (sample_slots / words), not restated here.

fault=...: one mistake built in, as tests/test_pipeline_reference.py's simulate() does; test_replay_ring_table.py names the
comparison that rejects each one."""
import numpy as np

from oracle import rng as orng

HOLE = None
FAULTS = ("sn_modulo_cap", "base_omitted", "flag_per_column", "dummy_not_popped", "truncated_at_seam", "index_by_remainder")
F32 = np.float32


class Replay:
    def __init__(self, ns, na, fault=None):
        assert fault is None or fault in FAULTS, fault
        self.ns, self.na, self.fault = int(ns), int(na), fault
        self.s, self.a, self.r, self.t = [], [], [], []
        self.n_sa = self.n_rt = 0
        self.halt = None
        self.pushes = {"sa": [], "rt": []}          # (first logical entry, rows) of every push that wrote

    # ---- operations
    def set_halt(self, value):
        self.halt = None if value is None else int(value)

    @staticmethod
    def _store(lst, at, value):
        if at < len(lst):
            if value is not HOLE:
                lst[at] = value
        else:
            assert at == len(lst)
            lst.append(value)

    def push_sa(self, s, a=None):
        s = np.asarray(s)
        n = s.shape[0]
        assert s.shape == (n, self.ns) and (a is None or np.asarray(a).shape == (n, self.na))
        if n == 0:
            return
        up = bool(self.halt)
        if not up:
            self.pushes["sa"].append((self.n_sa, n))
        for i in range(n):
            self._store(self.s, self.n_sa + i, HOLE if up else s[i].astype(F32))
            self._store(self.a, self.n_sa + i, HOLE if up else (np.zeros(self.na, F32) if a is None else np.asarray(a)[i].astype(F32)))
        self.n_sa += n

    def pop_sa(self, n):
        if self.fault != "dummy_not_popped":
            self.n_sa -= n
        assert self.n_sa >= 0

    def push_rt(self, r, done_flags=None, cols_per_traj=1, force=0):
        r = np.asarray(r)
        n = r.shape[0]
        if n == 0:
            return
        up = bool(self.halt)
        if not up:
            self.pushes["rt"].append((self.n_rt, n))
        for i in range(n):
            if done_flags is None:
                flag = 0
            elif self.fault == "flag_per_column":
                flag = done_flags[i % len(done_flags)]
            else:
                flag = done_flags[i // cols_per_traj]
            self._store(self.r, self.n_rt + i, HOLE if up else r[i].astype(F32))
            self._store(self.t, self.n_rt + i, HOLE if up else F32(1.0 if (force or flag != 0) else 0.0))
        self.n_rt += n
        if self.halt is not None and not up and done_flags is not None and done_flags[0] != 0:
            self.halt = 1

    # ---- what the device arrays must hold
    def _written(self, which, modulus):
        """logical entries that reached their row (all of them; fault: the part of a push beyond the seam is lost)"""
        if self.fault != "truncated_at_seam":
            return None
        keep = set()
        for first, n in self.pushes[which]:
            keep.update(l for l in range(first, first + n) if (first % modulus) + (l - first) < modulus)
        return keep

    def image(self, cap, stride, init=None):
        """{state [cap + stride, ns], action [cap + stride, na], reward [cap], terminal [cap]} in float32; init: what the arrays
        held before the first push (default zeros)"""
        cap1 = cap + stride
        shapes = dict(state=(cap1, self.ns), action=(cap1, self.na), reward=(cap,), terminal=(cap,))
        out = {k: (np.zeros(sh, F32) if init is None else np.array(init[k], dtype=F32).reshape(sh)) for k, sh in shapes.items()}
        for key, lst, mod, which in (("state", self.s, cap1, "sa"), ("action", self.a, cap1, "sa"), ("reward", self.r, cap, "rt"),
                                     ("terminal", self.t, cap, "rt")):
            keep = self._written(which, mod)
            for l, v in enumerate(lst):                # rising l: the newest entry of a row comes last
                if v is not HOLE and (keep is None or l in keep):
                    out[key][l % mod] = v
        return out

    # ---- sampling
    def n_valid(self, cap):
        return min(self.n_rt, cap)

    def slots(self, seed, offset, count, cap, stride):
        """int64 [3, count]: the physical slots of (s, a), of (r, t) and of s' of `count` draws from the stream (seed, offset)"""
        nv = self.n_valid(cap)
        n_rt = nv if self.fault == "base_omitted" else self.n_rt
        sl = orng.sample_slots(seed, offset, count, nv, n_rt, cap, stride)
        if self.fault == "index_by_remainder":
            ind = (orng.words(seed, offset, count).astype(np.uint64) % np.uint64(nv - stride)).astype(np.int64)
            lg = max(0, self.n_rt - cap) + ind
            sl = np.stack([lg % (cap + stride), lg % cap, (lg + stride) % (cap + stride)])
        if self.fault == "sn_modulo_cap":
            sl = np.stack([sl[0], sl[1], (self.logical(sl[1], cap) + stride) % cap])
        return sl

    def logical(self, slots_rt, cap):
        """the logical entry behind a slot of the reward ring: the one entry of [base, base + cap) with that remainder"""
        base = max(0, self.n_rt - cap)
        return base + (np.asarray(slots_rt, dtype=np.int64) - base) % cap

    def batch(self, slots, cap, stride):
        """(s [n, ns], a [n, na], r [n], t [n], s' [n, ns]) of the logical entries behind `slots`, from the lists"""
        lg = self.logical(np.asarray(slots)[1], cap)
        assert lg.max() + stride < self.n_sa + (0 if self.fault is None else 10 ** 9) and lg.max() < self.n_rt
        pick = lambda lst, idx, w: np.array([lst[i] for i in idx], dtype=F32).reshape((len(idx),) + w)
        return (pick(self.s, lg, (self.ns,)), pick(self.a, lg, (self.na,)), pick(self.r, lg, ()), pick(self.t, lg, ()),
                pick(self.s, lg + stride, (self.ns,)))


def gather(image, slots):
    """the five batch arrays read out of physical traces through physical slots: what replay_sample_kernel does"""
    i_s, i_rt, i_sn = (np.asarray(v, dtype=np.int64) for v in slots)
    return image["state"][i_s], image["action"][i_s], image["reward"][i_rt], image["terminal"][i_rt], image["state"][i_sn]


BATCH_NAMES = ("state", "action", "reward", "terminal", "next_state")
