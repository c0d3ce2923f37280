"""The members' glue launch (pdec_population_glue: the member prologue of step_glue_kernel on a grid of M workgroups,
csrc/act.hip) driven through the C ABI on raw networks, traces and a row table the test writes -- no environment, no Population
object -- on actor shapes no shipped setup has (fp64 states, fp32 parameters throughout).

A sequence of five launches on M = 5 members with different counters, every one of them compared three ways:
  * with the solo pdec_step_glue on twin buffers (own traces, own halt flag, a clone of the actor), called with the arguments
    run.py would pass for the member's counters: actions, all four traces over their whole allocation and the halt word, bit
    for bit;
  * with the plain model of replay_ring_ref.py for the pushes (rings that start filled with a sentinel: every row of every
    trace is compared, the untouched ones included) and with a restatement of how run.py settles the counters for all 16 row slots;
  * with oracle.nn.policy_act and oracle.rng's normal draws for the actions: 1e-13 for fp64 states under promoted fp32 weights
    (test_acting_path_is_fp64_with_fp32_weights), noise_scale_cases.draw_tolerance on top for entries that carry noise.

  A  phase 0, no reward / done (the first step: PRE_ACT push only).  Members 0 and 1 have ustep + 1 <= start_steps (member 1
     exactly) and take the zero action, POP_NOISE stays; member 2 is the first count that acts.
  B  phase 0 with reward and done.  Member 1 now acts; member 2's done flag is set (halt raised, POP_NRT moves, nothing else, no
     PRE_ACT rows); member 3 was halted before the launch (nothing of its moves); member 4's two pushes wrap inside the launch
     (one column: they land on the last row of each ring).
  C  phase 0 with reward and done again: member 4's next pushes start behind the seams; member 2 is halted by now.
  D  phase 1, the time-out push: terminal = 1 on every pushed row of the members that are not halted; member 0's done flag
     raises its halt word.
  E  phase 2, the POST_EPISODE push of the final state with zero action rows: member 1 has POP_ACTIVE = 0 and pushes nothing,
     the halt words are ignored, no counter moves."""
import ctypes as C_

import numpy as np
import pytest

import replay_ring_ref as ref
from noise_scale_cases import draw_tolerance
from oracle import nn
from oracle import rng as orng

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

M, START_STEPS, ROW = 5, 5, 16
USTEP, NSA, NRT, NOISE, SAMPLE, HALT, ACTIVE, BPA, BPC, NOISE_AMP, LIMIT = range(11)
SENTINEL = dict(state=-777.0, action=555.0, reward=333.0, terminal=-9.0)
TRACES = ("state", "action", "reward", "terminal")
ACT = {"identity": nn.IDENT, "relu": nn.RELU, "tanh": nn.TANH}

# id: (actor dims, activations, cols, noise rows (None: every output))
SHAPES = {
    "one_layer": ((3, 1), ("identity",), 1, None),
    "ks22_control": ((1, 6, 1), ("relu", "tanh"), 8, None),
    "four_layers_memory_row": ((12, 20, 20, 20, 2), ("relu", "relu", "relu", "tanh"), 5, 1),
    "wide_many_trips": ((9, 70, 1), ("relu", "tanh"), 40, None),
}


def _wrapping_count(cols, cap, cap1):
    """the least n = n_rt = n_sa before launch A for which launch B's reward push (from n) and state push (from n + cols, behind
    A's) both run over the end of their rings -- with one column: both land on the last row"""
    def over(start, mod):
        return start == mod - 1 if cols == 1 else mod - cols < start < mod
    for n in range(cap + 1, 4 * cap * cap1):
        if over(n % cap, cap) and over((n + cols) % cap1, cap1):
            return n
    raise AssertionError("no such count")


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


def expect_rows(rows, phase, has_r, done, cols, na):
    """the row table one launch later, as run.py settles a solo run's counters: nothing moves once the halt word is up; the
    reward push of the step that ends the episode counts and raises it, the rest of that step does not; the zero action of the
    start policy draws no noise; the time-out push moves POP_NRT only; the POST_EPISODE push moves nothing"""
    r = rows.copy()
    if phase == 2:
        return r
    for m in range(M):
        if r[m, HALT] & 0xFFFFFFFF:
            continue
        ended = bool(has_r and done[m] != 0)
        if has_r:
            r[m, NRT] += cols
        if ended:
            r[m, HALT] = (r[m, HALT] & ~0xFFFFFFFF) | 1
        if phase == 0 and not ended:
            if r[m, USTEP] + 1 > START_STEPS:
                r[m, NOISE] += (cols * na + 3) // 4
            r[m, USTEP] += 1
            r[m, NSA] += cols
    return r


class Glue:
    def __init__(self, pkg, shape):
        dims, acts, cols, nrows = SHAPES[shape]
        self.pkg, self.L = pkg, pkg._lib
        self.dims, self.acts, self.cols = list(dims), [ACT[a] for a in acts], cols
        self.ns, self.na = dims[0], dims[-1]
        self.nrows = self.na if nrows is None else nrows
        self.cap, self.stride = 4 * cols + 3, cols
        self.cap1 = self.cap + self.stride
        self.rng = rng = np.random.default_rng([len(dims), cols])
        kw = dict(dtype=torch.float32, device="cuda:0")
        L = self.L
        self.f64 = L.dtype_code(torch.float64)
        self.nets, self.twins, self.params = [], [], []
        for m in range(M):
            PA = nn.glorot_uniform(rng, self.dims, np.float64)
            for i in range(1, len(PA), 2):
                PA[i] = rng.standard_normal(PA[i].shape) * 0.1
            dc = [self.ns + self.na, 8, 1]
            PC = nn.glorot_uniform(rng, dc, np.float64)
            four = [pkg.HipMLP(self.dims, list(acts), PA, dtype=torch.float32, max_cols=cols),
                    pkg.HipMLP(dc, ["relu", None], PC, dtype=torch.float32, max_cols=cols),
                    pkg.HipMLP(self.dims, list(acts), PA, dtype=torch.float32, max_cols=cols),
                    pkg.HipMLP(dc, ["relu", None], PC, dtype=torch.float32, max_cols=cols)]
            twin = pkg.HipMLP(self.dims, list(acts), PA, dtype=torch.float32, max_cols=cols)
            for net in (four[0], twin):
                L.check(net.lib.pdec_mlp_set_noise_rows(net.handle, self.nrows))
            self.nets.append(four)
            self.twins.append(twin)
            self.params.append(four[0].params())        # (the fp32 values the kernel promotes)
        self.lib = lib = self.nets[0][0].lib

        def rings():
            return dict(state=torch.full((self.cap1, self.ns), SENTINEL["state"], **kw),
                        action=torch.full((self.cap1, self.na), SENTINEL["action"], **kw),
                        reward=torch.full((self.cap,), SENTINEL["reward"], **kw),
                        terminal=torch.full((self.cap,), SENTINEL["terminal"], **kw))
        self.traces = [rings() for _ in range(M)]
        self.twin_traces = [rings() for _ in range(M)]
        self.twin_halt = torch.zeros(M, dtype=torch.int32, device="cuda:0")
        self.noise_seed = [4000 + m for m in range(M)]
        # the rows before launch A
        n4 = _wrapping_count(cols, self.cap, self.cap1)
        counts = [0, 2 * cols, self.cap + 3, 7, n4]
        rows = np.zeros((M, ROW), dtype=np.int64)
        rows[:, USTEP] = [2, START_STEPS - 1, START_STEPS, 9, 20]
        rows[:, NSA] = rows[:, NRT] = counts
        rows[:, NOISE] = [11, 12, 13, (1 << 33) + 5, 15]
        rows[:, SAMPLE] = [21, 22, 23, 24, 25]
        rows[:, ACTIVE] = 1
        rows[:, [BPA, BPC]] = [[0, 1], [1, 0], [0, 0], [1, 1], [0, 1]]         # (not the glue's: must stay)
        rows[:, NOISE_AMP] = _bits([0.3, 0.1, 0.2, 0.15, 0.25])
        rows[:, LIMIT] = _bits([1.0, 1.0, 0.05, 1.0, 0.5])                       # member 2 clamps most of its actions
        rows[:, 11:16] = rng.integers(1, 2 ** 40, size=(M, 5))                   # (slots the glue must not touch)
        self.rows = rows
        self.models = []
        for m in range(M):
            mod = ref.Replay(self.ns, self.na)
            mod.s, mod.a = [ref.HOLE] * counts[m], [ref.HOLE] * counts[m]
            mod.r, mod.t = [ref.HOLE] * counts[m], [ref.HOLE] * counts[m]
            mod.n_sa = mod.n_rt = counts[m]
            mod.set_halt(0)
            self.models.append(mod)
        served = C_.c_int(0)
        A0 = self.nets[0][0]
        L.check(lib.pdec_step_glue_served(A0.handle, A0.handle, self.f64, 1, cols, cols, C_.byref(served)))
        assert served.value == 1
        H = L.Handle * M
        hs = [H(*[int(getattr(four[k].handle, "value", four[k].handle)) for four in self.nets]) for k in range(4)]
        tr = (C_.c_void_p * (4 * M))(*[t[k].data_ptr() for t in self.traces for k in TRACES])
        seeds = (C_.c_uint64 * (2 * M))(*[s for m in range(M) for s in (self.noise_seed[m], 5000 + m)])
        self.losses = torch.zeros((M, 2), **kw)
        losses = (C_.c_void_p * M)(*[self.losses[m].data_ptr() for m in range(M)])
        self.rows_dev = torch.zeros((M, ROW), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        self.h = L.Handle()
        L.check(lib.pdec_population_create(C_.byref(self.h), M, hs[0], hs[1], hs[2], hs[3], tr, seeds, losses, self.f64, cols, self.cap,
                                           self.stride, 1, 1, 0.99, 0.995, 0, 5e-4, 1e-3, self.stride, 1, START_STEPS,
                                           L.ptr(self.rows_dev)))
        self.upload()

    def upload(self):
        self.rows_dev.copy_(torch.from_numpy(self.rows))
        torch.cuda.synchronize()

    def close(self):
        torch.cuda.synchronize()
        for t in self.twins:
            self.L.check(self.lib.pdec_set_episode_halt(t.handle, None))
        self.lib.pdec_destroy(self.h)
        for four in self.nets:
            for n in four:
                n.close()
        for t in self.twins:
            t.close()

    # ---- one launch, all comparisons
    def launch(self, tag, phase, with_r=True, done=None):
        L, lib, cols, ns, na, rng = self.L, self.lib, self.cols, self.ns, self.na, self.rng
        P = L.ptr
        has_r = phase != 2 and with_r
        done = np.zeros(M, dtype=np.int32) if done is None else np.asarray(done, dtype=np.int32)
        state_h = rng.standard_normal((M, cols, ns))
        r_h = -rng.uniform(0.1, 1.0, (M, cols))
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")      # noqa: E731
        state, r, flags = dev(state_h), dev(r_h), dev(done)
        out = torch.full((M, cols, na), 7.0, dtype=torch.float64, device="cuda:0")
        out_twin = torch.full((M, cols, na), 7.0, dtype=torch.float64, device="cuda:0")
        before = self.rows.copy()
        self.twin_halt.copy_(dev((before[:, HALT] & 0xFFFFFFFF).astype(np.int32)))
        torch.cuda.synchronize()
        L.check(lib.pdec_population_glue(self.h, phase, P(r) if has_r else None, P(flags) if has_r else None,
                                         P(state) if phase != 1 else None, P(out) if phase == 0 else None))
        torch.cuda.synchronize()
        got = self.rows_dev.cpu().numpy().copy()
        want = expect_rows(before, phase, has_r, done, cols, na)
        # ---- the solo call on the twin buffers, member by member, from the counters the member's row held
        served = C_.c_int(0)
        for m in range(M):
            tw, tt = self.twins[m], self.twin_traces[m]
            row = before[m]
            if phase == 2 and not row[ACTIVE]:
                continue
            L.check(lib.pdec_set_episode_halt(tw.handle, None if phase == 2 else P(self.twin_halt[m:m + 1])))
            acting = row[USTEP] + 1 > START_STEPS
            n_rt = cols if has_r else 0
            n_sa = 0 if phase == 1 else cols
            L.check(lib.pdec_step_glue(
                tw.handle, tw.handle, self.f64, P(r[m]) if has_r else None, P(flags[m:m + 1]) if has_r else None, cols, int(phase == 1),
                P(tt["reward"]), P(tt["terminal"]), self.cap, int(row[NRT] % self.cap), n_rt,
                (1 if acting else 2) if phase == 0 else 0, P(state[m]) if phase != 1 else None, cols,
                float(row[NOISE_AMP:NOISE_AMP + 1].view(np.float64)[0]), float(row[LIMIT:LIMIT + 1].view(np.float64)[0]),
                self.noise_seed[m], int(row[NOISE]), P(out_twin[m]) if phase == 0 else None, P(tt["state"]), P(tt["action"]),
                self.cap1, int(row[NSA] % self.cap1), n_sa, L.Handle(0), C_.byref(served)))
            assert served.value == 1, (tag, m)
        torch.cuda.synchronize()
        # ---- rows: all 16 slots of every member
        for m in range(M):
            assert np.array_equal(got[m], want[m]), (tag, m, np.flatnonzero(got[m] != want[m]).tolist(), got[m], want[m])
        self.rows = got
        assert np.array_equal(self.twin_halt.cpu().numpy(), (got[:, HALT] & 0xFFFFFFFF).astype(np.int32)) or phase == 2, tag
        # ---- actions: the twin's bit for bit, the oracle's within the acting path's tolerance
        acts_h = out.cpu().numpy()
        assert acts_h.tobytes() == out_twin.cpu().numpy().tobytes(), tag
        if phase == 0:
            for m in range(M):
                row = before[m]
                if not row[USTEP] + 1 > START_STEPS:
                    assert not acts_h[m].any() and not np.signbit(acts_h[m]).any(), (tag, m)
                    continue
                amp, lim = row[NOISE_AMP:NOISE_AMP + 1].view(np.float64)[0], row[LIMIT:LIMIT + 1].view(np.float64)[0]
                greedy = nn.forward([p.astype(np.float64) for p in self.params[m]], self.acts, state_h[m].T)      # [na, cols]
                z = orng.randn(self.noise_seed[m], int(row[NOISE]), cols * na).reshape(cols, na).T              # element c * na + f
                z[self.nrows:] = 0.0
                ref_a = nn.policy_act(self.params[m], self.acts, state_h[m].T, z, amp, lim, learning=True, memory_size=na - self.nrows)
                tol = 1e-13 + np.where(z != 0.0, draw_tolerance(greedy, amp, z, "f64"), 0.0)
                err = np.abs(acts_h[m].T - ref_a)
                assert (err <= tol).all(), (tag, m, float((err / tol).max()))
                assert np.abs(acts_h[m]).max() <= lim and not (acts_h[m] == 7.0).any()
                if self.nrows < na:             # the memory row carries no noise: it is the greedy action, clamped
                    assert (np.abs(acts_h[m].T[self.nrows:] - np.clip(greedy[self.nrows:], -lim, lim)) <= 1e-13).all(), (tag, m)
                assert (np.abs(amp * z[:self.nrows]) > 1e3 * tol[:self.nrows]).all()       # (the bound does tell noise from none)
        else:
            assert (acts_h == 7.0).all(), tag
        # ---- pushes: the model's image over the whole allocation, and the twin's traces bit for bit
        for m in range(M):
            mod, row = self.models[m], before[m]
            mod.set_halt(int(row[HALT] & 0xFFFFFFFF))         # (the test may have raised it between two launches)
            if phase == 2:
                if row[ACTIVE]:
                    keep = mod.halt
                    mod.set_halt(0)
                    mod.push_sa(state_h[m], None)
                    mod.set_halt(keep)
            elif not mod.halt:
                if has_r:
                    mod.push_rt(r_h[m], done[m:m + 1], cols, int(phase == 1))
                if phase == 0 and not mod.halt:
                    mod.push_sa(state_h[m], acts_h[m])
                assert (mod.n_sa, mod.n_rt) == (got[m, NSA], got[m, NRT]), (tag, m)
            assert int(mod.halt) == int(got[m, HALT] & 0xFFFFFFFF), (tag, m)
            image = mod.image(self.cap, self.stride, init={k: np.full(tuple(self.traces[m][k].shape), SENTINEL[k], np.float32)
                                                           for k in TRACES})
            for k in TRACES:
                mine, twin = self.traces[m][k].cpu().numpy(), self.twin_traces[m][k].cpu().numpy()
                assert np.array_equal(mine, image[k]), (tag, m, k)
                assert mine.tobytes() == twin.tobytes(), (tag, m, k, "solo twin")
        return before, got


@pytest.mark.parametrize("shape", list(SHAPES))
def test_member_glue_equals_solo_twins_model_and_oracle(pkg, shape):
    G = Glue(pkg, shape)
    try:
        cols, cap, cap1 = G.cols, G.cap, G.cap1
        # A: the first step
        b, a = G.launch("A", 0, with_r=False)
        assert (a[:, NOISE] - b[:, NOISE]).tolist() == [0, 0] + [(cols * G.na + 3) // 4] * 3
        assert (a[:, USTEP] - b[:, USTEP]).tolist() == [1] * M and (a[:, NSA] - b[:, NSA]).tolist() == [cols] * M
        assert np.array_equal(a[:, NRT], b[:, NRT])
        # B: member 2's episode ends here, member 3 is halted already, member 4 wraps both rings
        G.rows[3, HALT] = 1
        G.upload()
        start_rt, start_sa = int(G.rows[4, NRT] % cap), int(G.rows[4, NSA] % cap1)
        assert (start_rt + cols > cap and start_sa + cols > cap1) if cols > 1 else (start_rt == cap - 1 and start_sa == cap1 - 1)
        assert G.rows[4, NRT] > cap and G.rows[0, NRT] < cap                # a wrapped ring beside one that has not
        b, a = G.launch("B", 0, done=[0, 0, 1, 1, 0])
        d = a - b
        assert d[2].nonzero()[0].tolist() == [NRT, HALT] and d[2, NRT] == cols and a[2, HALT] == 1
        assert not d[3].any()
        assert d[1, NOISE] == (cols * G.na + 3) // 4 and d[0, NOISE] == 0      # member 1 acts from this step on
        # C: behind the seams
        assert int(G.rows[4, NRT] % cap) < cols and int(G.rows[4, NSA] % cap1) < cols
        b, a = G.launch("C", 0)
        assert not (a - b)[2].any() and not (a - b)[3].any()
        # D: the time-out push; member 0's done flag raises its halt word
        b, a = G.launch("D", 1, done=[1, 0, 0, 0, 0])
        d = a - b
        assert d[:, NRT].tolist() == [cols, cols, 0, 0, cols] and a[:, HALT].tolist() == [1, 0, 1, 1, 0]
        d[:, [NRT, HALT]] = 0
        assert not d.any()
        for m in (0, 1, 4):                     # terminal = 1 on the rows this launch pushed
            at = (int(b[m, NRT]) + np.arange(cols)) % cap
            assert (G.traces[m]["terminal"].cpu().numpy()[at] == 1.0).all(), m
        # E: the POST_EPISODE push
        G.rows[1, ACTIVE] = 0
        G.upload()
        b, a = G.launch("E", 2)
        assert np.array_equal(a, b)
        for m in range(M):
            at = (int(b[m, NSA]) + np.arange(cols)) % cap1
            rows_a = G.traces[m]["action"].cpu().numpy()[at]
            assert (rows_a == 0.0).all() if m != 1 else not (rows_a == 0.0).all(), m      # halted members 0, 2, 3 pushed too
    finally:
        G.close()
