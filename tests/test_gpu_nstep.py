"""GPU tests of the n-step object alone (csrc/nstep.hip: pdec_nstep_create / _step / _read), without an environment: synthetic rows
fed from rotating input buffers of 6 (state) and 3 (action, reward, terminal) slots into rotating outputs of 3 slots, as the pipeline
does, every output compared EXACTLY with the ring-free NumPy model of tests/nstep_ref.py, in fp32 and fp64; and the same sequence
enqueued through pdec_capture_begin / _end in chunks of 6 and replayed."""
import ctypes as C

import numpy as np
import pytest
import torch

from nstep_ref import NStepModel, window_lengths

pytestmark = pytest.mark.gpu

GAMMA = 0.99
DT = {"f32": (torch.float32, np.float32), "f64": (torch.float64, np.float64)}
PATTERNS = ("none", "every7", "every2", "two_in_a_window", "oldest_row", "random20")


def _flags(pattern, K, cols, n, rng):
    t = np.zeros((K, cols))
    if pattern == "every7":
        t[6::7] = 1
    elif pattern == "every2":                          # E = 2 < n for n >= 3
        t[1::2] = 1
    elif pattern == "two_in_a_window":                 # adjacent (even columns) and at both ends of a window (odd columns)
        k0 = n + 2
        t[k0, :] = 1
        t[k0 + 1, 0::2] = 1
        t[k0 + max(1, n - 1), 1::2] = 1
    elif pattern == "oldest_row":                      # a lone terminal: it is the window's oldest row n - 1 steps later
        t[n + 3, 0::3] = 1
        t[K - n, 1::3] = 1                             # ... in the very last call
    elif pattern == "random20":
        t = (rng.random((K, cols)) < 0.2).astype(np.float64)
    return t


def _rows(K, cols, ns, na, npdt, t, rng):
    return [(rng.normal(size=(cols, ns)).astype(npdt), rng.normal(size=(cols, na)).astype(npdt),
             (3.0 * rng.normal(size=cols)).astype(npdt), t[k].astype(npdt)) for k in range(K)]


class _Obj:
    def __init__(self, pkg, n, cols, ns, na, tdt, stream):
        self.L = L = pkg._lib
        self.lib = L.init(0)
        self.h = L.Handle()
        L.check(self.lib.pdec_nstep_create(C.byref(self.h), n, cols, ns, na, L.dtype_code(tdt)))
        L.check(self.lib.pdec_set_stream(self.h, C.c_void_p(stream.cuda_stream)))

    def step(self, s, a, r, t, so, ao, ro, to, gamma=GAMMA):
        p = self.L.ptr
        self.L.check(self.lib.pdec_nstep_step(self.h, p(s), p(a), p(r), p(t), gamma, p(so), p(ao), p(ro), p(to)))

    def close(self):
        self.lib.pdec_destroy(self.h)


def _buffers(cols, ns, na, tdt, slots=(6, 3, 3, 3)):
    kw = dict(dtype=tdt, device="cuda:0")
    shapes = ((cols, ns), (cols, na), (cols,), (cols,))
    return [[torch.zeros(sh, **kw) for _ in range(k)] for sh, k in zip(shapes, slots)]


def _eager(pkg, n, cols, ns, na, tdt, rows, gamma=GAMMA):
    """every step's four outputs (host copies), the ring position and the rings"""
    st = torch.cuda.Stream()
    o = _Obj(pkg, n, cols, ns, na, tdt, st)
    ins, outs = _buffers(cols, ns, na, tdt), _buffers(cols, ns, na, tdt, (3, 3, 3, 3))
    got = []
    for k, row in enumerate(rows):
        with torch.cuda.stream(st):
            src = [b[k % len(b)] for b in ins]
            for d, x in zip(src, row):
                d.copy_(torch.as_tensor(x))
            dst = [b[k % 3] for b in outs]
            o.step(*src, *dst, gamma=gamma)
        st.synchronize()
        got.append([d.cpu().numpy() for d in dst])
    pos = C.c_int64()
    npdt = rows[0][0].dtype
    rings = [np.empty((n,) + x.shape, npdt) for x in rows[0]]
    o.L.check(o.lib.pdec_nstep_read(o.h, C.byref(pos), *[o.L.ptr(r) for r in rings]))
    o.close()
    return got, int(pos.value), rings


def _check(n, rows, got, gamma=GAMMA):
    mdl = NStepModel(n, gamma)
    for k, row in enumerate(rows):
        want = mdl.push(*row)
        if k < n - 1:
            continue                                   # windows that reach back before step 0: not consumed
        for name, g in zip(("state", "action", "reward", "terminal"), got[k]):
            assert g.dtype == want[name].dtype
            assert np.array_equal(g, want[name], equal_nan=True), (name, k)
    return mdl


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("ns,na", [(1, 1), (10, 3)])
@pytest.mark.parametrize("cols", [15, 64, 200])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_step_matches_the_model_exactly(pkg, n, cols, ns, na, prec):
    tdt, npdt = DT[prec]
    K = 2 * n + 13
    for i, pattern in enumerate(PATTERNS):
        rng = np.random.default_rng(1000 * n + cols + i)
        t = _flags(pattern, K, cols, n, rng)
        rows = _rows(K, cols, ns, na, npdt, t, rng)
        got, pos, rings = _eager(pkg, n, cols, ns, na, tdt, rows)
        mdl = _check(n, rows, got)
        assert pos == K, pattern
        for g, w in zip(rings, mdl.ring()):
            assert np.array_equal(g, w), pattern
        if pattern == "two_in_a_window" and n >= 2:
            # some window held two terminals and was cut at the first
            assert any(((t[k - n + 1:k + 1] != 0).sum(axis=0) >= 2).any() for k in range(n - 1, K))
        if pattern == "oldest_row" and n >= 2:
            assert any((window_lengths(t[k - n + 1:k + 1]) == 0).any() for k in range(n - 1, K))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_a_non_finite_reward_reaches_the_windows_that_hold_it_before_their_first_terminal(pkg, prec):
    tdt, npdt = DT[prec]
    n, cols, K = 3, 64, 2 * 3 + 13
    rng = np.random.default_rng(5)
    t = np.zeros((K, cols))
    t[7, 5] = 1          # column 5: a terminal right in front of the NaN of step 8
    t[12, 7] = 1         # column 7: the inf of step 12 IS the terminal row
    t[10, 9] = 1         # column 9: a terminal behind the NaN of step 9, inside its windows
    rows = _rows(K, cols, 1, 1, npdt, t, rng)
    bad = {(8, 5): np.nan, (12, 7): np.inf, (9, 9): np.nan, (15, 20): -np.inf}
    for (k, c), v in bad.items():
        rows[k][2][c] = v
    got, _pos, _rings = _eager(pkg, n, cols, 1, 1, tdt, rows)
    _check(n, rows, got)
    want = set()
    for k in range(n - 1, K):
        u = k - n + 1
        m = window_lengths(t[u:k + 1])
        want |= {(k, c) for (q, c) in bad if u <= q <= u + int(m[c])}
    seen = {(k, int(c)) for k in range(n - 1, K) for c in np.flatnonzero(~np.isfinite(got[k][2]))}
    assert seen == want
    # column 5: the windows that start at 6 and 7 end at the terminal of step 7 and stay finite; those that start at 8 do not
    assert (8, 5) not in seen and (9, 5) not in seen and (10, 5) in seen


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_captured_chunks_of_six_replay_the_eager_sequence(pkg, n, prec):
    """Library calls only inside the graph: two n = 1 objects play the env step's and the reader's parts -- the feeder copies the
    chunk's staged rows into the rotating input slots, the drain copies the rotating outputs to one result row per step (an n = 1
    call returns its input, which the eager test pins)."""
    tdt, npdt = DT[prec]
    cols, ns, na = 200, 10, 3
    K = 6 * ((2 * n + 13 + 5) // 6)
    rng = np.random.default_rng(77 + n)
    t = _flags("random20", K, cols, n, rng)
    rows = _rows(K, cols, ns, na, npdt, t, rng)
    want, want_pos, want_rings = _eager(pkg, n, cols, ns, na, tdt, rows)

    st = torch.cuda.Stream()
    L = pkg._lib
    obj, feed, drain = (_Obj(pkg, m, cols, ns, na, tdt, st) for m in (n, 1, 1))
    ins, outs = _buffers(cols, ns, na, tdt), _buffers(cols, ns, na, tdt, (3, 3, 3, 3))
    stage, res = _buffers(cols, ns, na, tdt, (6, 6, 6, 6)), _buffers(cols, ns, na, tdt, (6, 6, 6, 6))
    torch.cuda.synchronize()
    L.check(obj.lib.pdec_capture_begin(obj.h))
    try:
        for i in range(6):
            src, dst = [b[i % len(b)] for b in ins], [b[i % 3] for b in outs]
            feed.step(*[b[i] for b in stage], *src)
            obj.step(*src, *dst)
            drain.step(*dst, *[b[i] for b in res])
    finally:
        g = L.Handle()
        L.check(obj.lib.pdec_capture_end(obj.h, C.byref(g)))
    got = []
    for k0 in range(0, K, 6):
        for i in range(6):
            for d, x in zip([b[i] for b in stage], rows[k0 + i]):
                d.copy_(torch.as_tensor(x))
        torch.cuda.synchronize()
        L.check(obj.lib.pdec_graph_launch(g, None))
        st.synchronize()
        got += [[b[i].cpu().numpy() for b in res] for i in range(6)]
    for k in range(n - 1, K):
        for a, b in zip(got[k], want[k]):
            assert np.array_equal(a, b, equal_nan=True), k
    pos = C.c_int64()
    rings = [np.empty_like(r) for r in want_rings]
    L.check(obj.lib.pdec_nstep_read(obj.h, C.byref(pos), *[L.ptr(r) for r in rings]))
    assert int(pos.value) == want_pos == K
    for a, b in zip(rings, want_rings):
        assert np.array_equal(a, b)
    obj.lib.pdec_destroy(g)
    for o in (obj, feed, drain):
        o.close()


def test_create_refuses_by_name(pkg):
    L = pkg._lib
    lib = L.init(0)
    h = L.Handle()
    for n in (0, 33, -2):
        assert lib.pdec_nstep_create(C.byref(h), n, 64, 1, 1, L.PDEC_F32) != 0
        assert b"n_step" in lib.pdec_last_error() and b"1 .. 32" in lib.pdec_last_error()
    assert lib.pdec_nstep_create(C.byref(h), 3, 0, 1, 1, L.PDEC_F32) != 0
    assert lib.pdec_nstep_create(C.byref(h), 3, 64, 1, 1, 7) != 0 and b"dtype" in lib.pdec_last_error()
    assert lib.pdec_nstep_read(L.Handle(12345), None, None, None, None, None) != 0
