"""The case table of test_gpu_replay_ring.py (replay_ring_cases.py) against what it claims, and the plain model of the replay
(replay_ring_ref.py) against the host mirror.  Runs without a GPU: the edges are all there (computed from the rows), the draws of
every sampling row reach the seams of both rings, CircularArraySARTTrajectory's torch path equals the model on every row it can
express, and every deliberately wrong variant of the model is rejected by the comparison named for it -- the evidence that the GPU
test would notice the same mistake in a kernel."""
import sys

import numpy as np
import pytest

import replay_ring_cases as rc
import replay_ring_ref as ref
from oracle import rng as orng

torch = pytest.importorskip("torch")


def model_of(name, fault=None, row=None):
    row = row or rc.ROWS[name]
    return rc.play(name, ref.Replay(row.ns, row.na, fault=fault), row)


def image_of(name, m, row=None):
    row = row or rc.ROWS[name]
    return m.image(row.cap, row.stride, init=rc.sentinel(row) if row.prefill else None)


def pushes(name):
    """(kind, op, first physical row, modulus) of every push op of a row, from the counters of the model"""
    row = rc.ROWS[name]
    m = ref.Replay(row.ns, row.na)
    out = []
    for k, op in enumerate(row.ops):
        if op[0] in ("sa", "sa0"):
            out.append(("sa", op, m.n_sa % (row.cap + row.stride), row.cap + row.stride, m.halt))
        elif op[0] == "rt":
            out.append(("rt", op, m.n_rt % row.cap, row.cap, m.halt))
        _apply(name, k, op, row, m)
    return out


def _apply(name, k, op, row, m):
    """op k of a row on the model (what rc.play does, one op at a time)"""
    if op[0] in ("sa", "sa0"):
        m.push_sa(*rc.op_data(name, k, op, row))
    elif op[0] == "pop":
        m.pop_sa(op[1])
    elif op[0] == "halt":
        m.set_halt(op[1])
    else:
        _, n, flags, cols, force = op
        m.push_rt(rc.op_data(name, k, op, row)[0], None if flags is None else np.array(flags, dtype=np.int32), cols, force)


ALL_PUSHES = {name: pushes(name) for name in rc.ROWS}


def test_table_imports_without_torch_or_numpy():
    import os
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); import replay_ring_cases as rc; "
            "assert 'torch' not in sys.modules and 'numpy' not in sys.modules; print(len(rc.ROWS))") % os.path.dirname(rc.__file__)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == [str(len(rc.ROWS))]


def test_rows_are_well_formed():
    for name, row in rc.ROWS.items():
        assert row.cap >= 1 and row.stride >= 0 and row.ns >= 1 and row.na >= 1 and row.dtype in ("f32", "f64") and row.edge, name
        assert 4 <= row.cap <= 400, name                                 # a few rows to a few hundred
        for kind, op, start, mod, halt in ALL_PUSHES[name]:
            assert 0 <= op[1] <= mod, (name, op)                         # the library refuses n > capacity
            if kind == "rt":
                _, n, flags, cols, force = op
                assert cols >= 1 and (flags is None or len(flags) * cols >= n), (name, op)
                assert halt is None or n <= rc.BLOCK, (name, op)
        m = model_of(name)
        for seed, offset, Bu in row.samples:
            assert Bu >= 1 and 1 <= m.n_valid(row.cap) - row.stride and m.n_rt <= m.n_sa <= m.n_rt + max(row.stride, 0), (name, seed)
    assert len(rc.ROWS) == 31 and len(rc.sampling_rows()) == 9


def test_push_and_flag_and_halt_edges_are_all_there():
    P = [(name, rc.ROWS[name]) + p for name in rc.ROWS for p in ALL_PUSHES[name]]
    written = [p for p in P if not p[6] or p[6] == 0]
    for kind in ("sa", "rt"):
        K = [p for p in written if p[2] == kind and p[3][1] > 0]
        assert any(start + op[1] == mod for _, _, _, op, start, mod, _ in K), kind                 # ends exactly on the last row
        assert any(start == 0 and n > 0 for n, (_, _, _, op, start, mod, _) in ((p[3][1], p) for p in K))
        assert any(start == mod - 1 and op[1] > 1 for _, _, _, op, start, mod, _ in K), kind       # starts on the last row, wraps
        assert any(op[1] == mod and start != 0 for _, _, _, op, start, mod, _ in K), kind          # n == capacity, start != 0
    # the seam inside a push of rows wider than one feature
    wide = {row.ns for _, row, kind, op, start, mod, _ in written if kind == "sa" and start + op[1] > mod and 0 < start}
    assert {3, 8} <= wide
    elems = {op[1] * (row.ns + row.na) for _, row, kind, op, _, _, _ in written if kind == "sa"}
    assert {rc.BLOCK - 1, rc.BLOCK, rc.BLOCK + 1} <= elems and max(elems) > 2 * rc.BLOCK
    rts = {op[1] for _, _, kind, op, _, _, halt in P if kind == "rt" and halt is None}
    assert {rc.BLOCK - 1, rc.BLOCK, rc.BLOCK + 1} <= rts
    # both source dtypes, for either push, over more than one block
    for kind in ("sa", "rt"):
        big = {row.dtype for _, row, k, op, _, _, _ in written if k == kind and op[1] * ((row.ns + row.na) if k == "sa" else 1) > rc.BLOCK}
        assert big == {"f32", "f64"}, kind
    # a == NULL onto rows that held non-zero actions, in both dtypes
    dummies = set()
    for name, row in rc.ROWS.items():
        m = ref.Replay(row.ns, row.na)
        for k, op in enumerate(row.ops):
            if op[0] == "sa0" and op[1] and not m.halt:
                before = m.image(row.cap, row.stride)["action"]
                hit = [(m.n_sa + i) % (row.cap + row.stride) for i in range(op[1])]
                if all(np.all(before[h] != 0) for h in hit):
                    dummies.add(row.dtype)
            _apply(name, k, op, row, m)
    assert dummies == {"f32", "f64"}
    assert any(all(op[1] == 0 for op in row.ops) and row.prefill for row in rc.ROWS.values())       # n == 0
    shapes = {(row.ns, row.na) for row in rc.ROWS.values()}
    assert {(s, a) for s in (1, 3, 8) for a in (1, 2)} <= shapes
    assert {1, 3, 8} <= {row.stride for row in rc.ROWS.values() if not rc.expressible(row)}
    assert any(not rc.expressible(row) and row.cap % max(op[1], 1) for row in rc.ROWS.values() for op in row.ops if op[0] == "sa")
    # terminal flags
    rt = [(op, halt) for _, _, kind, op, _, _, halt in P if kind == "rt"]
    grid = {(op[3], len(op[2]), op[2]) for op, _ in rt if op[2] is not None and not op[4] and len(op[2]) * op[3] == op[1]}
    for cols in (1, 3, 8):
        for m_ in (1, 2, 5):
            for f in rc._patterns(m_):
                assert (cols, m_, f) in grid, (cols, m_, f)
    assert any(op[2] is None and not op[4] for op, _ in rt) and any(op[2] is None and op[4] for op, _ in rt)
    assert any(op[2] is not None and not any(op[2]) and op[4] for op, _ in rt)                     # force over a zero vector
    # halt
    ends = {}
    for name, row in rc.ROWS.items():
        if any(op[0] == "halt" for op in row.ops):
            assert row.prefill and not rc.expressible(row), name
            first = next(op for op in row.ops if op[0] == "rt")
            ends[name] = (row.ops[0][1], first[2], model_of(name).halt)
    assert (0, (0,), 0) in ends.values()                                  # down, no done
    assert any(v[0] == 0 and v[1][0] == 1 and v[2] == 1 for v in ends.values())                     # down, done[0]: raised
    assert any(v[0] == 0 and v[1][0] == 0 and any(v[1][1:]) and v[2] == 0 for v in ends.values())   # only done[1]: stays down
    assert any(v[0] == 1 for v in ends.values())                                                    # up
    m = model_of("halt_down_done0")
    assert m.halt == 1 and len(m.pushes["sa"]) == 1 and len(m.pushes["rt"]) == 1                    # the pushes behind it are skipped
    m = model_of("halt_up")
    assert not m.pushes["sa"] and not m.pushes["rt"]
    for a, b in zip(("state", "action", "reward", "terminal"), ("state", "action", "reward", "terminal")):
        assert np.array_equal(image_of("halt_up", m)[a], rc.sentinel(rc.ROWS["halt_up"])[b])
    assert {"rt_halt_more_than_one_block", "sa_n_above_capacity", "rt_n_above_capacity", "sample_nothing_valid",
            "sample_valid_above_capacity"} == set(rc.REFUSALS)


def test_sampling_edges_are_all_there():
    S = {n: (rc.ROWS[n], model_of(n)) for n in rc.sampling_rows()}
    st = {n: (r.stride, m.n_valid(r.cap), m.n_rt, m.n_sa, r.cap) for n, (r, m) in S.items()}
    assert any(s == 1 and nv == s + 1 for s, nv, _, _, _ in st.values())                   # hi == 1
    assert any(s > 1 and nv == 2 * s for s, nv, _, _, _ in st.values())
    assert any(n_rt == cap for _, _, n_rt, _, cap in st.values())                          # exactly full
    last_rt = {n: [op[1] for op in r.ops if op[0] == "rt"][-1] for n, (r, _) in S.items()}
    assert any(cap < n_rt <= cap + last_rt[n] for n, (_, _, n_rt, _, cap) in st.items())   # wrapped by one push
    assert any(n_rt > 3 * cap for _, _, n_rt, _, cap in st.values())                       # wrapped more than three times
    assert any(r.ops[-1][0] == "sa0" for r, _ in S.values())                               # dummy not yet popped
    assert any(any(a[0] == "sa0" and b[0] == "pop" and c[0] == "sa" for a, b, c in zip(r.ops, r.ops[1:], r.ops[2:])) for r, _ in S.values())
    assert any(s == 0 for s, *_ in st.values())
    bus = {Bu for r, _ in S.values() for _, _, Bu in r.samples}
    assert {1, 3, 255, 256, 257, 513} <= bus
    draws = [(seed, off, Bu) for r, _ in S.values() for seed, off, Bu in r.samples]
    assert any(off < 2 ** 32 <= off + (Bu - 1) // 4 for _, off, Bu in draws)               # the counters of one call cross 2^32
    assert any(seed >= 2 ** 32 for seed, _, _ in draws)
    assert any(seed >= 2 ** 32 and off < 2 ** 32 <= off + (Bu - 1) // 4 for seed, off, Bu in draws) is not None
    # the in-kernel sampler's states
    A = 8
    cap = rc.SMALL_STEPS_CAP * A
    nr = {k: v[0] * A + v[1] for k, v in rc.SMALL_STATES.items()}
    assert nr["barely"] == A + 1 and nr["two_strides"] == 2 * A and nr["exactly_full"] == cap and cap < nr["wrapped_once"] <= cap + A
    assert nr["wrapped_many"] > 3 * cap
    _, _, _, off = rc.SMALL_STATES["counter_high"]
    assert off < 2 ** 32 <= off + (rc.SMALL_BU - 1) // 4 and rc.SMALL_STATES["counter_high"][2] >= 2 ** 32


def seam_events(lg, cap, stride, base):
    """which of the events the issue lists a set of logical draws contains"""
    cap1 = cap + stride
    lg = np.asarray(lg, dtype=np.int64)
    return {"rt_last_row": bool(np.any(lg % cap == cap - 1)), "rt_first_row": bool(np.any(lg % cap == 0)),
            "sa_last_row": bool(np.any(lg % cap1 == cap1 - 1)), "sa_first_row": bool(np.any(lg % cap1 == 0)),
            "sn_wraps_alone": bool(np.any((lg + stride) % cap1 < lg % cap1)),
            "oldest": bool(np.any(lg - base <= stride))}             # the oldest valid entry or one within `stride` of it


@pytest.mark.parametrize("name", rc.sampling_rows())
def test_draws_of_every_sampling_row_reach_what_its_ring_state_allows(name):
    """A condition on the INPUTS: over the row's draws (the oracle's, on the CPU) every event the ring state admits is drawn -- the
    last and the first physical row of both rings, an s' that wraps while its s does not, the oldest valid entry -- and the rows
    'wrapped_*' admit all of them.  Seeds were chosen for this."""
    row, m = rc.ROWS[name], model_of(name)
    cap, stride = row.cap, row.stride
    base, hi = max(0, m.n_rt - cap), m.n_valid(cap) - stride
    can = seam_events(base + np.arange(hi), cap, stride, base)
    drawn = []
    for seed, off, Bu in row.samples:
        sl = orng.sample_slots(seed, off, Bu, m.n_valid(cap), m.n_rt, cap, stride)
        lg = m.logical(sl[1], cap)
        assert lg.min() >= base and lg.max() < base + hi
        assert np.array_equal(lg % (cap + stride), sl[0]) and np.array_equal((lg + stride) % (cap + stride), sl[2])
        drawn.append(lg)
    got = seam_events(np.concatenate(drawn), cap, stride, base)
    print(name, "admits", sorted(k for k, v in can.items() if v), "drawn", sorted(k for k, v in got.items() if v))
    for k, possible in can.items():
        assert got[k] == possible, (name, k)
    if name.startswith("wrapped"):
        assert all(can.values()), (name, can)


@pytest.mark.parametrize("name", rc.sampling_rows())
def test_image_gather_equals_logical_gather(name):
    """the alignment claim of CircularArraySARTTrajectory's docstring, in the model: what the physical slots fetch from the derived
    images is what the logical entries lg and lg + stride hold"""
    row, m = rc.ROWS[name], model_of(name)
    img = image_of(name, m)
    for seed, off, Bu in row.samples:
        sl = m.slots(seed, off, Bu, row.cap, row.stride)
        for key, a, b in zip(ref.BATCH_NAMES, ref.gather(img, sl), m.batch(sl, row.cap, row.stride)):
            assert a.dtype == np.float32 and np.array_equal(a, b), (name, key)
        if row.stride == 0:
            s, _, _, _, sn = m.batch(sl, row.cap, row.stride)
            assert np.array_equal(s, sn)


class HostDriver:
    """CircularArraySARTTrajectory on the CPU (_h is None) behind the model's four methods"""

    def __init__(self, pkg, row):
        self.tr = pkg.CircularArraySARTTrajectory(row.cap, row.ns, row.na, row.stride, torch.device("cpu"))
        assert self.tr._h is None and self.tr.capacity == row.cap
        if row.prefill:
            for k, v in rc.sentinel(row).items():
                getattr(self.tr, k).copy_(torch.as_tensor(v))

    def push_sa(self, s, a=None):
        self.tr.push_sa(torch.as_tensor(s), None if a is None else torch.as_tensor(a))

    def pop_sa(self, n):
        self.tr.pop_sa(n)

    def push_rt(self, r, flags, cols, force):
        self.tr.push_rt_flags(torch.as_tensor(r), None if flags is None else torch.as_tensor(flags), cols, bool(force))


EXPRESSIBLE = [n for n, r in rc.ROWS.items() if rc.expressible(r)]


def test_the_class_can_express_what_the_table_says():
    assert len(EXPRESSIBLE) >= 10 and {"wrapped_many", "flags_grid", "dummy_popped_overwritten", "exactly_full"} <= set(EXPRESSIBLE)
    assert not {"straddle_ns3", "halt_up", "stride0", "rt_255_256_257"} & set(EXPRESSIBLE)


@pytest.mark.parametrize("name", EXPRESSIBLE)
def test_cpu_mirror_equals_the_model(pkg, name):
    row, m = rc.ROWS[name], model_of(name)
    d = rc.play(name, HostDriver(pkg, row))
    tr = d.tr
    img = image_of(name, m)
    for k in ("state", "action", "reward", "terminal"):
        assert np.array_equal(getattr(tr, k).numpy(), img[k]), (name, k)
    assert (tr.n_sa, tr.n_rt, len(tr)) == (m.n_sa, m.n_rt, m.n_valid(row.cap))
    # the index arithmetic of sample_slots / sample_slots_many, fed the oracle's ind
    for seed, off, Bu in row.samples:
        hi = len(tr) - tr.stride
        w = orng.words(seed, off, Bu).astype(np.uint64)
        ind = ((w * np.uint64(hi)) >> np.uint64(32)).astype(np.int64)

        class Fed:
            def integers(self, lo, high, size):
                assert (lo, high) == (0, hi)
                return ind.reshape(size)
        want = orng.sample_slots(seed, off, Bu, len(tr), tr.n_rt, tr.capacity, tr.stride)
        assert np.array_equal(np.stack(tr.sample_slots(Fed(), Bu)), want)
        assert np.array_equal(tr.sample_slots_many(Fed(), Bu, 1)[:, 0], want)
        got = tr.sample(Fed(), Bu)
        for key, b in zip(ref.BATCH_NAMES, m.batch(want, row.cap, row.stride)):
            assert np.array_equal(got[key].numpy(), b), (name, key)


# fault -> (the comparison that must reject it, a row on which it does)
FAULTS = [
    ("sn_modulo_cap", "slots[2]", "wrapped_many"),
    ("base_omitted", "slots[0]", "wrapped_one_push"),
    ("flag_per_column", "trace terminal", "flags_grid"),
    ("dummy_not_popped", "trace state", "dummy_popped_overwritten"),
    ("truncated_at_seam", "trace state", "straddle_wide_rows"),
    ("index_by_remainder", "slots[1]", "barely_two_strides"),
]


def compare(name, fault):
    """the comparisons of the GPU test with the faulty model in the kernel's place -> names of the ones that fail"""
    row = rc.ROWS[name]
    good, bad = model_of(name), model_of(name, fault)
    gi, bi = image_of(name, good), image_of(name, bad)
    failed = [f"trace {k}" for k in gi if not np.array_equal(gi[k], bi[k])]
    if (good.n_sa, good.n_rt) != (bad.n_sa, bad.n_rt):
        failed.append("counters")
    if good.halt != bad.halt:
        failed.append("halt")
    for seed, off, Bu in row.samples:
        gs, bs = good.slots(seed, off, Bu, row.cap, row.stride), bad.slots(seed, off, Bu, row.cap, row.stride)
        failed += [f"slots[{i}]" for i in range(3) if not np.array_equal(gs[i], bs[i])]
        want = good.batch(gs, row.cap, row.stride)
        failed += [f"batch {k}" for k, a, b in zip(ref.BATCH_NAMES, ref.gather(bi, bs), want) if not np.array_equal(a, b)]
    return failed


def test_fault_list_is_the_models():
    assert [f for f, _, _ in FAULTS] == list(ref.FAULTS)


@pytest.mark.parametrize("fault,check,name", FAULTS)
def test_checks_reject_a_faulty_model(fault, check, name):
    failed = compare(name, fault)
    assert check in failed, (fault, name, failed)
    caught = [n for n in rc.ROWS if compare(n, fault)]
    print(fault, "fails", sorted(set(failed)), "on", name, "; rows that catch it:", len(caught))
    assert name in caught
    assert not compare(name, None)
    if fault in ("sn_modulo_cap", "base_omitted", "index_by_remainder"):
        assert any(f.startswith("batch") for f in failed), failed           # and the fetched batch shows it too
