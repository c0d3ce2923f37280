"""The case table of test_gpu_replay_ring.py: the trajectory glue of csrc/replay.hip (replay_push2_kernel, replay_push_rt_kernel,
replay_sample_kernel, autoreset_kernel), the same pushes inside csrc/act.hip's step_glue_kernel and the slot table of
csrc/small_args.hpp, at the seams of the two rings -- away from the one geometry the shipped runs use (ns = na = 1, stride = A = 8,
a capacity that is a multiple of the push).  Imports neither torch nor numpy (numpy only inside the functions that draw data), so
test_replay_ring_table.py can hold the table against its claims on a machine without a GPU.

ROWS: name -> Row(cap, stride, ns, na, dtype, ops, samples, prefill, edge).  The state / action ring has cap + stride rows, the
reward / terminal ring cap.  dtype is the SOURCE type of the pushes ("f32" / "f64"; the traces are always float32).  ops:
  ("sa", n)                         push n (state, action) rows
  ("sa0", n)                        push n state rows with a == NULL: the zero-action dummy of POST_EPISODE
  ("pop", n)                        the host pops the dummy: n_sa -= n
  ("rt", n, flags, cols, force)     push n rewards; flags: None (done_flags == NULL) or one int per trajectory of `cols` columns
  ("halt", v)                       attach an episode halt flag holding v (None: detach)
samples: (seed, offset, Bu) draws of pdec_replay_sample from the ring the ops leave behind.  prefill: the traces hold a sentinel
pattern before the first op (the rows that check "nothing written").  edge: what the row is there for.

A row goes through CircularArraySARTTrajectory where the class can express it (`expressible`) and through the library's C entry
points otherwise: a capacity that is no multiple of the stride, a halt flag, done_flags == NULL without a time-out, a flag vector
that does not cover the push exactly, stride 0.

A ring can be sampled while n_rt <= n_sa <= n_rt + stride: the state ring is only `stride` rows longer than the reward ring, so
more than `stride` rows pushed ahead of their rewards would overwrite states that can still be drawn (the stage loop pushes
stride = B A rows a step).  The sampling rows whose pushes are larger than the stride therefore end with a partial PRE_ACT push.

stride = 0 is accepted by pdec_replay_sample and the model gives it a meaning -- both rings have `cap` rows and s' == s -- so the
row `stride0` holds it.

Data: np.random.default_rng([crc32(name), k]) for op k of a row; standard normal in float64, rounded to float32 for an "f32" row.
Every value is distinct, so a row read from or written to the wrong place shows."""
import zlib
from collections import namedtuple

Row = namedtuple("Row", "cap stride ns na dtype ops samples prefill edge")

BLOCK = 256                        # threads of a push / sample block (csrc/replay.hip)
E_INVALID = -1                     # PDEC_E_INVALID (include/pdeconv.h)
SEED64 = (7 << 32) | 12345         # a seed whose high word is not zero
OFF_CROSS = (1 << 32) - 3          # counters offset + k / 4 cross 2^32 from the fourth block on
SENTINEL = -77.0


def _row(cap, stride, ns, na, dtype, ops, edge, samples=(), prefill=False):
    return Row(cap, stride, ns, na, dtype, tuple(ops), tuple(samples), prefill, edge)


def _steps(k, n, cols=None, flags_at=None):
    """k control steps of n columns: PRE_ACT push, POST_ACT push (flags (1,) at step flags_at)"""
    ops = []
    for i in range(k):
        ops += [("sa", n), ("rt", n, (1 if i == flags_at else 0,), cols or n, 0)]
    return ops


def _patterns(ntraj):
    return [tuple([0] * ntraj), tuple([1] * ntraj), tuple([1] + [0] * (ntraj - 1)), tuple([0] * (ntraj - 1) + [1])]


_FLAG_GRID = [("rt", c * m, f, c, 0) for c in (1, 3, 8) for m in (1, 2, 5) for f in _patterns(m)]

ROWS = {
    # ------------------------------------------------------------------ pushes
    "ends_on_last_row": _row(20, 3, 3, 2, "f64", [("sa", 16), ("sa", 7), ("rt", 13, None, 1, 0), ("rt", 7, None, 1, 0), ("sa", 1)],
                             "a push that ends exactly on the last row of either ring; the next one starts at row 0"),
    "starts_on_last_row": _row(20, 1, 1, 1, "f32", [("sa", 20), ("sa", 5), ("rt", 19, (0,), 19, 0), ("rt", 4, (1,), 4, 0)],
                               "a push that starts on the last row and wraps"),
    "straddle_wide_rows": _row(10, 3, 8, 2, "f64", [("sa", 11), ("sa", 6), ("rt", 8, None, 1, 0), ("rt", 5, None, 1, 0)],
                               "a push across the seam with ns = 8, na = 2: the row / feature split of the flat index"),
    "straddle_ns3": _row(11, 8, 3, 1, "f32", [("sa", 17), ("sa", 5), ("rt", 9, None, 1, 0), ("rt", 7, None, 1, 0)],
                         "the same with ns = 3 at stride 8, a capacity that no push divides"),
    "n_equals_capacity": _row(12, 8, 1, 2, "f64", [("sa", 7), ("sa", 20), ("rt", 5, None, 1, 0), ("rt", 12, None, 1, 0)],
                              "n == capacity with start != 0: every row rewritten, the seam in the middle"),
    "elems_255": _row(63, 3, 3, 2, "f32", [("sa", 30), ("sa", 51), ("rt", 40, (0, 1), 20, 0)],
                      "n (ns + na) = 255: one block, its last thread idle; wraps"),
    "elems_256": _row(70, 8, 3, 1, "f64", [("sa", 30), ("sa", 64), ("rt", 40, None, 1, 0)], "n (ns + na) = 256: one block exactly"),
    "elems_257": _row(5, 1, 255, 2, "f64", [("sa", 5), ("sa", 1), ("sa", 1), ("rt", 3, None, 1, 0)],
                      "n (ns + na) = 257 (one row of 255 + 2): the action part straddles the two blocks"),
    "elems_600": _row(72, 8, 8, 2, "f32", [("sa", 50), ("sa", 60), ("rt", 40, (1, 0), 20, 0)],
                      "n (ns + na) = 600: three blocks, the state / action split inside the third; wraps"),
    "rt_255_256_257": _row(300, 8, 1, 1, "f64", [("sa", 8), ("rt", 255, (0,) * 31 + (1,), 8, 0), ("rt", 256, (1,) + (0,) * 31, 8, 0),
                                                ("rt", 257, (0,) * 32 + (1,), 8, 0)],
                           "reward pushes of 255, 256 and 257 rows without a halt flag; the last trajectory is a partial one"),
    "rt_f32_blocks": _row(300, 3, 1, 2, "f32", [("sa", 3), ("rt", 257, (0, 1) * 43, 3, 0), ("rt", 255, (1, 0) * 43, 3, 0)],
                          "the fp32-source reward push over two blocks, 3 columns per trajectory"),
    "dummy_over_actions": _row(6, 3, 1, 2, "f64", [("sa", 9), ("sa0", 3), ("rt", 6, (0, 1, 0), 2, 0)],
                               "a == NULL onto rows that held non-zero actions"),
    "dummy_over_actions_f32": _row(9, 3, 8, 1, "f32", [("sa", 12), ("sa0", 5), ("rt", 9, (0,), 9, 1)],
                                   "the same from an fp32 source, the dummy across the seam"),
    "n_zero": _row(9, 3, 3, 1, "f64", [("sa", 0), ("sa0", 0), ("rt", 0, None, 1, 0)], "n == 0 leaves everything untouched", prefill=True),
    "ns8_na1": _row(16, 8, 8, 1, "f64", _steps(5, 8), "ns = 8, na = 1 through the class, wrapped"),
    "ns1_na2": _row(9, 3, 1, 2, "f32", _steps(7, 3), "ns = 1, na = 2 through the class, wrapped"),
    # ------------------------------------------------------------------ terminal flags
    "flags_grid": _row(96, 8, 1, 1, "f64", [("sa", 8)] + _FLAG_GRID,
                       "cols_per_traj 1 / 3 / 8 x 1 / 2 / 5 trajectories x none / all / first / last"),
    "flags_null_and_force": _row(50, 8, 1, 1, "f32", [("sa", 8), ("rt", 15, None, 3, 0), ("rt", 15, (0,) * 5, 3, 1), ("rt", 16, (0, 0), 8, 1),
                                                     ("rt", 5, None, 1, 1), ("rt", 10, (0, 1, 0, 0, 1), 2, 0)],
                                 "done_flags == NULL, and force = 1 over a zero flag vector"),
    # ------------------------------------------------------------------ halt
    "halt_down_no_done": _row(12, 3, 3, 1, "f64", [("halt", 0), ("sa", 4), ("rt", 4, (0,), 4, 0), ("sa", 4), ("rt", 4, None, 4, 0)],
                              "flag down, no done: everything pushed, the flag stays down", prefill=True),
    "halt_down_done0": _row(12, 3, 3, 1, "f64", [("halt", 0), ("sa", 4), ("rt", 4, (1, 0), 2, 0), ("sa", 4), ("rt", 4, (0, 0), 2, 0), ("sa0", 2)],
                            "flag down, done[0] set: the row is pushed and the flag raised; the following pushes are skipped", prefill=True),
    "halt_down_done1_only": _row(12, 3, 1, 2, "f32", [("halt", 0), ("sa", 4), ("rt", 4, (0, 1), 2, 0), ("sa", 4)],
                                 "flag down, only done[1] set: the flag stays down", prefill=True),
    "halt_up": _row(12, 3, 1, 2, "f64", [("halt", 1), ("sa", 4), ("rt", 4, (1,), 4, 0), ("sa0", 4), ("rt", 4, None, 1, 1)],
                    "flag up: neither kernel writes anything", prefill=True),
    # ------------------------------------------------------------------ sampling
    "barely_hi1": _row(8, 1, 3, 1, "f64", [("sa", 3), ("rt", 2, None, 1, 0)], "n_valid = stride + 1 at stride 1: hi == 1, every draw is entry 0",
                       samples=[(11, 0, 3), (11, 9, 1)]),
    "barely_two_strides": _row(12, 3, 1, 2, "f32", [("sa", 9), ("rt", 6, None, 1, 0)], "n_valid = 2 stride", samples=[(12, 4, 255)]),
    "exactly_full": _row(24, 8, 1, 1, "f64", _steps(3, 8, flags_at=1) + [("sa", 8)], "n_rt == cap: full, not wrapped", samples=[(13, 2, 256)]),
    "wrapped_one_push": _row(40, 3, 1, 1, "f64", _steps(5, 10, cols=10, flags_at=3) + [("sa", 3)],
                             "wrapped by one push of 10 into 40 / 43 rows: base = one push", samples=[(14, 1, 257)]),
    "wrapped_many": _row(24, 3, 3, 2, "f32", _steps(20, 5, cols=5, flags_at=17) + [("sa", 2)],
                         "pushes of 5 into 24 / 27 rows: wrapped four times, the seams of the two rings apart",
                         samples=[(15, 7, 513), (15, 1000, 1)]),
    "wrapped_many_counter_high": _row(24, 3, 3, 2, "f32", _steps(20, 5, cols=5, flags_at=17) + [("sa", 2)],
                                      "the same ring; the counters of one call cross 2^32 (the high counter word), and a seed >= 2^32",
                                      samples=[(16, OFF_CROSS, 255), (SEED64, 3, 256), (SEED64, OFF_CROSS, 3)]),
    "dummy_not_popped": _row(40, 8, 8, 1, "f64", _steps(7, 8, flags_at=6) + [("sa0", 8)], "a dummy row pushed and not yet popped; wrapped",
                             samples=[(17, 5, 255)]),
    "dummy_popped_overwritten": _row(40, 8, 1, 2, "f64", _steps(4, 8, flags_at=3) + [("sa0", 8), ("pop", 8)] + _steps(3, 8) + [("sa", 8)],
                                     "a dummy row popped and overwritten by the next episode; wrapped", samples=[(18, 6, 256)]),
    "stride0": _row(16, 0, 1, 2, "f64", _steps(5, 5, cols=5), "stride 0: both rings of `cap` rows, s' == s", samples=[(19, 8, 257)]),
}

# host refusals: argument checks that return PDEC_E_INVALID before any launch.  (call, overrides of a valid baseline call)
REFUSALS = {
    "rt_halt_more_than_one_block": ("push_rt", dict(cap=300, n=257, halt=True)),
    "sa_n_above_capacity": ("push_sa", dict(cap=12, n=13)),
    "rt_n_above_capacity": ("push_rt", dict(cap=12, n=13, halt=False)),
    "sample_nothing_valid": ("sample", dict(cap=12, stride=3, n_valid=3, n_rt=3)),          # n_valid - stride < 1
    "sample_valid_above_capacity": ("sample", dict(cap=12, stride=3, n_valid=13, n_rt=13)),
}
ACCEPTED = {          # the same calls one step inside the bound: they succeed
    "rt_halt_one_block": ("push_rt", dict(cap=300, n=256, halt=True)),
    "sa_n_at_capacity": ("push_sa", dict(cap=12, n=12)),
    "sample_one_valid": ("sample", dict(cap=12, stride=3, n_valid=4, n_rt=4)),
}

# ring states of the in-kernel sampler (csrc/small_args.hpp, pdec_ddpg_update_small_rng) for a setup of A columns a step and a
# trajectory of 5 A rows: name -> (full control steps, further reward columns, seed, offset).  One loop of SMALL_BU columns.
SMALL_BU, SMALL_STEPS_CAP = 6, 5
SMALL_STATES = {
    "barely": (1, 1, 21, 3),               # n_valid = A + 1: hi == 1
    "two_strides": (2, 0, 22, 4),
    "exactly_full": (5, 0, 23, 5),
    "wrapped_once": (6, 0, 24, 6),
    "wrapped_many": (23, 0, 25, 7),
    "counter_high": (23, 0, SEED64, (1 << 32) - 1),       # six draws = counters 2^32 - 1 and 2^32
}

# step glue at the seams (KS22, B = 1, A = 8, a trajectory of 320 rows: rings of 320 and 328 rows): control steps pushed before
# the glue launches, and the number of glue launches.  The launch that the case is about (done flag / zero action) is the second.
GLUE_CAP = 320
GLUE_LAPS = {
    # n_rt = 304, n_sa = 312: launch 2 fills rows 312..319 of the reward ring AND 320..327 of the state ring, launch 3 starts both at 0
    "first_lap": (38, 3),
    # n_rt = 624, n_sa = 632: launch 2 fills the last rows of the reward ring, launch 3 those of the state ring, launch 4 starts it at 0
    "second_lap": (78, 4),
}
GLUE_CASES = ("mid_episode", "zero_policy", "episode_ends_here", "episode_ended_before")

# same-step reset: geometries out of ks_geometry_cases.py (the smaller rows; mono_192_wide is the global agent)
RESET_GEOMETRIES = ("generic_60", "mono_192_wide")
RESET_B = (1, 3, 5)


def done_patterns(B):
    """none, all, one in the middle, first with last"""
    mid = [0] * B
    mid[B // 2] = 1
    ends = [0] * B
    ends[0] = ends[-1] = 1
    return [[0] * B, [1] * B, mid, ends]


# ------------------------------------------------------------------ what a row is
def expressible(row):
    """can CircularArraySARTTrajectory (its torch path included) play the row?"""
    if row.stride < 1 or row.cap % row.stride or row.cap < row.stride:
        return False
    for op in row.ops:
        if op[0] == "halt":
            return False
        if op[0] == "rt":
            _, n, flags, cols, force = op
            if flags is None and not force:
                return False
            if flags is not None and len(flags) * cols != n:
                return False
    return True


def seed_of(name, k):
    return [zlib.crc32(name.encode()), int(k)]


def np_dtype(prec):
    import numpy as np
    return {"f32": np.float32, "f64": np.float64}[prec]


def op_data(name, k, op, row):
    """the arrays of op k of a row, in the row's source dtype: (s, a | None) of a push_sa, (r,) of a push_rt"""
    import numpy as np
    rng = np.random.default_rng(seed_of(name, k))
    dt = np_dtype(row.dtype)
    if op[0] in ("sa", "sa0"):
        s = rng.standard_normal((op[1], row.ns)).astype(dt)
        return s, (rng.standard_normal((op[1], row.na)).astype(dt) if op[0] == "sa" else None)
    return (rng.standard_normal(op[1]).astype(dt),)


def sentinel(row):
    """the prefill of the four traces: distinct non-zero values"""
    import numpy as np
    cap1 = row.cap + row.stride
    f = lambda n, k: (SENTINEL - k - np.arange(n, dtype=np.float32) / 8).astype(np.float32)
    return dict(state=f(cap1 * row.ns, 0).reshape(cap1, row.ns), action=f(cap1 * row.na, 1000).reshape(cap1, row.na),
                reward=f(row.cap, 2000), terminal=f(row.cap, 3000))


def play(name, target, row=None):
    """apply the row's ops to `target`: the model (replay_ring_ref.Replay) or a driver with the same four methods"""
    import numpy as np
    row = row or ROWS[name]
    for k, op in enumerate(row.ops):
        if op[0] in ("sa", "sa0"):
            target.push_sa(*op_data(name, k, op, row))
        elif op[0] == "pop":
            target.pop_sa(op[1])
        elif op[0] == "rt":
            _, n, flags, cols, force = op
            target.push_rt(op_data(name, k, op, row)[0], None if flags is None else np.array(flags, dtype=np.int32), cols, force)
        elif op[0] == "halt":
            target.set_halt(op[1])
        else:
            raise ValueError(op)
    return target


def sampling_rows():
    return [n for n, r in ROWS.items() if r.samples]
