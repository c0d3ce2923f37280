"""The case table of test_gpu_population_update.py: the members' update launch (pdec_population_update, csrc/mlp_small.hip) on
every kernel small_plan can hand it.  Host only (numpy and oracle.rng on the rows of test_gpu_small_update.CASES; nothing here
touches a GPU); test_population_update_table.py holds its claims.

The shapes are the rows of CASES in test_gpu_small_update.py -- ns, na, widths, layers, Bu, rho and the kernel each must reach --
so every name of the small-update dispatch has a population case.  Every case runs M = 6 members with the roles below, each on
the trigger edge it is named for (sm_member_begin: no halt, min(n_rt, cap) > update_after rows, update_step % update_freq == 0):

  0  first_row_count_that_fires   nv = after + 1, ustep even, fresh ADAM state                                updates
  1  wrapped_aged_far_offset      n_rt = cap + 23 (the ring has wrapped), POP_SAMPLE > 2^32, ADAM state three solo
                                  launches old (its beta-power slots start at 1)                                updates
  2  row_count_equals_after       nv == after exactly                                                           does not
  3  ustep_odd                    ustep % update_freq == 1                                                      does not
  4  halted                       POP_HALT = 1, otherwise due                                                   does not
  5  shares_seed_of_member_0      as member 0 with member 0's sample seed at another offset                     updates

A row is the int64 [16] of csrc/population.hpp (enum PopSlot / PopHyperSlot; slot 15 is free)."""
import zlib
from collections import namedtuple
from functools import lru_cache

import numpy as np

from oracle import rng as orng
from test_gpu_small_update import CASES as SMALL_CASES

M, LOOPS, FREQ, CAP, STRIDE = 6, 2, 2, 64, 1
AFTER_ROWS = 4 * STRIDE
COLS, START_STEPS = 1, 0
ROW = 16
USTEP, NSA, NRT, NOISE, SAMPLE, HALT, ACTIVE, BPA, BPC, NOISE_AMP, LIMIT, GAMMA, RHO, ETA_A, ETA_C, SPARE = range(ROW)
MOVES = (SAMPLE, BPA, BPC)                      # what an update moves in its member's row
GAMMA0, ETA_A0, ETA_C0 = 0.99, 5e-4, 1e-3       # the launch-wide values (test_gpu_small_update's)

# the bounded instantiations of ddpg_small2_kernel: one gamma, rho and pair of step sizes for the whole launch
BOUNDED = ("ddpg_small2_kernel<4,3,4,0>", "ddpg_small2_kernel<10,9,4,0>", "ddpg_small2_kernel<13,12,4,0>",
           "ddpg_small2_kernel<16,15,4,0>")

CASES = dict(SMALL_CASES)

Member = namedtuple("Member", "role n_rt ustep halt aged seed offset updates")


def kernel_of(case):
    return CASES[case][7]


def serves_member_hyper(case):
    return kernel_of(case) not in BOUNDED


def dsample(case):
    """Philox counters one launch of LOOPS minibatches of Bu draws consumes"""
    return (LOOPS * CASES[case][5] + 3) // 4


def _draws(case, seed, offset, n_rt, launch=0):
    Bu = CASES[case][5]
    return orng.sample_slots(seed, offset + launch * dsample(case), LOOPS * Bu, min(n_rt, CAP), n_rt, CAP, STRIDE)


@lru_cache(maxsize=None)
def members(case):
    """the six members of a case.  Two free numbers are searched, not drawn, so that the few draws of a launch (2 at Bu = 1) show
    what the member is there for: member 1's offset is the first past 2^32 + 12345 whose first launch draws a row past the
    ring's seam (state slot != reward slot), member 5's the first from 1003 on whose two launches differ from member 0's"""
    s0 = 1000 + zlib.crc32(case.encode()) % 9973
    a = AFTER_ROWS
    off1 = (1 << 32) + 12345
    while not (_draws(case, s0 + 1, off1, CAP + 23)[0] != _draws(case, s0 + 1, off1, CAP + 23)[1]).any():
        off1 += 1
    off5 = 1003
    while any(np.array_equal(_draws(case, s0, off5, a + 1, k), _draws(case, s0, 3, a + 1, k)) for k in (0, 1)):
        off5 += 1
    return (Member("first_row_count_that_fires", a + 1, 6, 0, False, s0, 3, True),
            Member("wrapped_aged_far_offset", CAP + 23, 10, 0, True, s0 + 1, off1, True),
            Member("row_count_equals_after", a, 4, 0, False, s0 + 2, 40, False),
            Member("ustep_odd", CAP - 3, 7, 0, False, s0 + 3, 50, False),
            Member("halted", CAP + 5, 8, 1, False, s0 + 4, 60, False),
            Member("shares_seed_of_member_0", a + 1, 12, 0, False, s0, off5, True))


def n_valid(mb):
    """length(trajectory)"""
    return min(mb.n_rt, CAP)


def fires(mb):
    """Agent._maybe_update's trigger as sm_member_begin states it"""
    return not mb.halt and n_valid(mb) > AFTER_ROWS and mb.ustep % FREQ == 0


def slots(case, mb, launch=0):
    """int64 [3, LOOPS, Bu]: the slots member `mb` draws in its launch number `launch` (0, 1, ...) of the population"""
    Bu = CASES[case][5]
    s = orng.sample_slots(mb.seed, mb.offset + launch * dsample(case), LOOPS * Bu, n_valid(mb), mb.n_rt, CAP, STRIDE)
    return s.reshape(3, LOOPS, Bu)


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


def nan_patterns(m):
    """four different NaN bit patterns (quiet and signalling, both signs, payloads that name the member) as int64"""
    u = np.array([0x7FF8000000000001 + m, 0xFFF8000000000100 + m, 0x7FF0000000010000 + m, 0xFFFFFFFFFFFFFF00 + m], dtype=np.uint64)
    return u.view(np.int64)


def hyper(case):
    """[M, 4] gamma, rho, eta_a, eta_c of the per-member form: the updating members differ in all four (frozen cases keep
    rho = 1: the kernel is one for the launch), member 1 has both step sizes 0"""
    frozen = np.float32(CASES[case][6]) == np.float32(1.0)
    h = np.empty((M, 4))
    h[:, 0] = (0.99, 0.95, 0.97, 0.96, 0.98, 0.9)
    h[:, 1] = 1.0 if frozen else (0.995, 0.99, 0.97, 0.96, 0.999, 0.98)
    h[:, 2] = (5e-4, 0.0, 1e-3, 2e-4, 7e-4, 2e-3)
    h[:, 3] = (1e-3, 0.0, 2e-3, 5e-4, 3e-4, 3e-4)
    h[0] = (GAMMA0, CASES[case][6], ETA_A0, ETA_C0)      # member 0's are the values the population is created with
    return h


def rows(case, member_hyper=False):
    """int64 [M, 16] before the launch, BPA / BPC left 0 (pdec_population_bp_sel fills them).  Without member_hyper slots
    11..14 hold NaN bit patterns: the launch must not read them"""
    r = np.zeros((M, ROW), dtype=np.int64)
    for m, mb in enumerate(members(case)):
        r[m, [USTEP, NSA, NRT, NOISE, SAMPLE, HALT, ACTIVE]] = (mb.ustep, mb.n_rt + STRIDE, mb.n_rt, 700 + m, mb.offset, mb.halt, 1)
        r[m, NOISE_AMP:LIMIT + 1] = _bits([0.1 + 0.01 * m, 1.0])
        r[m, GAMMA:ETA_C + 1] = _bits(hyper(case)[m]) if member_hyper else nan_patterns(m)
        r[m, SPARE] = 0x5EED0000 + m
    return r


def rows_after(case, before, launches=1):
    """the rows `launches` population launches later: POP_SAMPLE advanced and both beta-power slots flipped for the members that
    update, every other slot and every other member as before"""
    r = before.copy()
    for m, mb in enumerate(members(case)):
        if mb.updates:
            r[m, SAMPLE] += launches * dsample(case)
            if launches % 2:
                r[m, [BPA, BPC]] ^= 1
    return r
