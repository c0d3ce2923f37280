"""The case table of test_gpu_ks_faults.py: the rows of ks_geometry_cases.py on which per-trajectory actuator and sensor faults
(pdec_env_set_faults: csrc/ks_step.hip, ks_rollout.hip, ksfd.hip, env.hip: sense_kernel, episode_clock.hip) are held to the reference of
ks_fault_ref.py, the fault arrays they run with and the bound of the state comparison.  Imports numpy only: test_ks_fault_table.py
holds the table against the oracle without a GPU.

The arrays.  B = 5 (3 at 1024 cells); trajectory 1 is fully healthy (gains 1, bias 0), so a packed pair of the spectral step holds
a healthy and a faulty trajectory in one work-group.  The others take, entry by entry, the values of VALUES below in an order drawn
from a generator seeded by the row's sizes: no two trajectories agree in any entry of any array, and none sits within 0.25 of the
entry's mean over the batch, so that no trajectory can be mistaken for its partner, its neighbour or the mean.  The biases are in
units of the field (the inputs have |y| < 5)."""
import numpy as np

import ks_geometry_cases as kc

# the rows of ks_disturbance_cases.STEP_ROWS -- FftWave256 with odd A != S and a non-monotone map, FftFixed192 (window 5), the
# generic engine, FftWave1024, the one-wave finite-difference kernel and the general one with both integrators -- and the row of
# ks_geometry_cases with a temporal stack of two (the general featurize path: rows copied from the previous state)
STEP_ROWS = ("perm_oddA_256", "dense_192", "generic_60", "subset_1024", "fd_perm_256", "fd_irregular_256", "fd_midpoint_100",
             "stack2_perm_256")
STEPS = 3                       # teacher-forced control steps of the step tests
ROLL_T, ROLL_FROM = 8, 3        # the rollouts: T steps; once more with the actor engaging at step ROLL_FROM
ROLL_CASE = "perm_oddA_256"
HEALTHY = 1                     # the trajectory without faults
KEYS = ("actuator_gain", "sensor_gain", "sensor_bias")

# how far each mistake must move one control step of the oracle, in bounds of the GPU test's fp32 comparison: the margin of
# ks_disturbance_cases.MIN_BOUNDS, for the same reason (a test that a mistaken kernel passes by the width of its bound tests
# nothing)
MIN_BOUNDS = 30.0


def batch(case):
    return 3 if kc.CASES[case].nx == 1024 else 5


def sizes(case):
    c = kc.CASES[case]
    return kc.n_actuators(case), len(c.sensor_positions)


def pairs(case):
    """the trajectories that share a work-group of the spectral step (a packed pair), the neighbours of the batch otherwise"""
    B = batch(case)
    return [(b, b + 1) for b in range(0, B - 1, 2)]


# what the faulty trajectories hold, per entry: at B = 5 the four values in an order drawn per entry, at B = 3 the two values of the
# first pair on even entries and of the second on odd ones.  Each set keeps every value APART from the others, from the healthy
# value and from the mean of the entry over the batch (the healthy value included); it holds a dead gain, one above 1, a reversed
# actuator, a sensor reading 30 % high and biases of both signs.
VALUES = {"actuator_gain": (-1.5, 0.6, 0.0, 1.5), "sensor_gain": (0.0, 1.3, 0.4, 2.0), "sensor_bias": (-1.5, 0.75, -0.5, 2.0)}
HEALTHY_VALUE = {"actuator_gain": 1.0, "sensor_gain": 1.0, "sensor_bias": 0.0}
APART = 0.25


def faults(case):
    """dict of float64 arrays actuator_gain [B, A], sensor_gain [B, S], sensor_bias [B, S]"""
    B = batch(case)
    A, S = sizes(case)
    rng = np.random.default_rng([17, kc.CASES[case].nx, A, S])
    faulty = [b for b in range(B) if b != HEALTHY]
    out = {}
    for k in KEYS:
        n = A if k == "actuator_gain" else S
        x = np.full((B, n), HEALTHY_VALUE[k])
        for j in range(n):
            vals = VALUES[k] if B == 5 else VALUES[k][2 * (j % 2):2 * (j % 2) + 2]
            x[faulty, j] = rng.permutation(vals)
        out[k] = x
    return out


def healthy(case, B=None):
    A, S = sizes(case)
    B = batch(case) if B is None else B
    return dict(actuator_gain=np.ones((B, A)), sensor_gain=np.ones((B, S)), sensor_bias=np.zeros((B, S)))


# ------------------------------------------------------------------ the bound of the state comparison
def tol_state(prec, case, geo, ymax, gmax, bmax):
    """ks_geometry_cases.tol_state extended by the two roundings of g * d + b.  There: the dot d, a sum of Wd products with
    |d| <= ymax, is off by at most (Wd + 1) u ymax in any order of summation, the scale adds one more rounding, counted as
    (Wd + 3) u ymax / max_value.  Here the product g d adds u |g d| and carries the dot's error |g| times, and the sum g d + b adds
    u |g d + b| (a fused multiply-add rounds once: less).  With X = max|g| ymax + max|b| in the place of ymax every term is at most
    u X: (Wd + 5) u X / max_value.  Twice that, as there: the oracle's own fp64 sum carries the same bound in the fp64 comparison.
    Rows copied from the previous state are exact.  gmax, bmax: over the trajectory's own arrays (1 and 0 for the healthy one)."""
    c = kc.CASES[case]
    return 2 * (geo["Wd"] + 5) * kc.UNIT[prec] * (gmax * ymax + bmax) / c.max_value
