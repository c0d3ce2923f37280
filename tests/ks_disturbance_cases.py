"""The case table of test_gpu_ks_disturbance.py: the rows of ks_geometry_cases.py on which the per-trajectory KS disturbance
(pdec_env_set_disturbance: csrc/ks_step.hip, ks_rollout.hip, ksfd.hip) and delayed control (pdec_env_set_control_from) are held
to oracle/ks.py, and the amplitude vectors they run with.  The oracle takes one amplitude per configuration (KSConfig.mu), so a
batch is one KSConfig per trajectory from ks_geometry_cases.build.  Imports numpy only: test_ks_disturbance_table.py holds the
table against the oracle without a GPU.

The amplitudes.  A control step moves the field by about dt mu = 0.1 mu, so two amplitudes 0.1 apart differ by 1e-2 per step --
against the fp32 bound on y of 3e-5 max(1, |y|), |y| < 5.  (0.05, -0.05, 0.15, 0.0, 0.1) at B = 5: the two packed pairs (0, 1) and
(2, 3) are 0.1 and 0.15 apart, both signs and a zero occur, trajectory 4 is alone in its work-group, and nobody but trajectory 0
carries the batch's mean (0.05).  At 1024 cells B = 3, the first three: one pair and the lone trajectory."""
import numpy as np

import ks_geometry_cases as kc

MU = (0.05, -0.05, 0.15, 0.0, 0.1)

# the rows of the fused step and its split pieces: FftWave256 with odd A, FftFixed192, the generic engine, FftWave1024, the one-wave
# finite-difference kernel and the general one with both of its integrators
STEP_ROWS = ("perm_oddA_256", "dense_192", "generic_60", "subset_1024", "fd_perm_256", "fd_irregular_256", "fd_midpoint_100")
# the further rows on which the issue's own figures were taken (the table test keeps them measured)
TABLE_ROWS = STEP_ROWS + ("sparse_600",)
STEPS = 3                       # teacher-forced control steps of the step tests
ROLL_T, ROLL_FROM = 8, 3        # the rollouts: T steps, the actor engages at step ROLL_FROM

# how far a mistaken amplitude must move one control step of the oracle, in bounds of the GPU test's fp32 comparison
# (ks_geometry_cases.tol_y): 30 on every row.  Two amplitudes 0.1 apart move y by about dt 0.1 = 1e-2 in a step.  The spectral bound is
# 3e-5 max(1, |y|), |y| < 5 at these inputs: 1e-2 / 1.5e-4 = 67 at the least.  The finite-difference bound is 2e-4 max |y| with
# |y| about 1 after the first step of these inputs: 1e-2 / 2e-4 = 50.  Those kernels run one trajectory per work-group, so the mistake
# to catch there is a NEIGHBOUR's amplitude; the pairs below name the neighbours.  In fp64 (1e-11) every mistake is 1e8 bounds away.
MIN_BOUNDS = {"cnab2": 30.0, "rk4_fd": 30.0, "midpoint_fd": 30.0}


def batch(case):
    return 3 if kc.CASES[case].nx == 1024 else 5


def amplitudes(case):
    return np.array(MU[:batch(case)], dtype=np.float64)


def pairs(case):
    """the trajectories that share a work-group of the spectral step (a packed pair), the neighbours of the batch otherwise"""
    B = batch(case)
    return [(b, b + 1) for b in range(0, B - 1, 2)]


def configs(pkg, ks, case, mus):
    """(setup at the row's own mu, [KSConfig at mus[b] for b])"""
    setup, _ = kc.build(pkg, ks, case)
    return setup, [kc.build(pkg, ks, case, mu=float(m))[1] for m in mus]
