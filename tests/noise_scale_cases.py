"""The case table of test_gpu_noise_scale.py: the smallest shapes at which each acting path that honours the per-trajectory
exploration amplitude (pdec_mlp_set_noise_scale) can get an index wrong, the amplitudes they run with, and a host restatement of
the routing rules (fused_act_ok, fused2_act_supported, the few-column kernel, the generic sequence) that
says which kernel a row must reach.  Imports numpy only: test_noise_scale_table.py holds the table without a GPU or the library.

Every acting row is (kernel it must reach, dtype of the states, dtype of the networks, layer widths, B trajectories, A columns
each, cols_per_entry, noise rows).  The amplitudes cycle through three distinct levels, one of them 0, so neighbouring entries
always differ; an entry is cols_per_entry consecutive columns, and with A = 5 or 7 entries straddle the 16-column wave tiles and
the 64-column blocks of the fused kernels."""
import math
from collections import namedtuple

import numpy as np

ACT_LIMIT = 100.0            # no element can reach the clamp (no_clamp_bound): the clamp is held by CLAMP_ROW alone
LEVELS = (0.7, 0.0, 2.0)     # the three amplitudes of a mixed array, at most 2
EQUAL = 1.3                  # the amplitude of the equal-values array and of the scalar call it must reproduce
ROLL_LEVELS = (0.3, 0.0, 0.1)
ROLL_EQUAL = 0.2
SEED, OFFSET = 4242, 17

Row = namedtuple("Row", "kernel state_dtype net_dtype dims acts B A cpe noise_rows")

RELU, TANH = "relu", "tanh"
ROWS = {
    # fused 3-layer acting: 135 columns = two full 64-column blocks and a ragged one of 7
    "fused3_mta2": Row("policy_act_fused_kernel<2>", "f32", "f32", (12, 24, 24, 1), (RELU, RELU, TANH), 27, 5, 5, -1),
    "fused3_mta1": Row("policy_act_fused_kernel<1>", "f32", "f32", (12, 10, 10, 1), (RELU, RELU, TANH), 27, 5, 5, -1),
    "fused3_cpe1": Row("policy_act_fused_kernel<2>", "f32", "f32", (12, 24, 24, 1), (RELU, RELU, TANH), 27, 5, 1, -1),
    "fused3_cpe2A": Row("policy_act_fused_kernel<1>", "f32", "f32", (12, 10, 10, 1), (RELU, RELU, TANH), 28, 5, 10, -1),
    # fused 2-layer acting: 259 columns, past the 256-state threshold
    "fused2_kb2": Row("policy_act2_kernel<2,2>", "f32", "f32", (12, 20, 1), (RELU, TANH), 37, 7, 7, -1),
    "fused2_kb5": Row("policy_act2_kernel<1,5>", "f32", "f32", (24, 12, 1), (RELU, TANH), 37, 7, 7, -1),
    # the few-column kernel: fp64 states under Float32 nets (the reference's shape), fp32, and two outputs with one noise row
    "small_f64_f32": Row("small_act_kernel", "f64", "f32", (12, 20, 1), (RELU, TANH), 1, 8, 8, -1),
    "small_f32": Row("small_act_kernel", "f32", "f32", (12, 20, 1), (RELU, TANH), 3, 5, 5, -1),
    "small_memory": Row("small_act_kernel", "f32", "f32", (13, 20, 2), (RELU, TANH), 3, 5, 5, 1),
    # the generic sequence: hidden width 32 is one step outside the fused predicate, 259 columns outside the few-column kernel
    "generic_f32": Row("generic", "f32", "f32", (12, 32, 32, 1), (RELU, RELU, TANH), 37, 7, 7, -1),
    "generic_f64": Row("generic", "f64", "f64", (12, 32, 32, 1), (RELU, RELU, TANH), 37, 7, 7, -1),
}
GLUE_ROW = "small_f64_f32"   # pdec_step_glue at B = 1
CLAMP_ROW = "small_f32"      # run once more with act_limit = 1: the noise is added before the clamp

# the rollouts: (environment, B, steps).  KS: ks_geometry_cases.perm_oddA_256 (N = 256, odd A), an odd batch so that the last
# trajectory is alone in its workgroup; Keller-Segel: the shipped geometry
KS_ROLL = ("perm_oddA_256", 3, 4)
KSEG_ROLL = (2, 4)

# routing constants restated from the sources (csrc/mlp_mfma.hip, mlp_mfma2.hip, act.hip, mlp.hpp)
KXP, FUSED3_ACT_MAX_H, K2MAX, FUSED2_KBS = 16, 31, 6, (2, 5, 6)
SMALL_ACT_MAXL, SMALL_ACT_LDS = 4, 48 * 1024


def cols(r):
    return r.B * r.A


def entries(r):
    assert cols(r) % r.cpe == 0, r
    return cols(r) // r.cpe


def mixed(n, levels=LEVELS):
    """n amplitudes cycling through the three levels: neighbours always differ"""
    return np.array([levels[i % 3] for i in range(n)], dtype=np.float64)


def per_column(scale, r):
    return np.repeat(np.asarray(scale), r.cpe)


def _tiles(H):
    return (H + 1 + 15) // 16


def route(r):
    """the name pdec_debug_batched_update_route(which = 4) reports for the row's actor on its columns"""
    d, f32 = r.dims, r.net_dtype == "f32" and r.state_dtype == "f32"
    L = len(d) - 1
    if (f32 and L == 3 and d[1] == d[2] and d[0] + 1 <= KXP and d[3] == 1 and r.acts[:2] == (RELU, RELU)
            and _tiles(d[1]) in (9, 2, 1) and d[1] <= FUSED3_ACT_MAX_H):
        return f"policy_act_fused_kernel<{_tiles(d[1])}>"
    if (f32 and L == 2 and d[2] == 1 and cols(r) >= 256 and r.acts[0] == RELU and r.acts[1] in (TANH, "identity")
            and d[0] <= 8 * K2MAX and _tiles(d[1]) <= 2):
        kb = next(k for k in FUSED2_KBS if (d[0] + 7) // 8 <= k)
        return f"policy_act2_kernel<{_tiles(d[1])},{kb}>"
    ts = 8 if r.state_dtype == "f64" else 4
    same_or_promoted = r.net_dtype == r.state_dtype or (r.net_dtype == "f32" and r.state_dtype == "f64")
    if L <= SMALL_ACT_MAXL and same_or_promoted and 2 * max(d) * cols(r) * ts <= SMALL_ACT_LDS:
        return "small_act_kernel"
    return "generic"


def max_normal():
    """the largest |z| the Box-Muller transform of u = (w + 0.5) 2^-32 can give: sqrt(-2 ln(2^-33))"""
    return math.sqrt(2 * 33 * math.log(2))


def no_clamp_bound(levels):
    """the largest |action| of a tanh-bounded actor plus noise at these amplitudes"""
    return 1.0 + max(levels) * max_normal()


def draw_tolerance(greedy, scale_c, z_c, dtype):
    """the bound on |noisy - greedy - scale_c z_c|: one rounding of the product, one of the sum and the rounding of z to the
    kernel's type, plus the device's normal draw against the host's (1e-12, test_gpu_memory.py)"""
    u = 2.0 ** -24 if dtype == "f32" else 2.0 ** -53
    return 3 * u * (np.abs(greedy) + np.abs(scale_c * z_c)) + 1e-12 * scale_c
