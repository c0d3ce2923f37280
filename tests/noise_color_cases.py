"""The case table of test_gpu_noise_color.py: temporally correlated exploration noise (pdec_mlp_set_noise_color) on every acting
kernel that honours it.  The acting rows, the routing rules and the draw tolerance are those of noise_scale_cases.py -- the shapes
there are already the smallest at which each kernel can get a column index wrong: 135 and 259 columns, entries straddling the
16-column tiles and the 64-column blocks, fp64 states under fp32 nets, two outputs with one noise row -- and this file adds the
correlations they run with, the fp64 recurrence and its error bound.  Imports numpy only.

The process: element i = column * outputs + row keeps a double x[i]; a learning call draws the normal z the white call draws
for i and computes x = a_e x + b_e z (e = column / cols_per_entry, b = sqrt(1 - a^2)), then adds (T)x * amplitude."""
import numpy as np

from noise_scale_cases import (ROWS, GLUE_ROW, CLAMP_ROW, SEED, OFFSET, ACT_LIMIT, LEVELS, EQUAL, route, mixed, cols,  # noqa: F401
                               entries, per_column, draw_tolerance, max_normal)

CORR = (0.9, 0.0, 0.5)       # the three correlations of a mixed array, cycling per entry: neighbours differ, one is white
STEPS = 4                    # consecutive acting calls
U = 2.0 ** -53


def corr(n):
    """n correlations cycling through CORR"""
    return mixed(n, CORR)


def ab_of(a):
    """{a, b = sqrt(1 - a^2)} per entry, [n, 2] in float64: what pdec_mlp_set_noise_color reads"""
    a = np.asarray(a, dtype=np.float64)
    return np.ascontiguousarray(np.stack([a, np.sqrt(1.0 - a * a)], axis=1))


def counters(r):
    """Philox counters one acting call of the row consumes (four normals each)"""
    return (cols(r) * r.dims[-1] + 3) // 4


def model(x0, ab, z_steps, noise_rows=-1):
    """the fp64 recurrence: x0 [cols, outputs], ab [cols, 2] (per column), z_steps [T, cols, outputs]; returns the states after
    every step [T, cols, outputs].  Rows >= noise_rows keep x0."""
    x = np.array(x0, dtype=np.float64, copy=True)
    nrows = x.shape[1] if noise_rows < 0 else noise_rows
    a, b = ab[:, 0:1], ab[:, 1:2]
    out = []
    for z in z_steps:
        x = x.copy()
        x[:, :nrows] = a * x[:, :nrows] + b * z[:, :nrows]
        out.append(x)
    return np.stack(out)


def state_tolerance(t, a):
    """the bound on |device state - model| after t steps at correlation a (array or scalar), from an exact x0.  Per step
    e_t <= a e_{t-1} + 1e-12 b + 2 u (|a x| + |b z|): the device's normal against the host's (1e-12, the project's bound,
    test_gpu_memory.py) scaled by b, and 2 u for the roundings of the two products and the sum, which also covers an FMA
    contraction of either product; |x|, |z| <= max_normal()."""
    a = np.asarray(a, dtype=np.float64)
    b = np.sqrt(1.0 - a * a)
    e = np.zeros_like(a)
    for _ in range(t):
        e = a * e + 1e-12 * b + 2 * U * (a + b) * max_normal()
    return e


def action_tolerance(greedy, scale_c, x_c, dtype, e_t):
    """the bound on |noisy - greedy - scale_c x_c|: the draw tolerance with x in the place of z, plus the state's error times the
    amplitude"""
    return draw_tolerance(greedy, scale_c, x_c, dtype) + scale_c * e_t
