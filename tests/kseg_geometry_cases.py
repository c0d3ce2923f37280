"""The case table of test_gpu_kseg_geometry.py: geometries of the 1-D Keller-Segel environment (csrc/kseg.hip:
kseg_env_step_kernel, kseg_rollout_kernel; csrc/env_sense.hpp: sense_dots, actuate_cell, featurize_traj, reward_traj, block_max, write_terminal and the
band construction of pdec_env_create) away from the one shipped point (100 cells, 20 sensors every 5 cells, actuators on sensors
3..18, window 3, temporal_steps 2), plus a plain-Python restatement of the host rules that decide what a geometry reaches
(work-group size, band widths, sense_dots' grouping, the LDS bill of the persistent rollout).  Imports numpy only, so
test_kseg_geometry_table.py holds every claim of the table against the oracle and the setup's host tables without a GPU.

Every row keeps dx = Lx / nx = 0.1 (the shipped cell size): with h = dt / substeps the explicit RK4 step is stable for about
4 h / dx^2 < 2.78, which the defaults meet at dx = 0.1 (0.075) and nx = 1024 on Lx = 10 does not (19.7)."""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "nx Lx sensor_positions actuators_to_sensors window_size temporal_steps substeps integrator "
                          "action_punish delta_action_punish check_max_value max_value")


def _case(nx, sensors, a2s, window_size=3, temporal_steps=2, substeps=32, integrator="rk4", action_punish=0.0,
          delta_action_punish=0.0, check_max_value="y", max_value=20.0, Lx=None):
    return Case(int(nx), float(nx / 10 if Lx is None else Lx), tuple(int(s) for s in sensors), tuple(int(a) for a in a2s),
                window_size, temporal_steps, substeps, integrator, action_punish, delta_action_punish, check_max_value, max_value)


def _every(n, step=1, first=1):
    return range(first, n + 1, step)


_S100 = range(3, 101, 5)                                   # the shipped sensors: 3, 8, ..., 98
_WRAP100 = [1] + list(range(2, 21, 2))                     # first and last sensor are actuators: window 3 reads sensors 20 and 1 across the seam
_S257 = list(range(3, 254, 5)) + [255]                     # 52 sensors, the last box ends on the last cell
_S1024 = list(range(3, 1019, 5)) + [1022]                  # 205 sensors, the last box ends on cell 1024

CASES = {
    # ---- work-group sizes (nthreads = ceil(nx / 64) 64) and what the last cell shares a wave with
    "wave1_nx64": _case(64, range(3, 63, 3), _every(20)),                                  # 64 threads, no dead lane; boxes overlap
    "dead63_nx65": _case(65, range(3, 64, 5), _every(13)),                                 # 128 threads, cell 65 alone in wave 1, under the last actuator
    "nx257": _case(257, _S257, [52, 1] + list(range(3, 51, 2))),                           # 320 threads, cell 257 alone in wave 4
    "nx1000": _case(1000, range(3, 1001, 5), _every(200, 2)),                              # 1024 threads, 24 dead lanes, 100 actuators
    "nx1024": _case(1024, _S1024, [205] + list(range(1, 205, 2))[:99]),                    # 1024 threads, 16 full waves, 100 actuators
    "smallest_nx8": _case(8, [3, 4, 5, 6], [1, 2, 3, 4]),                                  # N = 4 is pdec_env_create's floor; 8 is the smallest grid with S >= window = 3
    # ---- the shipped grid with other bands
    "wrap_nx100": _case(100, _S100, _WRAP100),
    "overlap_nx100": _case(100, range(3, 99, 3), _every(32)),                              # spacing 3: Cnt == 2, Wd still 5
    "rotated_nx100": _case(100, range(3, 99, 3), list(range(5, 33)) + [1, 2, 3, 4]),           # overlapping boxes of actuators A-1 and 0: the band wraps
    "permuted_nx100": _case(100, _S100, [17, 3, 20, 8, 1, 12, 5, 14, 10], action_punish=0.3, delta_action_punish=0.7),
    "punish_nx100": _case(100, _S100, range(3, 19), action_punish=0.3, delta_action_punish=0.7),
    # ---- featurize: the fmap gather with two species, the general path with a deep stack
    "fmap_w3_nx100": _case(100, _S100, _WRAP100, window_size=3, temporal_steps=1),
    "fmap_w5_nx65": _case(65, range(3, 64, 5), [13, 2, 1, 7, 12], window_size=5, temporal_steps=1),
    "stack3_w1_nx100": _case(100, _S100, _WRAP100, window_size=1, temporal_steps=3),
    "stack3_w5_nx64": _case(64, range(3, 63, 3), [20, 1, 2, 10, 19], window_size=5, temporal_steps=3),
    # ---- sense_dots: one group (S > nthreads / 2), actuate_cell: five rows per cell
    "ng1_nx64": _case(64, range(3, 63), _every(60)),
    # ---- the built-in midpoint integrator and the other blow-up tests away from the shipped size
    "midpoint_nx65": _case(65, range(3, 64, 5), _every(13), integrator="midpoint", substeps=8),
    "rewardcheck_nx100": _case(100, _S100, _WRAP100, check_max_value="reward", max_value=0.5),
    "nocheck_nx65": _case(65, range(3, 64, 5), _every(13), check_max_value="off"),
    # ---- the persistent rollout above 256 threads with few actuators (kseg_rollout_kernel<T, true, 1024>)
    "roll_nx320": _case(320, range(3, 321, 20), [16, 1, 3, 5, 8, 11, 13, 14]),
}

# blow-up handling (test 3c): base rows whose LAST sensor is an actuator, so a patch on the last cells is seen by the reward test
# too; nx = 65: the patch sits on the one live lane of wave 1, nx = 1024: in the last of 16 waves of block_max
BLOWUP = ["dead63_nx65", "wrap_nx100", "nx1024", "smallest_nx8"]
BLOWUP_REWARD_MAX = 0.5          # max_value of the "reward" form: tame rewards are ~1e-4, a patched box gives > 10

# rollouts (test 3d): the actor is [ns, ROLL_H, 1] relu / tanh; served: does the persistent launch take (case, dtype size)
ROLL_H = 20
ROLLOUT = ["wrap_nx100", "fmap_w3_nx100", "roll_nx320", "nx1024"]
RO_W = 32                        # csrc/roll_actor.hpp: the widest layer of the in-kernel actor


# ------------------------------------------------------------------ builders
def build(pkg, kg, case, **override):
    """(pkg.KellerSegelSetup, oracle KSegConfig) of a row, both from the same numbers"""
    c = CASES[case] if isinstance(case, str) else case
    c = c._replace(**override)
    pos, a2s = np.array(c.sensor_positions, dtype=np.int64), np.array(c.actuators_to_sensors, dtype=np.int64)
    both = dict(nx=c.nx, Lx=c.Lx, sensor_positions=pos, actuators_to_sensors=a2s, window_size=c.window_size,
                temporal_steps=c.temporal_steps, substeps=c.substeps, action_punish=c.action_punish,
                delta_action_punish=c.delta_action_punish, max_value=c.max_value)
    setup = pkg.KellerSegelSetup(integrator=c.integrator, check_max_value=c.check_max_value, **both)
    return setup, kg.KSegConfig(**both)


# sense_dots' 8-row unrolled body needs a chunk of >= 8 band rows per group.  The setup's boxes are 5 cells wide, so this one
# geometry widens them after construction on both sides (half window 10: 21 cells; 80 sensors on 100 cells: one group of 21 rows
# = two unrolled passes and a tail of 5).  The KS environment's Gaussians reach the same body at its own sizes.
WIDE_HALF_WINDOW = 10
WIDE = _case(100, range(11, 91), range(3, 80, 8))


def build_wide(pkg, kg):
    """(setup, oracle config) of WIDE with 21-cell boxes: KSegConfig takes the half window, the setup's tables are replaced"""
    c = WIDE
    pos, a2s = np.array(c.sensor_positions, dtype=np.int64), np.array(c.actuators_to_sensors, dtype=np.int64)
    both = dict(nx=c.nx, Lx=c.Lx, sensor_positions=pos, actuators_to_sensors=a2s, window_size=c.window_size,
                temporal_steps=c.temporal_steps, substeps=c.substeps)
    setup = pkg.KellerSegelSetup(**both)
    cfg = kg.KSegConfig(half_window=WIDE_HALF_WINDOW, **both)
    setup.gaussians = cfg.gaussians.copy()
    setup.gaussians_actuators = cfg.gaussians_actuators.copy()
    return setup, cfg


def inputs(case, B, steps=3, seed=0):
    """deterministic inputs of a row: y0 [B, 2, nx] = 1 + 0.05 randn (Julia layout), actions [steps, B, A] and the previous
    action [B, A] uniform in [-1, 1]"""
    c = CASES[case] if isinstance(case, str) else case
    rng = np.random.default_rng([seed, c.nx, len(c.actuators_to_sensors)])
    A = len(c.actuators_to_sensors)
    y0 = 1.0 + 0.05 * rng.standard_normal((B, 2, c.nx))
    return y0, rng.uniform(-1, 1, (steps, B, A)), rng.uniform(-1, 1, (B, A))


def oracle_step(kg, cfg, case, y, p):
    c = CASES[case] if isinstance(case, str) else case
    return kg.do_step_midpoint(cfg, y, p, c.substeps) if c.integrator == "midpoint" else kg.do_step(cfg, y, p, c.substeps)


def blown(x, max_value):
    """the blow-up predicate of the kernels: NOT every |x| <= max_value, so a NaN raises it (deviation from
    Julia's maximum(abs.(x)) > max_value, which a NaN leaves false)"""
    return not bool(np.all(np.abs(x) <= max_value))


def blowup_inputs(case, B=5):
    """inputs of test 3c: the tame ones, and a copy with u of trajectory 1 set beyond every max_value on its last three cells
    (40: after one control step the oracle's field is finite and still above 33; the same patch on v as well makes the oracle
    itself overflow within the step) and one NaN cell in trajectory 3"""
    y0, act, prev = inputs(case, B, steps=1, seed=7)
    bad = y0.copy()
    bad[1, 0, -3:] = 40.0
    bad[3, 0, bad.shape[2] // 2] = np.nan
    return y0, bad, act[0], prev


# ------------------------------------------------------------------ the host rules, restated
def nthreads(nx):
    return -(-nx // 64) * 64


def ring_window(mask, start=False):
    """length (and with start=True the first index) of the circular window pdec_env_create keeps of a 0/1 pattern: the ring
    minus its longest run of zeros, the first such run where several are as long"""
    m = np.asarray(mask, dtype=bool)
    n = len(m)
    if not m.any():
        return (0, 0) if start else 0
    if m.all():
        return (0, n) if start else n
    best = run = pos = 0
    for i in range(2 * n):
        run = 0 if m[i % n] else run + 1
        if run > best and run <= n:
            best, pos = run, i
    return ((pos + 1) % n, n - best) if start else n - best


def geometry(G, Ga, a2s, case):
    """what a row reaches, from the dense tables (setup.tables()) alone"""
    c = CASES[case] if isinstance(case, str) else case
    S, N = G.shape
    A = Ga.shape[0]
    nt = nthreads(N)
    Wd = max(1, max(ring_window(G[s] != 0) for s in range(S)))
    Cnt = max(1, max(ring_window(Ga[:, n] != 0) for n in range(N)))
    band = [ring_window(Ga[:, n] != 0, start=True) for n in range(N)]
    w = c.window_size // 2
    reads = np.array([[a2s[a] - i for i in range(-w, w + 1)] for a in range(A)])
    ng = min(max(nt // S, 1), 8)
    chunk = -(-Wd // ng)
    return dict(
        nthreads=nt, dead_lanes=nt - N, waves=nt // 64, last_cell_alone=(N % 64 == 1),
        S=S, A=A, ns=c.window_size * 2 * c.temporal_steps, fmap=(c.temporal_steps == 1),
        # the bands pdec_env_create builds
        Wd=Wd, Cnt=Cnt, cover=int((Ga != 0).sum(axis=0).max()), band_wraps=any(a0 + ln > A for a0, ln in band),
        last_cell_actuated=bool((Ga[:, -1] != 0).any()), first_cell_actuated=bool((Ga[:, 0] != 0).any()),
        # the sensor window of featurize
        wraps_low=bool((reads < 0).any()), wraps_high=bool((reads >= S).any()), monotone=bool(np.all(np.diff(a2s) > 0)),
        # sense_dots of the step kernels (nt threads; the stand-alone closures run it with 128)
        ng=ng, chunk=chunk, chunk_overshoots=bool(ng * chunk > Wd), unrolled_rows=8 * (chunk // 8))


def rollout_lds(geo, tsize, dims=None):
    """kseg_lds_bytes of csrc/kseg.hip + rollout_lds (Keller-Segel) of csrc/roll_actor.hpp for an actor of layer sizes `dims`"""
    N, S, A, ns = geo["nthreads"] - geo["dead_lanes"], geo["S"], geo["A"], geo["ns"]
    dims = [ns, ROLL_H, 1] if dims is None else dims
    step = (2 * (N + 2) + 2 * A + 2 * S + 16 * S + 16) * tsize
    image = (sum((d + 1) * RO_W for d in dims[:-1]) + 3) // 4 * 4
    return step + (2 * A * ns + 2 * A + image + 2 * A * RO_W) * tsize + 16


def rollout_served(geo, tsize, check_max_value="y"):
    return check_max_value != "reward" and max(geo["ns"], ROLL_H) <= RO_W and rollout_lds(geo, tsize) <= 64 * 1024
