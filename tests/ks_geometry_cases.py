"""The case table of test_gpu_ks_geometry.py: geometries of the Kuramoto-Sivashinsky environment (csrc/ks_step.hip: ks_env_step_kernel,
ks_rollout_kernel, ksfd_env_step_kernel, ksfd_wave_step_kernel, sense_kernel and their shared pieces sense_dots, actuate_cell(s),
actuate_consecutive, reward_traj / reward_pair, featurize_traj / featurize_pair, block_max, write_terminal, and the band tables
Wd / Cnt / sn0 / an0 / fmap / gsum of pdec_env_create) away from the three shipped layouts (KS22: 8 sensors every 24 cells, KS200:
80 every 3, bench_C2: every 4 -- identity actuators_to_sensors, A = S even, uniform spacing, no cell without an actuator), plus a
plain-Python restatement of the host rules that decide what a geometry reaches (work-group size, FFT engine, band widths in the
plan's dtype, sense_dots' grouping, the actuation branch, the LDS bills of the step and of the persistent rollout).  Imports numpy
only, so test_ks_geometry_table.py holds every claim of the table against oracle/ks.py and the setup's host tables without a GPU.

Every row keeps the shipped cell sizes dx = 200 / 240 (22 / 192 at 192 cells), so the oracle's step stays tame.  The reference
MULTIPLIES the Gaussian exponent by sigma^2 (KSSetup.jl:90), so a larger sigma is a NARROWER kernel."""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "nx Lx sensor_positions actuator_positions actuators_to_sensors sigma_sensors sigma_actuators window_size "
                          "temporal_steps mu action_punish delta_action_punish check_max_value max_value mono integrator precs")

DX = 200.0 / 240.0


def _case(nx, sensors, a2s=None, actuators=None, sigma=1.0, window_size=3, temporal_steps=1, mu=0.0, action_punish=0.002,
          delta_action_punish=0.002, check_max_value="y", max_value=30.0, mono=False, integrator="cnab2", Lx=None,
          precs=("f64", "f32")):
    sensors = tuple(int(s) for s in sensors)
    a2s = None if a2s is None else tuple(int(a) for a in a2s)
    if actuators is not None:
        actuators = tuple(int(a) for a in actuators)
    elif a2s is not None and not mono:           # a subset of the sensors acts: the actuators sit on their sensors (KSSetup.jl:113)
        actuators = tuple(sensors[a - 1] for a in a2s)
    return Case(int(nx), float(nx * DX if Lx is None else Lx), sensors, actuators, a2s, float(sigma), float(sigma), window_size,
                temporal_steps, mu, action_punish, delta_action_punish, check_max_value, max_value, mono, integrator, tuple(precs))


# the first 23 of np.random.default_rng(4).permutation(64) + 1, written out so that the row does not move with the generator; seed 4
# is the first whose 23 hold both sensor 1 and sensor 64: the window then wraps at both ends, and the blow-up patch on the last
# three cells lies under acting sensors, so the "reward" test sees it as well
PERM23 = (24, 58, 64, 42, 63, 35, 34, 12, 61, 27, 57, 19, 1, 56, 36, 41, 40, 43, 2, 14, 9, 48, 17)
IRREGULAR = (1, 2, 9, 30, 31, 77, 100, 128, 129, 200, 255, 256)     # adjacent sensors, and sensors on both sides of the seam
_S256 = range(1, 257, 4)
_PERM = dict(nx=256, sensors=_S256, a2s=PERM23)

CASES = {
    # ---- A != S, odd A, non-monotone a2s, punishments and the disturbance in the packed-pair step (FftWave256, consecutive).
    # mu = 0.05: a control step moves the field by dt mu = 0.005, so a disturbance of the wrong sign is off by 0.01 -- more than
    # 100 x the fp32 bound on y (KS200_disturbed.jl's 0.02 would clear it 74 times only)
    "perm_oddA_256": _case(**_PERM, mu=0.05, action_punish=0.3, delta_action_punish=0.7),
    # ---- narrow bands: one unrolled pass of sense_dots + tail / none; cells that no actuator reaches
    "narrow_256": _case(256, _S256, sigma=6.0, window_size=5),
    "narrower_256": _case(256, _S256, sigma=12.0, window_size=5),
    # ---- non-uniform sensors: FftWave256 with actuate_cells (2 N > 16 S), ng = 5 with an overshooting chunk
    "irregular_256": _case(256, IRREGULAR, a2s=(12, 1, 5, 6, 9), sigma=3.0),
    # ---- the other actuation branch of each compile-time engine, and of the generic one
    "dense_192": _case(192, range(1, 193, 4), sigma=0.7, window_size=5, Lx=22.0),
    "sparse_240": _case(240, range(1, 241, 30)),
    "sparse_600": _case(600, range(1, 601, 40)),
    "generic_60": _case(60, range(1, 61, 4), sigma=3.0),
    "subset_1024": _case(1024, range(1, 1025, 4), a2s=range(2, 256, 5), sigma=4.0),
    # ---- 1024 threads: ng = 4 with an overshooting chunk, at the largest grid of each dtype
    "ng4_4096": _case(4096, range(1, 4097, 16), precs=("f32",)),
    "ng4_2048": _case(2048, range(1, 2049, 16), precs=("f64",)),
    # ---- the global agent with A != S
    "mono_256": _case(256, range(1, 257, 8), actuators=range(3, 256, 20), mono=True),
    "mono_192_wide": _case(192, range(1, 193, 48), actuators=range(5, 193, 12), a2s=(np.arange(16) % 4) + 1, sigma=0.7, mono=True,
                           Lx=22.0),
    # ---- the general featurize path with a non-identity a2s
    "stack2_perm_256": _case(**_PERM, window_size=5, temporal_steps=2),
    # ---- the other blow-up tests.  max_value is also the sensor scale and a third of the reward's denominator (KSSetup.jl:169,
    # :201), so the "reward" row takes the default punishments and the smallest round bound that the tame rewards stay under by
    # a factor of two (test_ks_geometry_table.py holds it)
    "rewardcheck_256": _case(**_PERM, check_max_value="reward", max_value=5.0),
    "nocheck_256": _case(**_PERM, check_max_value="off"),
    # ---- the finite-difference twins: ksfd_wave_step_kernel (N = 256) and ksfd_env_step_kernel
    "fd_perm_256": _case(**_PERM, mu=0.02, action_punish=0.3, delta_action_punish=0.7, integrator="rk4_fd"),
    "fd_irregular_256": _case(256, IRREGULAR, a2s=(12, 1, 5, 6, 9), sigma=3.0, integrator="rk4_fd"),
    "fd_midpoint_100": _case(100, range(1, 101, 4), a2s=(25, 3, 17, 8, 1, 12, 21), sigma=6.0, mu=0.02, integrator="midpoint_fd"),
}

BLOWUP = ["perm_oddA_256", "irregular_256", "sparse_240", "mono_256", "rewardcheck_256", "nocheck_256", "fd_perm_256"]
BLOWUP_PATCH = 40.0              # trajectory 1's last three cells

# rollouts: the actor is [ns, H, 1] relu / tanh.  H = 20 where ks_rollout_lds stays under 64 KiB with it in both dtypes
# (perm_oddA_256 in fp64: 63.4 KB), 8 where only the narrower actor fits (A = S = 64 or 48 with window 5; 128 threads: the
# activation planes are 4 max(dims) nthreads elements)
RO_W = 32                        # csrc/roll_actor.hpp: the widest layer of the in-kernel actor
ROLL_H = {"narrow_256": 8, "narrower_256": 8, "dense_192": 8, "sparse_240": 8}
ROLL_H_DEFAULT = 20
ROLL_MUST_SERVE = ["perm_oddA_256", "narrow_256", "irregular_256", "dense_192", "sparse_240"]


def roll_h(case):
    return ROLL_H.get(case, ROLL_H_DEFAULT)


# ------------------------------------------------------------------ builders
def _get(case):
    return CASES[case] if isinstance(case, str) else case


def build(pkg, ks, case, **override):
    """(pkg.KSSetup, oracle KSConfig) of a row, both from the same numbers"""
    c = _get(case)._replace(**override)
    pos = np.array(c.sensor_positions, dtype=np.int64)
    both = dict(nx=c.nx, Lx=c.Lx, sensor_positions=pos,
                actuator_positions=None if c.actuator_positions is None else np.array(c.actuator_positions, dtype=np.int64),
                actuators_to_sensors=None if c.actuators_to_sensors is None else np.array(c.actuators_to_sensors, dtype=np.int64),
                sigma_sensors=c.sigma_sensors, sigma_actuators=c.sigma_actuators, mu=c.mu, max_value=c.max_value,
                action_punish=c.action_punish, delta_action_punish=c.delta_action_punish, window_size=c.window_size, mono=c.mono,
                temporal_steps=c.temporal_steps)
    setup = pkg.KSSetup(integrator=c.integrator, check_max_value=c.check_max_value, **both)
    return setup, ks.KSConfig(disturbance_in_step=not c.mono, **both)       # (KSglobalSetup.jl:167 has no disturbance term)


def n_actuators(case):
    c = _get(case)
    return len(c.sensor_positions if c.actuator_positions is None else c.actuator_positions)


def random_init(c, rng, B):
    """generate_random_init (KSSetup.jl:288-298), batched: eight sines with random weights, normalised to |y| = 30"""
    xx = (c.Lx / c.nx) * np.arange(1, c.nx + 1)
    a = rng.uniform(-1, 1, (B, 8))
    y0 = sum(a[:, i - 1:i] * np.sin(i * xx / (2 * np.pi))[None, :] for i in range(1, 9))
    return y0 * 30 / np.linalg.norm(y0, axis=1, keepdims=True)


def inputs(case, B, steps=3, seed=0):
    """deterministic inputs of a row: y0 [B, nx] = 0.15 generate_random_init, actions [steps, B, A] and the previous action
    [B, A] uniform in [-1, 1]"""
    c = _get(case)
    A = n_actuators(c)
    rng = np.random.default_rng([seed, c.nx, A])
    return 0.15 * random_init(c, rng, B), rng.uniform(-1, 1, (steps, B, A)), rng.uniform(-1, 1, (B, A))


def oracle_step(ks, cfg, case, y, p):
    c = _get(case)
    return {"cnab2": ks.do_step, "rk4_fd": ks.do_step_rk4_fd, "midpoint_fd": ks.do_step_midpoint_fd}[c.integrator](cfg, y, p)


def blown(x, max_value):
    """the blow-up predicate of the kernels: NOT every |x| <= max_value, so a NaN raises it (deviation from Julia's
    maximum(abs.(x)) > max_value, which a NaN leaves false)"""
    return not bool(np.all(np.abs(x) <= max_value))


def want_done(case, y, r):
    c = _get(case)
    return False if c.check_max_value == "off" else blown(r if c.check_max_value == "reward" else y, c.max_value)


def blowup_inputs(case, B=5):
    """inputs of the blow-up test: the tame ones, and a copy with trajectory 1 (the second half of pair 0) set to +40 on its last
    three cells and one NaN cell in trajectory 4 (the lone last one)"""
    y0, act, prev = inputs(case, B, steps=1, seed=7)
    bad = y0.copy()
    bad[1, -3:] = BLOWUP_PATCH
    bad[4, bad.shape[1] // 2] = np.nan
    return y0, bad, act[0], prev


# ------------------------------------------------------------------ the host rules, restated
ENGINES = {256: "FftWave256", 1024: "FftWave1024", 192: "FftFixed192", 240: "FftFixed240", 600: "FftFixed600"}
_FFT_BUFFERS = {"FftWave256": 1, "FftWave1024": 2, "FftR4": 2, "FftGeneric": 3, "FftFixed192": 3, "FftFixed240": 3, "FftFixed600": 3}


def nthreads(nx, integrator="cnab2"):
    if integrator != "cnab2":                   # the finite-difference kernels: one cell per thread; the fused step at 256 cells
        return 64 if nx == 256 else -(-nx // 64) * 64      # is ksfd_wave_step_kernel, one wave with four cells per lane
    return {192: 64, 240: 128, 600: 320}.get(nx, -(-(-(-nx // 4)) // 64) * 64)


def engine(nx):
    return ENGINES.get(nx, "FftGeneric")


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


def _ring_lengths(M):
    """ring_window's length for every row of a 0/1 matrix at once (n minus the longest circular run of zeros)"""
    M = np.asarray(M, dtype=bool)
    n = M.shape[1]
    out = np.zeros(M.shape[0], dtype=np.int64)
    for r, m in enumerate(M):
        if not m.any():
            continue
        if m.all():
            out[r] = n
            continue
        z = np.flatnonzero(m)
        gaps = np.diff(np.concatenate([z, [z[0] + n]])) - 1
        out[r] = n - gaps.max()
    return out


def geometry(G, Ga, a2s, case, prec="f64"):
    """what a row reaches, from the dense tables (setup.tables()) alone, for the plan's dtype: pdec_env_create counts an entry
    as non-zero if it is non-zero IN THAT DTYPE"""
    c = _get(case)
    if prec == "f32":
        G, Ga = G.astype(np.float32), Ga.astype(np.float32)
    S, N = G.shape
    A = Ga.shape[0]
    nt = nthreads(N, c.integrator)
    slen, alen = _ring_lengths(G != 0), _ring_lengths((Ga != 0).T)
    Wd, Cnt = max(1, int(slen.max())), max(1, int(alen.max()))
    cover = (Ga != 0).sum(axis=0)
    ng = min(max(nt // S, 1), 8)
    chunk = -(-Wd // ng)
    w = c.window_size // 2
    a2s = np.asarray(a2s)
    reads = np.array([[a2s[a] - i for i in range(-w, w + 1)] for a in range(A)])
    fft = c.integrator == "cnab2"
    consecutive = fft and N % 4 == 0 and 2 * N <= 16 * S
    ts = 8 if prec == "f64" else 4
    ns = S if c.mono else c.window_size * c.temporal_steps
    sense = (4 * A + 2 * S + 16 * S + 16) * ts
    lds = (_FFT_BUFFERS[engine(N)] * N * 2 * ts + sense) if fft else (2 * N + 4 + 2 * A + 2 * S + 16 * S + 16) * ts
    return dict(
        nthreads=nt, engine=engine(N) if fft else ("ksfd_wave" if N == 256 else "ksfd_lds"), S=S, A=A, ns=ns, mono=c.mono,
        fmap=(not c.mono and c.temporal_steps == 1),
        # the bands pdec_env_create builds
        Wd=Wd, Cnt=Cnt, min_cover=int(cover.min()), max_cover=int(cover.max()), uncovered=int((cover == 0).sum()),
        zero_rows=int(Cnt - alen.min()),
        # featurize's window and the actuator map
        wraps_low=bool((reads < 0).any()), wraps_high=bool((reads >= S).any()),
        monotone=bool(np.all(np.diff(a2s) > 0)), identity=bool(A == S and np.array_equal(a2s, np.arange(S))),
        repeated=bool(len(set(a2s.tolist())) < A),
        # sense_dots of the step kernels (nt threads; the stand-alone closures run it with 128)
        ng=ng, chunk=chunk, chunk_overshoots=bool(ng * chunk > Wd), unrolled_rows=8 * (chunk // 8), tail_rows=chunk % 8,
        ng_sense=min(max(128 // S, 1), 8),
        # the actuation branch of ks_env_step_kernel / ks_rollout_kernel
        consecutive=consecutive, cells=fft and not consecutive,
        lds_bytes=lds)


def with_engine(geo, case, prec, engine):
    """the geometry of a spectral row under PDEC_KS_LDS_FFT=1 ("FftR4", 256 / 1024 cells) or PDEC_KS_GENERIC_FFT=1 ("FftGeneric"):
    the work-group stays, the transform buffers (ENG::lds_complex) change"""
    N, ts = _get(case).nx, 8 if prec == "f64" else 4
    assert geo["engine"] in ("FftWave256", "FftWave1024") and geo["nthreads"] == N // 4
    return dict(geo, engine=engine, lds_bytes=geo["lds_bytes"] + (_FFT_BUFFERS[engine] - _FFT_BUFFERS[geo["engine"]]) * N * 2 * ts)


def ks_rollout_lds(geo, tsize, dims):
    """rollout_lds (KS) of csrc/roll_actor.hpp for an actor of layer sizes `dims` (geo of the same dtype)"""
    image = (sum((d + 1) * RO_W for d in dims[:-1]) + 3) // 4 * 4
    return geo["lds_bytes"] + (2 * geo["A"] * geo["ns"] + 4 * geo["A"] + image + 4 * max(dims) * geo["nthreads"]) * tsize + 16


def ks_rollout_shape_ok(geo, case, tsize, dims):
    c = _get(case)
    if c.integrator != "cnab2" or c.mono or c.temporal_steps != 1 or c.check_max_value == "reward":
        return False
    if geo["nthreads"] % 2 or not 1 <= len(dims) - 1 <= 3 or dims[-1] != 1 or dims[0] != geo["ns"] or max(dims) > RO_W:
        return False
    return ks_rollout_lds(geo, tsize, dims) <= 64 * 1024


def rollout_served(geo, case, prec):
    c = _get(case)
    name = case if isinstance(case, str) else None
    return ks_rollout_shape_ok(geo, c, 8 if prec == "f64" else 4, [geo["ns"], roll_h(name), 1])


# ------------------------------------------------------------------ the bounds of test_gpu_ks_geometry.py
UNIT = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}


def tol_y(prec, case, ref):
    c = _get(case)
    if c.integrator != "cnab2":          # test_rk4_fd_variant_matches_its_oracle: relative to max |ref|
        return (1e-11 if prec == "f64" else 2e-4) * float(np.abs(ref).max())
    return (1e-11 if prec == "f64" else 3e-5) * max(1.0, float(np.abs(ref).max()))      # test_every_fft_engine_and_size_limit


def tol_p(prec, ref):
    return (1e-12 if prec == "f64" else 1e-5) * max(1.0, float(np.abs(ref).max()))


def tol_state(prec, case, geo, ymax):
    """sensor dot / max_value at a given field, |y| <= ymax: a sum of Wd products g_j y_j with g_j >= 0, sum g_j = 1.  In ANY
    order of summation the computed sum is off by at most (Wd + 1) u sum |g_j y_j| <= (Wd + 1) u ymax (Wd - 1 additions and the
    product along the longest chain, the table entry's own rounding), the scale adds one more rounding: (Wd + 3) u ymax /
    max_value.  Twice that: the oracle's own fp64 sum carries the same bound in the fp64 comparison."""
    c = _get(case)
    return 2 * (geo["Wd"] + 3) * UNIT[prec] * ymax / c.max_value


def tol_reward(prec, case, geo, ymax):
    """r = -|6 d|^1.3 / (3 max_value) - ap a^2 - dp (a - a')^2 with the dot d off by e_d = (Wd + 2) u ymax (tol_state without the
    scale), |a|, |a'| <= 1:
      f'(ymax) e_d                         the dot's error through f(d) = (6 d)^1.3 / (3 max_value)
      9 u f(ymax)                          the scale by 6, pow (4 ulp), the division, the offset term
      1.3 u max(X^1.3 ln X, 0.29) / (3 mv) the exponent 1.3 rounded to the format, X = 6 ymax (x^1.3 |ln x| <= 0.29 below 1)
      3 u ap + 20 u dp                     each punishment: its factor, the square, the product (the difference, |a - a'| <= 2)
      2 u (f + ap + 4 dp)                  the two subtractions
    mono: the mean over A adds (A + 2) u of the largest term.  Twice the sum, as in tol_state."""
    c = _get(case)
    u, mv, X = UNIT[prec], c.max_value, 6 * ymax
    f = X ** 1.3 / (3 * mv)
    df = 1.3 * 6 ** 1.3 * ymax ** 0.3 / (3 * mv)
    big = f + c.action_punish + 4 * c.delta_action_punish
    t = df * (geo["Wd"] + 2) * u * ymax + 9 * u * f + 1.3 * u * max(X ** 1.3 * np.log(max(X, 1.0)), 0.29) / (3 * mv) \
        + 3 * u * c.action_punish + 20 * u * c.delta_action_punish + 2 * u * big
    if c.mono:
        t += (geo["A"] + 2) * u * big
    return 2 * t
