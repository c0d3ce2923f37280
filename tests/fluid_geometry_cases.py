"""The case table of test_gpu_fluid_geometry.py: geometries of the 2-D fluid environment (csrc/fluid_lds.hip: the LDS-tile kernels
fluid_k1/k2/k3_kernel and fluid_fft_fast/slow_kernel; csrc/fluid_wave.hip: the one-line-per-wave kernels
fluid_k1w/k2w/k2p/k3w/k31w_kernel on the seven WaveFft<E, Q, LB> plans and the fused integrator fluid_integrate_wave;
csrc/fluid_sense.hip: fluid_dots/feat/actuate_kernel) away from the grids the other fluid tests visit, plus a plain-Python
restatement of the host rules that decide what a geometry reaches (fluid_make and fluid_fused of csrc/fluid.hip, pick_tile, the plan
table fluid_wave_table with k2p_eligible and fluid_k2_launch, the batch parts of pdec_fluid_env_create, the LDS bytes of both families).
Imports numpy only, so test_fluid_geometry_table.py holds every claim of the table against the oracle and the setup's host tables
without a GPU; on the GPU the restated plan is held against the library's own (pdec_debug_fluid_plan) before a row runs.

Every row steps sub-steps of the reference's size, dt = K / (16 n) (h = dt / floor(16 nx dt), FluidSetup.jl:47): K sub-steps
spanning dt = 0.02 break the advective CFL limit and turn rounding into 1e-4 (test_gpu_fluid_fp32._pair).  The fused_* rows are
the exception: they take sub-steps HMUL_FUSED times that size, on a non-Hermitian spectrum with white noise up to the Nyquist
line and a forcing PSCALE_FUSED times the usual one, so that what one sub-step adds on the Nyquist line -- the line the
`j1 == j0` arm of fluid_k31w_kernel's stage loop computes on an un-padded grid -- and what a third sub-step adds to two are
above 1e-3 of max |result| (test_fluid_geometry_table.py asserts both), not at the floor a reference-sized sub-step leaves there.

Inputs (ic(4) fields, forcings, actions) are rounded to single precision for BOTH precisions: they are exact in fp64 too, and one
oracle result per row then serves the fp64 and the fp32 test.

Rounding estimates and measured GPU errors, relative to max |reference| (DESIGN.md 3.3 has the table): see ERRORS below."""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "n ifpad K B spa variance window tsteps herm hmul pscale run env")

HMUL_FUSED = 4.0          # sub-step of the fused_* rows, in units of the reference's 1 / (16 n)
PSCALE_FUSED = 40.0       # their forcing, in units of fft2(randn)
ENV_NAMES = ("PDEC_FLUID_FUSE", "PDEC_FLUID_K2P", "PDEC_FLUID_LDS_FFT", "PDEC_FLUID_SPLIT")


def _case(n, ifpad, K=2, B=2, spa=4, variance=0.08, window=3, tsteps=1, herm=True, hmul=1.0, pscale=1.0,
          run=("rhs", "step"), env=None):
    return Case(int(n), int(ifpad), int(K), int(B), int(spa), float(variance), int(window), int(tsteps), bool(herm), float(hmul),
                float(pscale), tuple(run), env)


_ALL = ("rhs", "step", "env")
_FUSED = dict(herm=False, hmul=HMUL_FUSED, pscale=PSCALE_FUSED, run=("step",))
_FUSED_RHS = dict(_FUSED, run=("rhs", "step"))             # rhs too: the un-fused launch list of the same plan with K2w

CASES = {
    # ---- the LDS-tile kernels with fewer than 16 lines per tile: rhs, do_step, closures and env step
    "lds_tl8_r5_160": _case(160, 1, run=_ALL),              # p = 240 = 2^4 3 5: TL 8 with a radix-5 stage, TLn 16
    "lds_tl8_192": _case(192, 1, run=_ALL),                 # p = 288: TL 8
    "lds_tl4_320": _case(320, 1, run=_ALL),                 # p = 480: TL 4, TLn 8; asks for the fused form, is not served
    "lds_tl2_540": _case(540, 1, run=_ALL),                 # p = 810 = 2 3^4 5: TL 2, TLn 4
    "lds_tl2_800": _case(800, 0, B=1, run=_ALL),            # p = 800: TL = TLn = 2, the un-padded LDS path
    # ---- the fused integrator
    "fused_unpadded_256": _case(256, 0, K=3, **_FUSED_RHS), # <4,1,6> + K2w, self-mirrored Nyquist line, repeated mode-4 K31
    "fused_unpadded_384": _case(384, 0, K=1, **_FUSED_RHS), # <2,3,6> + K2w; K = 1: no mode-4 K31
    "fused_k1_256": _case(256, 1, K=1, **_FUSED),           # K = 1 with K2p and tile-major W
    "fused_tiles_256": _case(256, 1, K=3, B=14, **_FUSED),  # 672 x-pass tiles: several per workgroup on W written by K31
    # ---- the un-fused wave integrator
    "wave_half_64": _case(64, 0, run=("step",)),            # <2,1,5>
    "wave_half_192": _case(128, 1, run=("step",)),          # <2,3,5>, pair = 0
    "wave_k2p_512": _case(512, 1, K=1, run=("step",)),      # <4,3,6>, K2p with 9 (fp64) / 5 (fp32) pieces per wave
    "wave_unpadded_128": _case(128, 0, run=("rhs", "step")),        # <2,1,6> with K2w, one line per wave without pairs
    "wave_unpadded_512": _case(512, 0, K=1, run=("rhs", "step")),   # <4,2,6> with K2w, un-fused
    # ---- sensing and actuation: closures and env step
    "sense_ragged_24": _case(24, 1, B=3, spa=3, variance=0.3, run=("env",)),          # S = 9, n % 16 != 0, box 17 of 24 cells
    "sense_spa2_40": _case(40, 1, B=3, spa=2, variance=0.3, run=("env",)),            # window wider than the sensor grid
    "sense_w5_40": _case(40, 0, B=3, spa=5, variance=0.15, window=5, run=("env",)),   # 25 state rows
    "sense_w1_t3_160": _case(160, 1, B=3, spa=4, variance=0.08, window=1, tsteps=3, run=("env",)),
    "sense_fullring": _case(16, 1, B=3, spa=4, variance=0.5, run=("env",)),           # every box as long as the ring
}

# ---- the documented switches: each value in a process of its own (the library reads a switch once per process)
SWITCH_CASES = {
    "k2p0_256": _case(256, 1, run=("rhs",), env=("PDEC_FLUID_K2P", "0")),            # fluid_k2w_kernel<T,2,3,4,6>
    "k2p0_512": _case(512, 1, run=("rhs",), env=("PDEC_FLUID_K2P", "0")),            # fluid_k2w_kernel<T,4,3,4,6>
    "fuse1_512_padded": _case(512, 1, run=("step",), env=("PDEC_FLUID_FUSE", "1")),
    "fuse1_512_unpadded": _case(512, 0, run=("step",), env=("PDEC_FLUID_FUSE", "1")),
    "fuse0_256": _case(256, 1, run=("step",), env=("PDEC_FLUID_FUSE", "0")),
    "ldsfft_128": _case(128, 1, run=("rhs", "step"), env=("PDEC_FLUID_LDS_FFT", "1")),
    "ldsfft_256": _case(256, 1, run=("rhs", "step"), env=("PDEC_FLUID_LDS_FFT", "1")),
    "ldsfft_512": _case(512, 1, run=("rhs", "step"), env=("PDEC_FLUID_LDS_FFT", "1")),
}
SWITCHES = [("PDEC_FLUID_K2P", "0"), ("PDEC_FLUID_FUSE", "1"), ("PDEC_FLUID_FUSE", "0"), ("PDEC_FLUID_LDS_FFT", "1")]
# PDEC_FLUID_K2P=0 against the default process: fluid_k2w_kernel and fluid_k2p_kernel evaluate the same expressions in the same
# order, so the right-hand sides are equal bit for bit (0) wherever the compiler contracts the multiply-adds of both alike -- all
# but <float,4,3,..>, where it does not (csrc/fluid_wave.hip above fluid_k2p_kernel).  There a result may differ by one rounding per
# butterfly level: 768 = 4^4 3 has five, three transforms and the product make 16 -> 16 x 2^-24 of max |rhs| (measured: 2.6).
K2P_VS_K2W = {("k2p0_256", "f64"): 0.0, ("k2p0_256", "f32"): 0.0, ("k2p0_512", "f64"): 0.0, ("k2p0_512", "f32"): 16 * 2.0 ** -24}

ALL_CASES = dict(CASES)
ALL_CASES.update(SWITCH_CASES)
PRECS = ("f64", "f32")

# ---- tolerances, relative to max |reference| (closures: to max(1, |reference|)): the project's own
TOL = {
    "f64": dict(rhs=1e-11, step=1e-11, closure=1e-12, env=1e-11),
    "f32": dict(rhs=2e-6, step=5e-6, closure=1e-5, env=1e-5, forcing=1e-6),
}
TOL["f64"]["forcing"] = TOL["f64"]["closure"]


def case_of(case):
    return ALL_CASES[case] if isinstance(case, str) else case


def switch_rows(var, value):
    return [n for n, c in SWITCH_CASES.items() if c.env == (var, value)]


# ------------------------------------------------------------------ builders
def dt_of(case):
    c = case_of(case)
    return c.K * c.hmul / (16.0 * c.n)


_BUILT, _INPUTS = {}, {}


def build(pkg, fluid, case):
    """(pkg.FluidSetup, oracle FluidConfig) of a row, both from the same numbers; memoised per geometry (rows that differ in
    their switch only share it)"""
    c = case_of(case)
    key = c._replace(env=None, run=None, B=0, herm=True, pscale=1.0)
    if key not in _BUILT:
        _BUILT[key] = _build(pkg, fluid, c)
    return _BUILT[key]


def _build(pkg, fluid, c):
    both = dict(nx=c.n, ifpad=c.ifpad, sensors_per_axis=c.spa, variance=c.variance, oversampling=c.K, dt=dt_of(c),
                window_size=c.window)
    setup = pkg.FluidSetup(temporal_steps=c.tsteps, **both)
    cfg = fluid.FluidConfig(**both)
    cfg.temporal_steps = c.tsteps
    return setup, cfg


def _f32(a):
    if np.iscomplexobj(a):
        return np.asarray(a).astype(np.complex64).astype(np.complex128)
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def inputs(fluid, cfg, case):
    """deterministic inputs of a row, every value exact in single precision: y [B, n, n] = ic(4) (oracle.fluid.ic; rows with
    herm = False add white noise of 5 % of max |y| on every mode, the Nyquist row and column included, as
    test_gpu_fluid._fields does), forcings p [B, n, n] = pscale fft2(randn), and for the env rows the previous action and
    tsteps actions uniform in [-1, 1], [B, 1, A].  Rows of one shape share their inputs."""
    c = case_of(case)
    key = c._replace(env=None, run=None, hmul=1.0)
    if key not in _INPUTS:
        _INPUTS[key] = _inputs(fluid, cfg, c)
    return _INPUTS[key]


def _inputs(fluid, cfg, c):
    rng = np.random.default_rng([c.n, c.ifpad, c.K, c.B, c.spa, c.window])
    y = np.stack([fluid.ic(cfg, 4, rng) for _ in range(c.B)])
    if not c.herm:
        y = y + 0.05 * np.abs(y).max() * (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape))
    p = c.pscale * np.stack([np.fft.fft2(rng.standard_normal((c.n, c.n))) for _ in range(c.B)])
    A = c.spa * c.spa
    a_prev = rng.uniform(-1, 1, (c.B, 1, A))
    acts = rng.uniform(-1, 1, (c.tsteps, c.B, 1, A))
    return dict(y=_f32(y), p=_f32(p), a_prev=_f32(a_prev), acts=_f32(acts))


_REF = {}


def reference(pkg, fluid, case):
    """setup, oracle config, inputs and the oracle's results of a row, computed once per process: rhs [B], step [B] (do_step of
    (y, p)), and for the env rows feat0 [B] (featurize at reset), and per control step t the lists pa, y, reward, state"""
    if case in _REF:
        return _REF[case]
    c = case_of(case)
    setup, cfg = build(pkg, fluid, case)
    x = inputs(fluid, cfg, case)
    r = dict(setup=setup, cfg=cfg, **x)
    if "rhs" in c.run:
        r["rhs"] = np.stack([fluid.rhs(cfg, x["y"][b].copy(), x["p"][b]) for b in range(c.B)])
    if "step" in c.run:
        r["step"] = np.stack([fluid.do_step(cfg, x["y"][b], x["p"][b], c.K) for b in range(c.B)])
    if "env" in c.run:
        r["feat0"] = [fluid.featurize(cfg, x["y"][b]) for b in range(c.B)]
        steps = []
        y, st, a_prev = list(x["y"]), list(r["feat0"]), list(x["a_prev"])
        for t in range(c.tsteps):
            s = dict(pa=[], y=[], reward=[], state=[])
            for b in range(c.B):
                a = x["acts"][t, b]
                pa = fluid.prepare_action(cfg, a)
                yn = fluid.do_step(cfg, y[b], pa, c.K)
                s["pa"].append(pa)
                s["y"].append(yn)
                s["reward"].append(fluid.reward_function(cfg, yn, a, a - a_prev[b]))
                s["state"].append(fluid.featurize(cfg, yn, st[b] if c.tsteps > 1 else None))
                y[b], st[b], a_prev[b] = yn, s["state"][-1], a
            steps.append(s)
        r["steps"] = steps
    _REF[case] = r
    return r


# ------------------------------------------------------------------ the host rules, restated
FL_NTH, FL_TILE_ELEMS = 1024, 3072       # csrc/fluid.hpp: FL_NTH, FL_NTH * FL_MAXE (TL * len <= 3072)
FL_K2_TC = 4                             # columns per workgroup of fluid_k2w_kernel
LDS_MAX = 160 * 1024
MAXPART = 4                              # PartStreams::MAX
# fluid_wave_table of csrc/fluid_wave.hip; test_fluid_geometry_table.py holds both lists against the library's own table
WAVE_PLANS = {768: (4, 3, 6), 512: (4, 2, 6), 256: (4, 1, 6), 384: (2, 3, 6), 128: (2, 1, 6), 192: (2, 3, 5), 64: (2, 1, 5)}
K2P_BUILT = {"f64": {(9, 8), (5, 4)}, "f32": {(5, 8), (3, 4)}}     # (NPW, NSU) of the table's K2p columns
PLAN_FIELDS = ("p", "nl", "TL", "TLn", "wave_E", "wave_Q", "wave_LB", "pair", "k2p", "fused", "nparts", "xtiles")


def pick_tile(length):
    t = 16
    while t > 1 and t * length > FL_TILE_ELEMS:
        t >>= 1
    return t


def fft_radices(length):
    """the prime factors make_fft_plan can use (2, 3, 5); None where the length has another"""
    out = []
    for r in (2, 3, 5):
        while length % r == 0:
            out.append(r)
            length //= r
    return out if length == 1 else None


def k2p_geom(nl, n, prec):
    """K2pGeom<16 | 8>: (DMA pieces per tile and field, pieces per wave NPW, output elements per thread NSU, elements per piece)"""
    zb = 16 if prec == "f64" else 8
    epl = 16 // zb
    lpl = 8 // epl
    lpp = 64 // lpl
    npieces = -(-nl // lpp)
    return npieces, -(-npieces // 8), n * 8 // 512, 64 * epl


def geometry(case, prec, env=None):
    """what a row reaches in one precision, from the table's own numbers; env: the switches of the process ({} = none set;
    default: the row's own)"""
    c = case_of(case)
    if env is None:
        env = dict([c.env]) if c.env else {}
    n, B = c.n, c.B
    p = n * 3 // 2 if c.ifpad else n
    nl = n + 1 if c.ifpad else n
    wave = None if "PDEC_FLUID_LDS_FFT" in env else WAVE_PLANS.get(p)
    E, Q, LB = wave if wave else (0, 0, 0)
    TL, TLn = pick_tile(p), pick_tile(n)
    zs = 16 if prec == "f64" else 8
    ts = zs // 2
    npieces, npw, nsu, piece = k2p_geom(nl, n, prec)
    want = env["PDEC_FLUID_K2P"][0] == "1" if "PDEC_FLUID_K2P" in env else n >= 256
    wave64 = bool(wave) and LB == 6
    k2p = bool(want and wave64 and p % 8 == 0 and c.ifpad and n * 8 % 512 == 0 and (npw, nsu) in K2P_BUILT[prec])
    fuse_asked = (env["PDEC_FLUID_FUSE"][0] == "1" if "PDEC_FLUID_FUSE" in env else 256 <= n < 512) and n >= 256
    fused = bool(fuse_asked and wave64)
    sp = env.get("PDEC_FLUID_SPLIT")
    nparts = int(sp) if sp is not None else (2 if (n >= 512 and B >= 8) else 0)
    nparts = 2 if nparts == 1 else nparts
    nparts = min(nparts, MAXPART, B)
    nparts = nparts if nparts >= 2 else 0
    pair = bool(wave) and n >= 256
    lpb = 4 * (64 >> LB) if wave else 0
    lds = dict(lds_p=(2 * TL * (p + 2) + p) * zs, lds_n=(2 * TLn * (n + 2) + n) * zs)
    if wave:
        lds.update(k1w=lpb * 2 * n * zs + n * ts, k2w=FL_K2_TC * (p + 1) * zs, k3w=lpb * n * zs, k31w=lpb * 2 * n * zs)
        if k2p:
            lds["k2p"] = (npieces * piece + n * 8 + ((Q - 1) * E if Q > 1 else 1) * 64) * zs
    rad_p, rad_n = fft_radices(p), fft_radices(n)
    return dict(
        p=p, nl=nl, TL=TL, TLn=TLn, wave=wave, wave_E=E, wave_Q=Q, wave_LB=LB, pair=int(pair), k2p=int(k2p), fused=int(fused),
        fuse_asked=bool(fuse_asked), nparts=nparts, xtiles=B * (p // 8) if k2p else 0, npw=npw if k2p else 0, nsu=nsu if k2p else 0,
        k2w=bool(wave) and not k2p, lds=lds, lds_max=max(lds.values()), tpl=FL_NTH // TL, tpl_n=FL_NTH // TLn,
        radix5=rad_p is not None and 5 in rad_p, factors=(rad_p is not None and rad_n is not None),
        family="wave" if wave else "lds", rhs_route=(E, Q, LB) if wave else "lds", step_route=(E, Q, LB) if fused else "loop", self_mirror=not c.ifpad, ragged16=n % 16 != 0, S=c.spa * c.spa,
        ns=c.window ** 2 * c.tsteps, window_revisits=c.window > c.spa, dots_idle_waves=(c.spa * c.spa) % 4 != 0,
        mode4_k31=max(c.K - 1, 0) if fused else 0)


def plan(case, prec, env=None):
    """the twelve numbers of pdec_debug_fluid_plan"""
    g = geometry(case, prec, env)
    return [int(g[k]) for k in PLAN_FIELDS]


# ---- rounding estimates (CPU) and measured errors (one MI355X), relative to max |reference|, for the geometries nobody had measured:
# padded lengths above 768, the radix-5 lengths, the fused integrator's new forms.  est: fp32 -- the oracle restated with
# single-precision FFTs and wavenumbers against the fp64 oracle; fp64 -- the oracle against itself on inputs perturbed by one ulp
# (largest of the first two trajectories).  gpu: the largest error of any trajectory.  The bound of a row is the project's
# tolerance (TOL); every measured error is below ten times its estimate AND below TOL, so no row needed a bound of its own.
#   row                  rhs: est f64 / gpu f64 / est f32 / gpu f32          do_step: est f64 / gpu f64 / est f32 / gpu f32
ERRORS = {
    "lds_tl8_r5_160":     dict(rhs=(5.8e-16, 6.1e-16, 3.2e-7, 2.2e-7), step=(1.9e-16, 2.2e-16, 5.3e-8, 1.6e-7)),
    "lds_tl8_192":        dict(rhs=(4.6e-16, 7.8e-16, 1.3e-7, 2.5e-7), step=(1.6e-16, 2.9e-16, 5.8e-8, 1.1e-7)),
    "lds_tl4_320":        dict(rhs=(3.7e-16, 9.0e-16, 3.3e-7, 2.2e-7), step=(1.7e-16, 2.3e-16, 5.9e-8, 1.5e-7)),
    "lds_tl2_540":        dict(rhs=(3.6e-16, 6.6e-16, 2.1e-7, 2.3e-7), step=(1.6e-16, 2.3e-16, 6.0e-8, 1.6e-7)),
    "lds_tl2_800":        dict(rhs=(2.7e-16, 8.6e-16, 1.2e-7, 2.0e-7), step=(1.5e-16, 1.5e-16, 4.1e-8, 1.8e-7)),
    "fused_unpadded_256": dict(rhs=(4.8e-16, 6.8e-16, 2.0e-7, 3.3e-7), step=(1.5e-16, 2.6e-16, 8.3e-8, 1.5e-7)),
    "fused_unpadded_384": dict(rhs=(5.1e-16, 8.8e-16, 1.5e-7, 3.4e-7), step=(1.6e-16, 1.4e-16, 3.5e-8, 7.3e-8)),
    "fused_k1_256":       dict(step=(1.6e-16, 1.5e-16, 3.8e-8, 7.8e-8)),
    "fused_tiles_256":    dict(step=(1.7e-16, 5.0e-16, 8.3e-8, 2.7e-7)),
}
