"""Host model of the two-wave N = 256 engine (csrc/ks_engines.hpp, FftWave256x2) and of the rule that selects it
(csrc/env.hpp, ks_step_engine): the data flow of the kernel step by step on numpy arrays [register][thread], and the route as
a function of everything the launch reads.  Used by test_ks_two_wave_table.py; needs neither a GPU nor the library."""
import numpy as np

N, NT = 256, 128
TID = np.arange(NT)
LANE, WV = TID & 63, TID >> 6
TW = np.exp(-2j * np.pi * np.arange(N) / N)


def mode_index(j):
    k0 = WV + 2 * (LANE >> 5)
    k1 = ((LANE >> 4) & 1) + 2 * ((LANE >> 3) & 1)
    k2 = ((LANE >> 2) & 1) + 2 * ((LANE >> 1) & 1)
    k3 = (LANE & 1) + 2 * j
    return k0 + 4 * k1 + 16 * k2 + 64 * k3


def phys_index(j):
    return TID + NT * j


def level1(a):
    return np.stack([a[0] + a[1], a[0] - a[1]])


def level2(a, d, sgn):
    """d: the threads that hold the (d02, d13) pair; sgn < 0: -i, the forward transform"""
    r = np.where(d, (-1j if sgn < 0 else 1j) * a[1], a[1])
    return np.stack([a[0] + r, a[0] - r])


def xch(a, bit):
    """register bit <-> bit `bit` of the thread id (6: the wave bit, through LDS in the kernel)"""
    m = 1 << bit
    has = (TID & m) != 0
    out = a.copy()
    out[1] = np.where(has, a[1], a[0][TID ^ m])
    out[0] = np.where(has, a[1][TID ^ m], a[0])
    return out


KL = (WV, (LANE >> 4) & 1, (LANE >> 2) & 1)
LOW = (LANE, 4 * (LANE & 15), 16 * (LANE & 3))


def twiddle(a, st, sgn):
    w0, w1 = TW[(KL[st] * LOW[st]) & 255], TW[((KL[st] + 2) * LOW[st]) & 255]
    if sgn > 0:
        w0, w1 = w0.conj(), w1.conj()
    return np.stack([np.where(KL[st] == 1, a[0] * w0, a[0]), a[1] * w1])


D = {6: WV == 1, 4: (LANE & 16) != 0, 2: (LANE & 4) != 0, 0: (LANE & 1) != 0}


def forward(a):
    a = level2(xch(level1(a), 6), D[6], -1); a = twiddle(a, 0, -1)
    a = level2(xch(level1(xch(a, 5)), 4), D[4], -1); a = twiddle(a, 1, -1)
    a = level2(xch(level1(xch(a, 3)), 2), D[2], -1); a = twiddle(a, 2, -1)
    return level2(xch(level1(xch(a, 1)), 0), D[0], -1)


def inverse(a):
    a = level2(xch(level1(a), 0), D[0], +1)
    a = level2(xch(level1(twiddle(xch(a, 1), 2, +1)), 2), D[2], +1)
    a = level2(xch(level1(twiddle(xch(a, 3), 1, +1)), 4), D[4], +1)
    return level2(xch(level1(twiddle(xch(a, 5), 0, +1)), 6), D[6], +1)


# ---- the route (ks_step_engine + TrainPipeline): the ONE combination that reaches the two-wave kernel
AXES = dict(asked=(False, True), fused=(False, True), pde=("ks_cnab2", "ks_rk4_fd", "kseg"), N=(192, 256, 1024),
            dtype=("f32", "f64"), lds_fft=(False, True), generic_fft=(False, True), share=(False, True), mu=(False, True),
            faults=(False, True), member=(False, True))


def engine(N, lds_fft, generic_fft):
    """ks_pick_engine"""
    if generic_fft:
        return "Generic"
    if N == 256:
        return "LdsR4_256" if lds_fft else "Wave256"
    if N == 1024:
        return "LdsR4_1024" if lds_fft else "Wave1024"
    return {192: "Fixed192", 240: "Fixed240", 600: "Fixed600"}.get(N, "Generic")


def route(asked, fused, pde, N, dtype, lds_fft, generic_fft, share, mu, faults, member):
    e = engine(N, lds_fft, generic_fft) if pde == "ks_cnab2" else None
    two = (asked and fused and pde == "ks_cnab2" and e == "Wave256" and dtype == "f32" and not share and not mu and not faults
           and not member)
    return "Wave256x2" if two else e
