"""Host restatement of the fluid's device draw (pdec_fluid_ic_rng, include/pdeconv.h) and small helpers the fluid tests of the
terminal rows, the device draw and the pipeline share.  TEST INFRASTRUCTURE ONLY.

The draw: one Philox4x32-10 counter per (trajectory b, vortex v) = offset + b nv + v, its words w0..w3, u_i = (w_i + 0.5) 2^-32
in double; row (x0, y0, a0, U) = (u0 Lx, u1 Ly, a0, 2 u3 - 1) with a0 = Lx / 20 (ic(3), nv = 30) or (Lx / 20)(0.5 + u2) (ic(4),
nv = 50).  src/fluid_rk4.jl:72-120 with the library's stream in the place of the host's generator."""
import numpy as np

NV = {3: 30, 4: 50}


def vortex_table(seed, offset, B, caseno, Lx=1.0, Ly=None):
    """[B, nv, 4] float64 = (x0, y0, a0, U) as the device draws it"""
    from oracle import rng
    Ly = Lx if Ly is None else Ly
    nv = NV[caseno]
    w = rng.words(int(seed), int(offset), 4 * B * nv).astype(np.float64).reshape(B, nv, 4)
    u = (w + 0.5) * (1.0 / 4294967296.0)
    out = np.empty((B, nv, 4))
    out[..., 0] = u[..., 0] * Lx
    out[..., 1] = u[..., 1] * Ly
    out[..., 2] = (Lx / 20) if caseno == 3 else (Lx / 20) * (0.5 + u[..., 2])
    out[..., 3] = 2.0 * u[..., 3] - 1.0
    return out


def fields_of(cfg, table):
    """the oracle's vortex sum (oracle.fluid.taylorvtx, in table order) per trajectory: complex [B, ny, nx]"""
    from oracle import fluid
    out = []
    for rows in table:
        y = 0
        for x0, y0, a0, U in rows:
            y = y + fluid.taylorvtx(cfg, x0, y0, a0, U)
        out.append(y)
    return np.stack(out)


def mem(z):
    """Julia complex [.., ny, nx] -> memory [.., nx, ny, 2]"""
    z = np.swapaxes(np.asarray(z, dtype=np.complex128), -1, -2)
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1))


def jul(a):
    """memory [.., nx, ny, 2] (array or tensor) -> Julia complex [.., ny, nx] (complex128)"""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a, dtype=np.float64)
    return np.swapaxes(a[..., 0] + 1j * a[..., 1], -1, -2)


_PAIRS = {}


def pair(pkg, n, spa=4, **kw):
    """(product setup, oracle config) on the "physical" sub-step of tests/test_gpu_fluid_fp32.py::_pair: oversampling 2,
    dt = 2 / (16 n), variance 0.08; kw: max_value, check_max_value (setup), memoised"""
    from oracle import fluid
    key = (n, spa, tuple(sorted(kw.items())))
    if key not in _PAIRS:
        setup = pkg.FluidSetup(nx=n, sensors_per_axis=spa, variance=0.08, oversampling=2, dt=2.0 / (16.0 * n), **kw)
        cfg = fluid.FluidConfig(nx=n, sensors_per_axis=spa, variance=0.08, oversampling=2, dt=2.0 / (16.0 * n),
                                **({"max_value": kw["max_value"]} if "max_value" in kw else {}))
        _PAIRS[key] = (setup, cfg)
    return _PAIRS[key]


def raw(x):
    """the bytes of a tensor / array (NaN-safe equality)"""
    if hasattr(x, "detach"):
        x = x.detach().contiguous().cpu().numpy()
    return np.ascontiguousarray(x).tobytes()
