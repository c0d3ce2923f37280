"""The two device entry points a fluid population stands on (csrc/fluid_sense.hip): pdec_fluid_ic_dev, the episode initialiser from a
vortex table that is already in device memory, against pdec_fluid_ic bit for bit; and pdec_fluid_error_detection, the fluid
script's error_detection (scripts/Fluid/setup/FluidSetup.jl:263-273) per trajectory, against oracle.fluid.error_detection with
FluidSetup.error_detection as the second witness.

The detection cases keep every neighbour difference at least 0.4 away from the threshold 10 (jumps of 9.5 and 10.5 on a base
field whose own neighbour differences stay below 0.07), far above the fp32 transform error on fields of this size (about 1e-4
by the 1e-5-per-step figures of DESIGN 3.3), so the booleans are compared without a tolerance."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SIZES = (48, 64, 128)          # not a power of two; the generic transforms; the reference's grid
_SETUPS, _ENVS = {}, {}


def _env(pkg, n, dtype, B):
    if n not in _SETUPS:
        _SETUPS[n] = pkg.FluidSetup(nx=n, sensors_per_axis=4, oversampling=2)
    key = (n, dtype, B)
    if key not in _ENVS:
        _ENVS[key] = pkg.PDEenv(_SETUPS[n], B=B, dtype=dtype, autoreset=False)
    return _SETUPS[n], _ENVS[key]


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


# ---------------------------------------------------------------- pdec_fluid_ic_dev

@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("n", SIZES)
def test_ic_dev_equals_ic_bit_for_bit(pkg, n, dtype):
    B = 3
    setup, env = _env(pkg, n, dtype, B)
    _, one = _env(pkg, n, dtype, 1)
    P = pkg._lib.ptr
    for nv in (1, 2, 30):
        rng = np.random.default_rng(100 * n + nv)
        u = rng.random((B, nv, 4))
        v = np.ascontiguousarray(np.stack([u[..., 0] * setup.Lx, u[..., 1] * setup.Ly, setup.Lx / 20 * (0.5 + u[..., 2]),
                                           2 * u[..., 3] - 1], axis=-1))
        ref = torch.empty_like(env.y)
        pkg._lib.check(env.lib.pdec_fluid_ic(env.handle, v.ctypes.data_as(C.POINTER(C.c_double)), nv, P(ref)))
        vd = torch.from_numpy(v).cuda()
        got = torch.full_like(env.y, float("nan"))
        pkg._lib.check(env.lib.pdec_fluid_ic_dev(env.handle, P(vd), nv, P(got)))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
        assert torch.equal(_bits(got), _bits(ref)), (n, nv)
        assert not torch.equal(_bits(ref[0]), _bits(ref[1]))          # the trajectories' tables differ
        for b in range(B):                                            # trajectory b does not depend on the batch it sits in
            vb = vd[b:b + 1].contiguous()
            g1 = torch.full_like(one.y, float("nan"))
            pkg._lib.check(one.lib.pdec_fluid_ic_dev(one.handle, P(vb), nv, P(g1)))
            torch.cuda.synchronize()
            assert torch.equal(_bits(g1[0]), _bits(ref[b])), (n, nv, b)


def test_ic_dev_refuses_bad_arguments(pkg):
    _, env = _env(pkg, 48, torch.float64, 3)
    ks = pkg.PDEenv(pkg.KSSetup.KS22(), B=1, dtype=torch.float64)
    out = torch.empty_like(env.y)
    v = torch.ones((3, 1, 4), dtype=torch.float64, device="cuda:0")
    P = pkg._lib.ptr
    assert env.lib.pdec_fluid_ic_dev(env.handle, P(v), 0, P(out)) != 0
    assert env.lib.pdec_fluid_ic_dev(env.handle, None, 1, P(out)) != 0
    assert env.lib.pdec_fluid_ic_dev(ks.handle, P(v), 1, P(out)) != 0
    flags = torch.zeros(3, dtype=torch.int32, device="cuda:0")
    assert env.lib.pdec_fluid_error_detection(ks.handle, P(out), P(flags)) != 0
    assert env.lib.pdec_fluid_error_detection(env.handle, P(out), None) != 0


# ---------------------------------------------------------------- pdec_fluid_error_detection

def _cases(n):
    """[(name, physical field [n, n] in memory order (slow axis first), a spectrum edit or None, errored by construction)]"""
    i = np.arange(n)
    base = 0.5 * np.sin(2 * np.pi * i / n)[:, None] * np.cos(2 * np.pi * i / n)[None, :]      # neighbour differences < 0.07
    ramp = i / (n - 1.0)                                                                    # one jump: cell n - 1 against cell 0

    def band(h, axis, lo, hi):
        w = base.copy()
        sl = [slice(None), slice(None)]
        sl[axis] = slice(lo, hi)
        w[tuple(sl)] += h
        return w

    out = [("smooth", base, None, False)]
    for h, bad in ((10.5, True), (9.5, False)):
        out.append((f"slow axis {h}", band(h, 0, 5, 9), None, bad))
        out.append((f"fast axis {h}", band(h, 1, 7, 8), None, bad))
        out.append((f"slow seam {h}", base + h * ramp[:, None], None, bad))
        out.append((f"fast seam {h}", base + h * ramp[None, :], None, bad))
        last = base.copy()
        last[n - 3:n - 1, 3:n - 6] += h                      # both axes, inside the last row tile of the kernel's grid
        out.append((f"last tile {h}", last, None, bad))
    out.append(("nan entry", band(10.5, 0, 5, 9), float("nan"), False))
    out.append(("inf entry", band(10.5, 0, 5, 9), float("inf"), False))
    return out


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("n", SIZES)
def test_error_detection_matches_oracle_and_host(pkg, n, dtype):
    from oracle import fluid
    B = 5
    setup, env = _env(pkg, n, dtype, B)
    cases = _cases(n)
    while len(cases) % B:
        cases.append(cases[0])
    y_before = env.y.clone()
    state_before = env.featurize()
    seen = set()
    for c0 in range(0, len(cases), B):
        chunk = cases[c0:c0 + B]
        spec = []
        for name, w, edit, _ in chunk:
            z = torch.fft.fft2(torch.from_numpy(w))
            if edit is not None:
                z[3, 5] = complex(edit, 0.0)
            spec.append(torch.view_as_real(z))
        y = torch.stack(spec).to(dtype).cuda().contiguous()          # the environment's layout [B, nx, ny, 2]
        keep = y.clone()
        got = setup.error_detection_device(env, y)
        assert got.dtype == torch.bool and tuple(got.shape) == (B,)
        got = got.cpu().tolist()
        yh = y.cpu()
        want = [fluid.error_detection(torch.view_as_complex(yh[b].double().contiguous()).numpy().T) for b in range(B)]
        host = [setup.error_detection(y[b]) for b in range(B)]
        built = [bad for _, _, _, bad in chunk]
        print(n, dtype, [c[0] for c in chunk], got)
        assert want == built, [c[0] for c in chunk]                  # the witnesses see what the fields were built to hold
        assert host == want
        assert got == want, [c[0] for c in chunk]                    # per trajectory, not the batch's OR
        assert torch.equal(_bits(y), _bits(keep))                    # y is only read (NaN-safe comparison)
        seen.update(got)
    assert seen == {True, False}
    # the call used the sensing's work arrays and nothing else of the environment
    assert torch.equal(_bits(env.y), _bits(y_before))
    assert torch.equal(_bits(env.featurize()), _bits(state_before))
    # default argument: env.y
    assert setup.error_detection_device(env).cpu().tolist() == [setup.error_detection(env.y[b]) for b in range(B)]
