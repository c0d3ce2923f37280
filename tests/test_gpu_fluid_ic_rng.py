"""pdec_fluid_ic_rng: ic(3) / ic(4) of the fluid with the vortex table drawn on the device from the library's Philox stream
(csrc/fluid_sense.hip: fluid_vortex_draw_kernel, then the launches of pdec_fluid_ic_dev).

The table against the host restatement (tests/fluid_ic_ref.py on oracle.rng.words) within 1e-15 absolute -- its entries are single
fp64 products or sums of values in (0, 1.5), the margin allows a fused multiply-add --; the field bit for bit pdec_fluid_ic_dev
of the read-back table, and within the bounds tests/test_gpu_fluid.py (fp64: 1e-11 relative) and tests/test_gpu_fluid_fp32.py
(1e-6 relative) hold pdec_fluid_ic to against the oracle's vortex sum over the host table."""
import ctypes as C

import numpy as np
import pytest

from fluid_ic_ref import NV, fields_of, jul, pair, raw, vortex_table

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
SEED, OFF = 77, (1 << 33) + 5            # (the offset crosses into the counter's second word)
_REFS = {}


def _ref(pkg, n, caseno, B):
    """host table and the oracle's fields, once per (grid, case): the B = 3 ones, whose first trajectory is the B = 1 call's"""
    if (n, caseno) not in _REFS:
        _, cfg = pair(pkg, n)
        t = vortex_table(SEED, OFF, 3, caseno)
        _REFS[n, caseno] = (t, fields_of(cfg, t))
    t, f = _REFS[n, caseno]
    return t[:B], f[:B]


def _draw(pkg, env, caseno, seed=SEED, off=OFF, table=True):
    L = pkg._lib
    tab = torch.full((env.B, NV[caseno], 4), float("nan"), dtype=torch.float64, device="cuda:0") if table else None
    out = torch.empty_like(env.y)
    L.check(env.lib.pdec_fluid_ic_rng(env.handle, seed, off, caseno, L.ptr(tab), L.ptr(out)))
    torch.cuda.synchronize()
    return tab, out


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [32, 64])
@pytest.mark.parametrize("caseno", [3, 4])
def test_table_and_field(pkg, caseno, n, B, dt):
    L = pkg._lib
    setup, _ = pair(pkg, n)
    env = pkg.PDEenv(setup, B=B, dtype=dt)
    tab, out = _draw(pkg, env, caseno)
    href, fref = _ref(pkg, n, caseno, B)
    err = np.abs(tab.cpu().numpy() - href).max()
    print(f"case {caseno} n={n} B={B}: table max abs error {err:.3g}")
    assert err <= 1e-15
    # bit for bit pdec_fluid_ic_dev of the read-back table
    again = torch.empty_like(env.y)
    L.check(env.lib.pdec_fluid_ic_dev(env.handle, L.ptr(tab), NV[caseno], L.ptr(again)))
    torch.cuda.synchronize()
    assert raw(again) == raw(out)
    # ... without the copy of the table too
    _, out2 = _draw(pkg, env, caseno, table=False)
    assert raw(out2) == raw(out)
    got = jul(out)
    bound = 1e-11 if dt == torch.float64 else 1e-6
    for b in range(B):
        rel = np.abs(got[b] - fref[b]).max() / np.abs(fref[b]).max()
        print(f"  trajectory {b}: field rel. error {rel:.3g} (bound {bound})")
        assert rel <= bound, (b, rel)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("caseno", [3, 4])
def test_two_halves_draw_what_one_batch_draws(pkg, caseno, dt):
    setup, _ = pair(pkg, 32)
    nv = NV[caseno]
    whole, two = pkg.PDEenv(setup, B=4, dtype=dt), pkg.PDEenv(setup, B=2, dtype=dt)
    tw, yw = _draw(pkg, whole, caseno, off=OFF)
    for r in range(2):
        th, yh = _draw(pkg, two, caseno, off=OFF + r * 2 * nv)
        assert raw(th) == raw(tw[2 * r:2 * r + 2]) and raw(yh) == raw(yw[2 * r:2 * r + 2]), r


@pytest.mark.parametrize("evaluation", [False, True])
def test_env_random_init_is_the_entry(pkg, evaluation):
    """PDEenv.random_init on a fluid environment: ic(4) of an evaluation setup, else ic(3); returns B nv counters"""
    setup = pkg.FluidSetup(nx=32, sensors_per_axis=4, variance=0.08, oversampling=2, dt=2.0 / (16.0 * 32), evaluation=evaluation)
    env = pkg.PDEenv(setup, B=3, dtype=torch.float32)
    caseno = 4 if evaluation else 3
    out = torch.empty_like(env.y)
    tab = torch.empty((3, NV[caseno], 4), dtype=torch.float64, device="cuda:0")
    assert env.random_init(SEED, OFF, out=out, vortices_out=tab) == 3 * NV[caseno]
    assert env.random_init_coefficients() == 4 * NV[caseno]
    _, ref = _draw(pkg, env, caseno)
    assert raw(out) == raw(ref)
    assert np.abs(tab.cpu().numpy() - vortex_table(SEED, OFF, 3, caseno)).max() <= 1e-15


def test_refusals(pkg):
    L = pkg._lib
    setup, _ = pair(pkg, 32)
    env = pkg.PDEenv(setup, B=2, dtype=torch.float32)
    out = torch.empty_like(env.y)
    for caseno in (2, 5):
        with pytest.raises(pkg.PdecError, match=f"pdec_fluid_ic_rng: caseno {caseno}"):
            L.check(env.lib.pdec_fluid_ic_rng(env.handle, 1, 0, caseno, None, L.ptr(out)))
    with pytest.raises(pkg.PdecError, match="pdec_fluid_ic_rng: null y_out"):
        L.check(env.lib.pdec_fluid_ic_rng(env.handle, 1, 0, 3, None, None))
    ks = pkg.PDEenv(pkg.KSSetup.KS22(), B=2, dtype=torch.float32)
    with pytest.raises(pkg.PdecError, match="pdec_fluid_ic_rng: not a fluid env handle"):
        L.check(ks.lib.pdec_fluid_ic_rng(ks.handle, 1, 0, 3, None, L.ptr(out)))
    # pdec_env_random_init itself keeps refusing the fluid: it has no case argument
    with pytest.raises(pkg.PdecError, match="pdec_env_random_init"):
        L.check(env.lib.pdec_env_random_init(env.handle, 1, 0, L.ptr(out)))
