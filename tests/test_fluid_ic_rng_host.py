"""Host side of the fluid's device draw (pdec_fluid_ic_rng): the ranges of the restated vortex table, the entry's arity in the
header and in the ctypes binding, and the counters a fluid environment's random_init reports.  No GPU."""
import os
import re

import numpy as np
import pytest

from fluid_ic_ref import NV, vortex_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("caseno", [3, 4])
@pytest.mark.parametrize("Lx", [1.0, 2.5])
def test_ranges_of_the_restated_table(caseno, Lx):
    t = vortex_table(seed=9, offset=123456789012, B=40, caseno=caseno, Lx=Lx)
    assert t.shape == (40, NV[caseno], 4)
    assert (t[..., :2] > 0).all() and (t[..., :2] < Lx).all()
    if caseno == 3:
        assert (t[..., 2] == Lx / 20).all()
    else:
        assert (t[..., 2] > Lx / 40).all() and (t[..., 2] < 3 * Lx / 40).all() and t[..., 2].std() > 0.01 * Lx
    assert (t[..., 3] > -1).all() and (t[..., 3] < 1).all()
    assert abs(t[..., 3].mean()) < 0.1 and abs(t[..., 0].mean() - Lx / 2) < 0.05 * Lx
    # one counter per (trajectory, vortex): a batch is its trajectories' own stretches of the stream
    two = vortex_table(seed=9, offset=123456789012 + 7 * NV[caseno], B=2, caseno=caseno, Lx=Lx)
    assert np.array_equal(two, t[7:9])


def test_header_and_ctypes_name_the_entry(pkg):
    hdr = open(os.path.join(ROOT, "include", "pdeconv.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+pdec_fluid_ic_rng\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)
    assert m is not None
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 6 == len(pkg._lib.SIGNATURES["pdec_fluid_ic_rng"])
    assert [a.split()[-1].lstrip("*") for a in args] == ["h", "seed", "offset", "caseno", "vortices_out", "y_out"]
    import ctypes as C
    assert pkg._lib.SIGNATURES["pdec_fluid_ic_rng"][1:4] == [C.c_uint64, C.c_uint64, C.c_int]
    assert "pdec_fluid_ic_rng" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert len(pkg._lib.EnvCfg._fields_) == 30          # the case number is an argument, not a field


def test_random_init_coefficients_of_the_fluid(pkg):
    """4 nv uniforms per trajectory, so the rule B ceil(nc / 4) of the other kinds gives B nv counters"""
    PDEenv = pkg.PDEenv

    class _Env:            # random_init_coefficients reads the setup only
        is_fluid = True
    for evaluation, nc in ((False, 120), (True, 200)):
        e = _Env()
        e.setup = pkg.FluidSetup(nx=32, sensors_per_axis=4, oversampling=2, evaluation=evaluation)
        assert PDEenv.random_init_coefficients(e) == nc
