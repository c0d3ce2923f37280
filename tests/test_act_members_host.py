"""Host side of the member acting kernel (csrc/act_members.hip; population.py: act_members_tiles): the tile plan -- columns per
workgroup and workgroups per member from (columns per member, widest layer, bytes per element) -- restated in Python and
checked over the shipped actor shapes, and the C ABI of pdec_policy_act_members.  No GPU needed."""
import importlib
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = 48 * 1024


def _pop(pkg):
    return importlib.import_module(pkg.__name__ + ".population")


def _nna(pkg):
    return importlib.import_module(pkg.__name__ + ".nna")


def _shipped_actor_widths(pkg):
    """{name: widest layer (input included)} of the actors create_agent builds for Fluid_8 / 16 / 32 and the 2-D Keller-Segel
    setup, 2-layer as shipped and 3-layer (drop_middle_layer=False).  (Setups on a small grid: the actor's shape depends on the
    window, the temporal stack and nna_scale only.)"""
    out = {}
    setups = {"Fluid_8": pkg.FluidSetup.Fluid_8(nx=32), "Fluid_16": pkg.FluidSetup.Fluid_16(nx=32),
              "Fluid_32": pkg.FluidSetup.Fluid_32(nx=32), "KellerSegel2D": pkg.KellerSegel2DSetup(nx=64, ny=64)}
    for name, st in setups.items():
        ns = st.state_shape[0]
        for drop in (True, False):
            dims, _ = _nna(pkg).layer_spec(ns, 1, st.nna_scale, True, drop)
            out[f"{name}/{len(dims) - 1}"] = max(dims)
    return out


def test_tile_plan_covers_every_column_once_within_one_member_and_within_lds(pkg):
    tiles_of = _pop(pkg).act_members_tiles
    assert _pop(pkg).ACT_MEMBERS_LDS == LDS
    widths = _shipped_actor_widths(pkg)
    assert widths["Fluid_8/2"] == 18 and widths["KellerSegel2D/2"] == 36, widths
    cs = sorted(set(list(range(1, 200)) + [255, 256, 257, 319, 320, 321, 511, 512, 513, 1023, 1024, 1025, 4095, 4096]))
    for name, maxw in widths.items():
        for itemsize in (4, 8):
            for C in cs:
                tc, nt = tiles_of(C, maxw, itemsize)
                key = (name, itemsize, C)
                assert tc >= 64 and tc % 64 == 0, key
                assert 2 * maxw * tc * itemsize <= LDS, key
                # the largest multiple of 64 that fits, unless the member has fewer columns
                assert 2 * maxw * (tc + 64) * itemsize > LDS or tc == -(-C // 64) * 64, key
                assert tc <= -(-C // 64) * 64, key
                # tile t of member m: global columns m C + t tc ... + nc, nc = min(tc, C - t tc) -- every column of a member
                # exactly once, no tile beyond its member's block
                M = 3
                seen = np.zeros(M * C, dtype=np.int32)
                for m in range(M):
                    for t in range(nt):
                        c0, nc = t * tc, min(tc, C - t * tc)
                        assert nc >= 1, key
                        lo, hi = m * C + c0, m * C + c0 + nc
                        assert m * C <= lo and hi <= (m + 1) * C, key
                        seen[lo:hi] += 1
                assert (seen == 1).all(), key
    # a layer so wide that 64 columns do not fit: not served
    assert tiles_of(10, 97, 4) == (0, 0) and tiles_of(10, 96, 4)[0] == 64
    assert tiles_of(10, 49, 8) == (0, 0) and tiles_of(10, 48, 8)[0] == 64


def test_act_members_is_declared_bound_and_exported(pkg):
    """pdec_policy_act_members: the eight parameters of include/pdeconv.h, as many in ctypes and in the Julia ccall (type tuple and
    actual arguments), named in INTEGRATION.md, exported; pdec_rollout_members keeps its 18; the plan's debug entry is declared in
    pdeconv_debug.h only"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdeconv.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+pdec_policy_act_members\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)
    assert m, "pdec_policy_act_members is not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["pdec_handle env", "const pdec_handle* actors", "int M", "const void* state", "int cols_per_member",
                    "double act_limit", "void* actions_out", "int* served"]
    assert len(pkg._lib.SIGNATURES["pdec_policy_act_members"]) == 8
    m18 = re.search(r"\bint\s+pdec_rollout_members\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)
    assert m18 and len(m18.group(1).split(",")) == 18 and len(pkg._lib.SIGNATURES["pdec_rollout_members"]) == 18
    jl = open(os.path.join(ROOT, "julia", "PDEenvHIP.jl")).read()
    call = re.search(r"ccall\(\(:pdec_policy_act_members, LIB\),\s*Cint,\s*\((.*?)\),\s*(.*?)\)\)", jl, flags=re.S)
    assert call, "julia/PDEenvHIP.jl does not bind pdec_policy_act_members"
    assert len([a for a in call.group(1).replace("\n", " ").split(",") if a.strip()]) == 8
    assert len([a for a in call.group(2).replace("\n", " ").split(",") if a.strip()]) == 8
    assert "pdec_policy_act_members" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "pdec_debug_act_members_plan" not in hdr
    dbg = open(os.path.join(ROOT, "include", "pdeconv_debug.h")).read()
    assert re.search(r"\bint\s+pdec_debug_act_members_plan\s*\(", dbg)
    assert len(pkg._lib.DEBUG_SIGNATURES["pdec_debug_act_members_plan"]) == 6
    import ctypes
    lib = ctypes.CDLL(pkg._lib.LIB_PATH)
    assert hasattr(lib, "pdec_policy_act_members") and hasattr(lib, "pdec_debug_act_members_plan")


def test_batched_predicate_names_the_two_2d_setups_only(pkg):
    pop = _pop(pkg)
    assert pop._has_batched_rollout(pkg.FluidSetup(nx=32)) and pop._has_batched_rollout(pkg.KellerSegel2DSetup(nx=64, ny=64))
    assert not pop._has_batched_rollout(pkg.KSSetup.KS22()) and not pop._has_batched_rollout(pkg.KSSetup.KS22_global())
    assert not pop._has_batched_rollout(pkg.KellerSegelSetup())
    assert not pop._has_batched_rollout(pkg.FluidSetup(nx=32, memory_size=2))
    # the persistent predicate answers as before
    assert pop._has_persistent_rollout(pkg.KSSetup.KS22()) and not pop._has_persistent_rollout(pkg.FluidSetup(nx=32))
