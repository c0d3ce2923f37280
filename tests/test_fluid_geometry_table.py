"""The case table of test_gpu_fluid_geometry.py (fluid_geometry_cases.py) held against the oracle and the setup's host tables.
Runs without a GPU: it proves that every row reaches what it is there for (the kernel family, the WaveFft plan, lines per LDS
tile, the persistent x-pass and its piece counts, the fused integrator and its fall-through, the sensing edges), that every
instantiation the plan table of csrc/fluid_wave.hip builds has a row (and that the table is the one restated here), that the inputs stay finite, tame and alive in the oracle itself
-- so the GPU test cannot pass on NaNs or on zeros -- that the inputs of the fused rows tell the self-mirror arm and the mode-4
chain apart, and it fails by name when a purpose of the table loses its row."""
import numpy as np
import pytest

import fluid_geometry_cases as fc
from oracle import fluid

ROWS = list(fc.ALL_CASES)


@pytest.fixture(scope="module")
def geo():
    return {(name, prec): fc.geometry(name, prec) for name in fc.ALL_CASES for prec in fc.PRECS}


def test_rows_say_what_their_names_say(geo):
    L = "lds"
    # name: (p, nl, TL, TLn, rhs route, do_step route, k2p, x-pass tiles, pair)
    want = {
        "lds_tl8_r5_160": (240, 161, 8, 16, L, "loop", 0, 0, 0),
        "lds_tl8_192": (288, 193, 8, 16, L, "loop", 0, 0, 0),
        "lds_tl4_320": (480, 321, 4, 8, L, "loop", 0, 0, 0),
        "lds_tl2_540": (810, 541, 2, 4, L, "loop", 0, 0, 0),
        "lds_tl2_800": (800, 800, 2, 2, L, "loop", 0, 0, 0),
        "fused_unpadded_256": (256, 256, 8, 8, (4, 1, 6), (4, 1, 6), 0, 0, 1),
        "fused_unpadded_384": (384, 384, 8, 8, (2, 3, 6), (2, 3, 6), 0, 0, 1),
        "fused_k1_256": (384, 257, 8, 8, (2, 3, 6), (2, 3, 6), 1, 96, 1),
        "fused_tiles_256": (384, 257, 8, 8, (2, 3, 6), (2, 3, 6), 1, 672, 1),
        "wave_half_64": (64, 64, 16, 16, (2, 1, 5), "loop", 0, 0, 0),
        "wave_half_192": (192, 129, 16, 16, (2, 3, 5), "loop", 0, 0, 0),
        "wave_k2p_512": (768, 513, 4, 4, (4, 3, 6), "loop", 1, 192, 1),
        "wave_unpadded_128": (128, 128, 16, 16, (2, 1, 6), "loop", 0, 0, 0),
        "wave_unpadded_512": (512, 512, 4, 4, (4, 2, 6), "loop", 0, 0, 1),
        "sense_ragged_24": (36, 25, 16, 16, L, "loop", 0, 0, 0),
        "sense_spa2_40": (60, 41, 16, 16, L, "loop", 0, 0, 0),
        "sense_w5_40": (40, 40, 16, 16, L, "loop", 0, 0, 0),
        "sense_w1_t3_160": (240, 161, 8, 16, L, "loop", 0, 0, 0),
        "sense_fullring": (24, 17, 16, 16, L, "loop", 0, 0, 0),
        "k2p0_256": (384, 257, 8, 8, (2, 3, 6), (2, 3, 6), 0, 0, 1),
        "k2p0_512": (768, 513, 4, 4, (4, 3, 6), "loop", 0, 0, 1),
        "fuse1_512_padded": (768, 513, 4, 4, (4, 3, 6), (4, 3, 6), 1, 192, 1),
        "fuse1_512_unpadded": (512, 512, 4, 4, (4, 2, 6), (4, 2, 6), 0, 0, 1),
        "fuse0_256": (384, 257, 8, 8, (2, 3, 6), "loop", 1, 96, 1),
        "ldsfft_128": (192, 129, 16, 16, L, "loop", 0, 0, 0),
        "ldsfft_256": (384, 257, 8, 8, L, "loop", 0, 0, 0),
        "ldsfft_512": (768, 513, 4, 4, L, "loop", 0, 0, 0),
    }
    assert set(want) == set(fc.ALL_CASES)
    for name, w in want.items():
        for prec in fc.PRECS:
            g = geo[name, prec]
            got = (g["p"], g["nl"], g["TL"], g["TLn"], g["rhs_route"], g["step_route"], g["k2p"], g["xtiles"], g["pair"])
            assert got == w, (name, prec, got)
            # what fluid_make refuses, and the twelve numbers of pdec_debug_fluid_plan
            assert g["factors"] and g["TL"] >= 2 and g["p"] <= 1536 and g["lds_max"] <= fc.LDS_MAX, (name, prec, g["lds"])
            assert g["nparts"] == 0 and len(fc.plan(name, prec)) == len(fc.PLAN_FIELDS) == 12
    # the pieces of the persistent x-pass differ by precision
    assert [(geo[n, pr]["npw"], geo[n, pr]["nsu"]) for n in ("wave_k2p_512", "fused_k1_256") for pr in fc.PRECS] == \
        [(9, 8), (5, 8), (5, 4), (3, 4)]
    # threads per line of tile_fft in the LDS rows
    assert {n: (geo[n, "f64"]["tpl"], geo[n, "f64"]["tpl_n"]) for n in fc.CASES if n.startswith("lds_")} == {
        "lds_tl8_r5_160": (128, 64), "lds_tl8_192": (128, 64), "lds_tl4_320": (256, 128), "lds_tl2_540": (512, 256),
        "lds_tl2_800": (512, 512)}
    assert fc.fft_radices(240) == [2, 2, 2, 2, 3, 5] and fc.fft_radices(810) == [2, 3, 3, 3, 3, 5] and fc.fft_radices(288).count(5) == 0
    assert geo["lds_tl4_320", "f64"]["fuse_asked"] and not geo["lds_tl4_320", "f64"]["fused"]
    # several x-pass tiles per workgroup: more tiles than twice the CUs of an MI355X (the fp32 grid of fluid_k2_launch)
    assert geo["fused_tiles_256", "f32"]["xtiles"] == 672 > 2 * 256
    assert [geo[n, "f64"]["mode4_k31"] for n in ("fused_unpadded_256", "fused_unpadded_384", "fused_k1_256", "fused_tiles_256")] == \
        [2, 0, 0, 2]
    # the switch rows are what their switch makes them: the same geometry with no switch set goes the default way
    none = {(n, pr): fc.geometry(n, pr, env={}) for n in fc.SWITCH_CASES for pr in fc.PRECS}
    for pr in fc.PRECS:
        assert none["k2p0_256", pr]["k2p"] and none["k2p0_512", pr]["k2p"]
        assert not none["fuse1_512_padded", pr]["fused"] and not none["fuse1_512_unpadded", pr]["fused"] and none["fuse0_256", pr]["fused"]
        assert [none[n, pr]["rhs_route"] for n in ("ldsfft_128", "ldsfft_256", "ldsfft_512")] == [(2, 3, 5), (2, 3, 6), (4, 3, 6)]
    assert sorted(set(c.env for c in fc.SWITCH_CASES.values())) == sorted(fc.SWITCHES)
    assert all(c.env is None for c in fc.CASES.values()) and set(fc.K2P_VS_K2W) == {(n, pr) for n in fc.switch_rows("PDEC_FLUID_K2P", "0") for pr in fc.PRECS}
    # sub-steps: the reference's size everywhere but in the fused rows
    for name, c in fc.ALL_CASES.items():
        assert c.hmul == (fc.HMUL_FUSED if name.startswith("fused_") else 1.0), name
        assert abs(fc.dt_of(name) / c.K * 16 * c.n - c.hmul) < 1e-12
        assert c.n % c.spa == 0 and (c.spa <= 4 or c.n <= 256) and (c.B <= 2 or c.n <= 256)
    # the restated rules at the shapes the other fluid tests and the benchmark run, for the record
    assert [fc.pick_tile(x) for x in (16, 192, 193, 384, 385, 768, 769, 1536)] == [16, 16, 8, 8, 4, 4, 2, 2]
    assert fc.k2p_geom(513, 512, "f64")[:3] == (65, 9, 8) and fc.k2p_geom(513, 512, "f32")[:3] == (33, 5, 8)
    assert fc.k2p_geom(257, 256, "f64")[:3] == (33, 5, 4) and fc.k2p_geom(257, 256, "f32")[:3] == (17, 3, 4)


# ---- every purpose of the table, by name: (what it is there for, predicate over a row's geometry in one precision and its case)
def _runs(c, what):
    return what in c.run


def _rhs_launch(plan):      # an un-fused right-hand side on this plan: env.rhs, or a do_step that takes the plain loop
    return lambda g, c, pr: g["rhs_route"] == plan and (_runs(c, "rhs") or ((_runs(c, "step") or _runs(c, "env")) and g["step_route"] == "loop"))


def _integrate(plan):       # fluid_integrate_wave on this plan
    return lambda g, c, pr: g["step_route"] == plan and (_runs(c, "step") or _runs(c, "env"))


def _k2w(plan):
    return lambda g, c, pr: g["rhs_route"] == plan and g["k2w"]


def _k2p(prec, npw, nsu):
    return lambda g, c, pr: pr == prec and g["k2p"] and (g["npw"], g["nsu"]) == (npw, nsu)


def _lds_tile(key, t):      # the LDS family at this tile size: the padded passes (TL) or the n x n passes of the closures (TLn)
    if key == "TL":
        return lambda g, c, pr: g["family"] == "lds" and g["TL"] == t and (_runs(c, "rhs") or _runs(c, "step") or _runs(c, "env"))
    return lambda g, c, pr: g["TLn"] == t and _runs(c, "env")


WAVE = sorted(fc.WAVE_PLANS.values())
FUSABLE = [pl for pl in WAVE if pl[2] == 6 and pl != (2, 1, 6)]
PURPOSES = {}
for _pl in WAVE:
    PURPOSES["fluid_rhs_launch_wave<T,%d,%d,%d>" % _pl] = _rhs_launch(_pl)
    PURPOSES["fluid_k2w_kernel<T,%d,%d,4,%d>" % _pl] = _k2w(_pl)
for _pl in FUSABLE:
    PURPOSES["fluid_integrate_wave<T,%d,%d,%d>" % _pl] = _integrate(_pl)
PURPOSES.update({
    "fluid_k2p_kernel<double,4,3,9,8>": _k2p("f64", 9, 8), "fluid_k2p_kernel<double,2,3,5,4>": _k2p("f64", 5, 4),
    "fluid_k2p_kernel<float,4,3,5,8>": _k2p("f32", 5, 8), "fluid_k2p_kernel<float,2,3,3,4>": _k2p("f32", 3, 4),
})
for _t in (16, 8, 4, 2):
    PURPOSES["LDS-tile kernels, TL %d" % _t] = _lds_tile("TL", _t)
    PURPOSES["fluid_fft_fast/slow_kernel, TLn %d" % _t] = _lds_tile("TLn", _t)
PURPOSES.update({
    "radix-5 stage with fewer than 16 lines per tile": lambda g, c, pr: g["family"] == "lds" and g["radix5"] and g["TL"] < 16 and _runs(c, "step"),
    "radix-5 stage with 2 lines per tile": lambda g, c, pr: g["family"] == "lds" and g["radix5"] and g["TL"] == 2,
    "un-padded LDS path": lambda g, c, pr: g["family"] == "lds" and not c.ifpad and g["TL"] == 2,
    "fused form asked for and not served": lambda g, c, pr: g["fuse_asked"] and not g["fused"] and c.env is None and _runs(c, "step"),
    "fused, un-padded: self-mirrored Nyquist line": lambda g, c, pr: g["fused"] and g["self_mirror"] and not c.herm and c.env is None,
    "fused with K = 1: no mode-4 K31": lambda g, c, pr: g["fused"] and c.K == 1 and c.env is None,
    "fused with K = 1 on tile-major W": lambda g, c, pr: g["fused"] and c.K == 1 and g["k2p"] and c.env is None,
    "fused with K >= 3: repeated mode-4 K31": lambda g, c, pr: g["fused"] and g["mode4_k31"] >= 2,
    "fused with several x-pass tiles per workgroup": lambda g, c, pr: g["fused"] and g["xtiles"] > 512 and c.K >= 2,
    "do_step on a half-wave plan, p = 64": lambda g, c, pr: g["rhs_route"] == (2, 1, 5) and _runs(c, "step"),
    "do_step on a half-wave plan, p = 192": lambda g, c, pr: g["rhs_route"] == (2, 3, 5) and _runs(c, "step") and g["pair"] == 0,
    "un-fused do_step with K2p at n = 512": lambda g, c, pr: g["step_route"] == "loop" and g["k2p"] and c.n == 512 and _runs(c, "step") and c.env is None,
    "window 5": lambda g, c, pr: c.window == 5 and g["ns"] == 25,
    "window 1 with three stacked steps": lambda g, c, pr: (c.window, c.tsteps, g["ns"]) == (1, 3, 3),
    "fewer sensors per axis than the window": lambda g, c, pr: g["window_revisits"] and _runs(c, "env"),
    "grid no multiple of 16": lambda g, c, pr: g["ragged16"] and _runs(c, "env"),
    "sensor count no multiple of 4": lambda g, c, pr: g["dots_idle_waves"] and _runs(c, "env"),
    "PDEC_FLUID_K2P=0 at n = 256 and 512": lambda g, c, pr: c.env == ("PDEC_FLUID_K2P", "0") and c.n == 512 and g["k2w"],
    "PDEC_FLUID_FUSE=1 at n = 512, padded": lambda g, c, pr: c.env == ("PDEC_FLUID_FUSE", "1") and g["step_route"] == (4, 3, 6),
    "PDEC_FLUID_FUSE=1 at n = 512, un-padded": lambda g, c, pr: c.env == ("PDEC_FLUID_FUSE", "1") and g["step_route"] == (4, 2, 6),
    "PDEC_FLUID_FUSE=0 at n = 256": lambda g, c, pr: c.env == ("PDEC_FLUID_FUSE", "0") and c.n == 256 and g["step_route"] == "loop",
    "PDEC_FLUID_LDS_FFT=1, TL 16": lambda g, c, pr: c.env == ("PDEC_FLUID_LDS_FFT", "1") and g["family"] == "lds" and g["TL"] == 16,
    "PDEC_FLUID_LDS_FFT=1, TL 8": lambda g, c, pr: c.env == ("PDEC_FLUID_LDS_FFT", "1") and g["family"] == "lds" and g["TL"] == 8,
    "PDEC_FLUID_LDS_FFT=1, TL 4": lambda g, c, pr: c.env == ("PDEC_FLUID_LDS_FFT", "1") and g["family"] == "lds" and g["TL"] == 4,
})


@pytest.mark.parametrize("purpose", list(PURPOSES))
def test_every_purpose_has_its_row(geo, purpose):
    hit = [(n, pr) for n in fc.ALL_CASES for pr in fc.PRECS if PURPOSES[purpose](geo[n, pr], fc.ALL_CASES[n], pr)]
    assert hit, f"no row of fluid_geometry_cases is there for: {purpose}"


def test_the_fused_form_of_the_128_point_plan_cannot_be_reached():
    """the plan table (csrc/fluid_wave.hip) builds no fluid_integrate_wave<T,2,1,6> (p = 128): the fused form needs n >= 256 and
    p >= n, so no geometry would reach it under any switch -- the one-line-per-wave plan that FUSABLE leaves out"""
    for n in range(8, 1025, 4):
        for ifpad in (0, 1):
            c = fc._case(n, ifpad, env=("PDEC_FLUID_FUSE", "1"))
            if fc.fft_radices(n) is None or fc.fft_radices(n * 3 // 2 if ifpad else n) is None:
                continue
            assert fc.geometry(c, "f64")["step_route"] != (2, 1, 6)


def test_the_librarys_plan_table_is_the_restated_one(pkg):
    """fluid_wave_table of csrc/fluid_wave.hip, read through pdec_debug_fluid_wave_table (host code: no device, no handle),
    is WAVE_PLANS; its K2p columns are K2P_BUILT, on the rows p = 768 and p = 384 and nowhere else, each with the pieces K2pGeom
    gives for n = 512 / n = 256; its fused column is FUSABLE; and the instantiation names of PURPOSES are its built cells,
    one for one -- so a plan added to or dropped from the library fails here until the restated lists follow"""
    import ctypes
    lib = ctypes.CDLL(pkg._lib.LIB_PATH)
    fn = lib.pdec_debug_fluid_wave_table
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.POINTER(ctypes.c_int32), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    nrows = ctypes.c_int(-1)
    assert fn(None, 0, ctypes.byref(nrows)) != 0 and nrows.value == len(fc.WAVE_PLANS)        # no room: refused, the count told
    per = 14
    buf = (ctypes.c_int32 * (per * nrows.value))()
    short = (ctypes.c_int32 * (per * nrows.value))()
    assert fn(short, per * nrows.value - 1, ctypes.byref(nrows)) != 0 and not any(short)      # one number short: nothing written
    assert fn(buf, len(buf), ctypes.byref(nrows)) == 0 and nrows.value == len(fc.WAVE_PLANS)
    rows = [list(buf[per * i:per * (i + 1)]) for i in range(nrows.value)]
    assert len({r[0] for r in rows}) == len(rows) and {r[0]: tuple(r[1:4]) for r in rows} == fc.WAVE_PLANS
    k2p_rows = {768: 512, 384: 256}                                                           # p: the padded grid's n
    ctype = {"f64": "double", "f32": "float"}
    names = set()
    for r in rows:
        p, plan = r[0], tuple(r[1:4])
        cells = dict(zip(fc.PRECS, (r[4:9], r[9:14])))
        for prec, (rhs, fused, k2p, npw, nsu) in cells.items():
            assert rhs == 1, (p, prec)                                                        # all seven plans of K1w, K2w and K3w
            assert fused == int(plan in FUSABLE), (p, prec)
            assert k2p == int(p in k2p_rows) and (bool(k2p) or (npw, nsu) == (0, 0)), (p, prec)
            if k2p:
                n = k2p_rows[p]
                assert (npw, nsu) == fc.k2p_geom(n + 1, n, prec)[1:3] and (npw, nsu) in fc.K2P_BUILT[prec], (p, prec)
                names.add("fluid_k2p_kernel<%s,%d,%d,%d,%d>" % (ctype[prec], plan[0], plan[1], npw, nsu))
        assert cells["f64"][:3] == cells["f32"][:3]                                           # the names with T: both dtypes
        names.add("fluid_rhs_launch_wave<T,%d,%d,%d>" % plan)
        names.add("fluid_k2w_kernel<T,%d,%d,%d,%d>" % (plan[0], plan[1], fc.FL_K2_TC, plan[2]))
        if cells["f64"][1]:
            names.add("fluid_integrate_wave<T,%d,%d,%d>" % plan)
    for prec in fc.PRECS:
        assert {tuple(r[7:9] if prec == "f64" else r[12:14]) for r in rows if r[0] in k2p_rows} == fc.K2P_BUILT[prec]
    assert names == {k for k in PURPOSES if "<" in k}


# ------------------------------------------------------------------ the setup's tables are the oracle's
def _dense(boxes, origin, n):
    """[S][BW][BH] boxes at (j0, i0) -> dense [S][ny, nx] kernels"""
    S, BW, BH = boxes.shape
    out = np.zeros((S, n, n))
    for s in range(S):
        j0, i0 = origin[s]
        ii, jj = (i0 + np.arange(BH)) % n, (j0 + np.arange(BW)) % n
        np.add.at(out[s], np.ix_(ii, jj), boxes[s].T)
    return out


@pytest.mark.parametrize("case", list(fc.CASES))
def test_setup_tables_are_the_oracles(pkg, case):
    c = fc.CASES[case]
    setup, cfg = fc.build(pkg, fluid, case)
    g = fc.geometry(case, "f64")
    e = setup.env_cfg(c.B, 0)
    assert (e.N, e.B, e.S, e.A, e.window, e.temporal_steps, e.K, e.ifpad, e.sensors_per_axis, e.memory_size) == \
        (c.n, c.B, g["S"], g["S"], c.window, c.tsteps, c.K, c.ifpad, c.spa, 0)
    assert (e.dt, e.Lx, e.nu, e.max_value, e.agent_power) == (cfg.dt, cfg.Lx, cfg.nu, cfg.max_value, cfg.agent_power) and e.dt == fc.dt_of(case)
    assert (e.action_punish, e.delta_action_punish, e.check_max_value) == (cfg.action_punish, cfg.delta_action_punish, 2)
    assert (e.sensor_scale, e.reward_power, e.reward_denom) == (1.0 / 70.0, 1.1, 320.0)          # FluidSetup.jl:216, :197
    assert setup.oversampling == cfg.oversampling == c.K and setup.state_shape == (g["ns"], g["S"])
    assert setup.sensor_positions == cfg.sensor_positions and len(cfg.sensor_positions) == g["S"]
    sb, so, ab, ao, BH, BW, a2s = setup.box_tables()
    assert list(a2s) == list(range(g["S"])) and 1 <= BH <= c.n and 1 <= BW <= c.n
    assert np.abs(_dense(sb, so, c.n) - cfg.gaussians).max() <= 1e-15
    assert np.abs(_dense(ab, ao, c.n) - cfg.gaussians_actuators).max() <= 1e-15
    assert (cfg.gaussians.reshape(g["S"], -1) != 0).any(axis=1).all()
    if case == "sense_ragged_24":
        assert (BH, BW) == (17, 17)
    if case == "sense_fullring":
        assert (BH, BW) == (c.n, c.n)                    # a box as long as the ring, along both axes


# ------------------------------------------------------------------ the inputs in the oracle
@pytest.mark.parametrize("case", ROWS)
def test_inputs_stay_finite_tame_and_alive_in_the_oracle(pkg, case):
    c = fc.ALL_CASES[case]
    r = fc.reference(pkg, fluid, case)
    y, p = r["y"], r["p"]
    assert y.shape == p.shape == (c.B, c.n, c.n) and len({y[b].tobytes() for b in range(c.B)}) == c.B
    for a in (y, p, r["a_prev"], r["acts"]):             # exact in single precision
        assert np.array_equal(a, fc._f32(a))
    assert np.abs(r["acts"]).max() <= 1 and np.abs(r["a_prev"]).max() <= 1
    herm = max(np.abs(np.fft.ifft2(y[b]).imag).max() / np.abs(np.fft.ifft2(y[b]).real).max() for b in range(c.B))
    assert (herm < 1e-6) == c.herm
    for b in range(c.B):
        if "rhs" in c.run:
            assert np.isfinite(r["rhs"][b]).all() and np.abs(r["rhs"][b]).max() > 0
        if "step" in c.run:
            s = r["step"][b]
            assert np.isfinite(s).all()
            n0, n1 = np.linalg.norm(y[b]), np.linalg.norm(s)
            assert abs(n1 / n0 - 1) < (0.02 if c.hmul == 1 else 0.2), (b, n1 / n0)         # alive, and no blow-up under way
            assert np.abs(s - y[b]).max() > 1e-6 * np.abs(s).max()                         # and the step did something
    if "env" in c.run:
        for b in range(c.B):
            assert np.isfinite(r["feat0"][b]).all() and np.abs(r["feat0"][b]).max() > 1e-4
            assert r["feat0"][b].shape == (fc.geometry(case, "f64")["ns"], c.spa * c.spa)
        for t, s in enumerate(r["steps"]):
            for b in range(c.B):
                yn, rew, st = s["y"][b], s["reward"][b], s["state"][b]
                assert np.isfinite(yn).all() and np.isfinite(rew).all() and np.isfinite(st).all()
                # far inside the blow-up bound (check_max_value = "reward", max_value 3): no rounding of the device raises a flag
                assert r["cfg"].max_value == r["setup"].max_value == 3.0
                assert 1e-6 < np.abs(rew).max() <= 0.3, (t, b, np.abs(rew).max())
                assert abs(np.linalg.norm(yn) / np.linalg.norm(r["y"][b]) - 1) < 0.02 * (t + 1)
                assert np.abs(s["pa"][b]).max() > 0 and np.abs(st).max() > 1e-4
        if c.tsteps > 1:                                  # the stack is full of distinct rows after tsteps steps
            st = r["steps"][-1]["state"][0]
            fresh = c.window ** 2
            assert all(np.abs(st[i * fresh:(i + 1) * fresh] - st[j * fresh:(j + 1) * fresh]).max() > 1e-7
                       for i in range(c.tsteps) for j in range(i))


@pytest.mark.parametrize("case", ["fused_unpadded_256", "fused_unpadded_384"])
def test_fused_inputs_tell_the_self_mirror_arm_apart(pkg, case):
    """on an un-padded grid the Nyquist line (row and column n / 2) is its own mirror: what a sub-step adds there, and what the
    advection term alone adds, is above 1e-3 of max |result| -- a thousand times the fp32 bound and 1e8 times the fp64 one --, and
    zeroing the line moves the result by far more than any tolerance"""
    c = fc.CASES[case]
    r = fc.reference(pkg, fluid, case)
    h, m = r["cfg"].dt / c.K, c.n // 2
    for b in range(c.B):
        ref, y0 = r["step"][b], r["y"][b]
        M = np.abs(ref).max()
        adv = fluid.advection(r["cfg"], y0.copy())
        for line in (np.s_[m, :], np.s_[:, m]):
            assert np.abs(y0[line]).max() >= 1e-2 * np.abs(y0).max()                      # populated
            assert np.abs((ref - y0)[line]).max() >= 1e-3 * M and h * np.abs(adv[line]).max() >= 1e-3 * M
            z = ref.copy()
            z[line] = 0
            assert np.abs(z - ref).max() >= 1e-3 * M >= 100 * fc.TOL["f32"]["step"] * M


@pytest.mark.parametrize("case", ["fused_unpadded_256", "fused_tiles_256"])
def test_fused_inputs_tell_the_third_substep_apart(pkg, case):
    """K = 3: the result differs from two sub-steps of the same size -- a chain that runs its mode-4 K31 once -- by more than 1e-3"""
    c = fc.CASES[case]
    r = fc.reference(pkg, fluid, case)
    assert c.K == 3
    cfg2 = fluid.FluidConfig(nx=c.n, ifpad=c.ifpad, dt=r["cfg"].dt * 2 / 3, oversampling=2)
    for b in range(2):
        two = fluid.do_step(cfg2, r["y"][b], r["p"][b], 2)
        assert np.abs(two - r["step"][b]).max() >= 1e-3 * np.abs(r["step"][b]).max()
