"""The case table of test_gpu_kseg2d_geometry.py (kseg2d_geometry_cases.py) held against the oracle and the setup's host tables.
Runs without a GPU: it proves that every row reaches what it is there for (tiles per trajectory, the tile order, the parts of a
split batch, clipped boxes, the second passes of the box-sum loops), that the inputs stay finite and inside the blow-up bound in
the oracle itself -- so the GPU test cannot pass on NaNs -- that the blow-up inputs lie on both sides of the bound, and it fails by
name when a purpose of the table loses its row."""
import numpy as np
import pytest

import kseg2d_geometry_cases as kc
from oracle import keller_segel2d as k2

CASES = list(kc.CASES)


@pytest.fixture(scope="module")
def geo():
    return {name: kc.geometry(name) for name in kc.CASES}


@pytest.mark.parametrize("case", CASES)
def test_setup_tables_are_the_oracles(pkg, case):
    c = kc.CASES[case]
    setup, cfg = kc.build(pkg, k2, case)
    g = kc.geometry(case)
    sx, sy, a2s = setup.tables()
    assert sx.dtype == sy.dtype == a2s.dtype == np.int32
    assert np.array_equal(sx, cfg.sensor_x - 1) and np.array_equal(sy, cfg.sensor_y - 1) and np.array_equal(a2s, cfg.a2s)
    assert list(a2s) == g["a2s"] and len(set(g["a2s"])) == g["A"] == kc.n_actuators(case) == cfg.A == setup.n_actuators
    assert (cfg.Sx, cfg.Sy, cfg.S, cfg.hw) == (g["Sx"], g["Sy"], g["S"], kc.HW) and setup.half_window == kc.HW
    # the constraints on every row (module docstring of the table)
    assert c.nx % 4 == 0 and c.nx >= 4 and c.ny >= 1 and c.substeps >= 3 and c.window_size % 2 == 1
    assert abs(setup.dx - 0.1) < 1e-12 and cfg.dx == setup.dx and 8 * (cfg.dt / c.substeps) / cfg.dx ** 2 < 2.78
    assert all(1 <= p <= c.nx for p in c.sensor_x) and all(1 <= p <= c.ny for p in c.sensor_y)
    e = setup.env_cfg(c.B, 0)
    assert (e.N, e.Ny, e.S, e.A, e.window, e.temporal_steps, e.K, e.B) == \
        (c.nx, c.ny, g["S"], g["A"], c.window_size, c.temporal_steps, c.substeps, c.B)
    assert e.check_max_value == {"y": 1, "reward": 2, "off": 0}[c.check_max_value]
    assert (e.action_punish, e.delta_action_punish, e.max_value) == (c.action_punish, c.delta_action_punish, c.max_value)
    assert (e.reward_in_scale, e.reward_offset, e.sensor_scale) == (1.0 / 5, -1.0, 0.25 / 5)
    assert setup.state_shape == (g["ns"], g["A"]) and g["ns"] == 2 * c.window_size ** 2 * c.temporal_steps
    # cell_act and acnt of pdec_kseg2d_env_create, restated from KSeg2DConfig.box: no two actuator boxes share a cell
    cell_act = np.full((c.ny, c.nx), -1)
    for a, s in enumerate(cfg.a2s):
        box = cfg.box(s)
        assert (cell_act[box] == -1).all(), f"actuator boxes {cell_act[box].max()} and {a} overlap"
        cell_act[box] = a
        assert cell_act[box].size == g["acnt"][a]
    assert [int((cell_act == a).sum()) for a in range(g["A"])] == g["acnt"]
    assert [np.zeros((c.ny, c.nx))[cfg.box(s)].size for s in range(cfg.S)] == g["scnt"]
    # prepare_action is the gather through cell_act
    act = np.arange(1.0, g["A"] + 1)[None]
    assert np.array_equal(k2.prepare_action(cfg, act), np.where(cell_act >= 0, 10.0 * act[0][np.maximum(cell_act, 0)], 0.0))


def test_default_actuators_are_the_border_rule(pkg):
    """actuators_to_sensors= / a2s= default to the border rule, and a wrong list is refused by name"""
    a, b = pkg.KellerSegel2DSetup(nx=64, ny=20), pkg.KellerSegel2DSetup(nx=64, ny=20, actuators_to_sensors=None)
    assert np.array_equal(a.actuators_to_sensors, b.actuators_to_sensors)
    Sx, Sy = a.Sx, a.Sy
    want = [iy * Sx + ix + 1 for iy in range(1, Sy - 1) for ix in range(2, Sx - 2)]          # border_y = min(2, (4 - 1) // 2) = 1
    assert list(a.actuators_to_sensors) == want
    cfg = k2.KSeg2DConfig(nx=64, ny=20, Lx=6.4, sensor_x=a.sensor_x, sensor_y=a.sensor_y)
    assert list(cfg.a2s + 1) == want
    assert list(k2.KSeg2DConfig(nx=64, ny=20, Lx=6.4, sensor_x=a.sensor_x, sensor_y=a.sensor_y, a2s=[5, 2]).a2s) == [4, 1]
    assert list(pkg.KellerSegel2DSetup(nx=64, ny=20, actuators_to_sensors=[5, 2]).tables()[2]) == [4, 1]
    for bad in ([0, 3], [Sx * Sy + 1], []):
        with pytest.raises(pkg.PdecError, match="KellerSegel2DSetup: actuators_to_sensors"):
            pkg.KellerSegel2DSetup(nx=64, ny=20, actuators_to_sensors=bad)


def test_rows_say_what_their_names_say(geo):
    T, F = True, False
    want = {
        "smallest_4x1": dict(tiles={4: (1, 1), 8: (1, 1)}, Sx=1, Sy=1, A=1, acnt=[4], clipped=T, window_revisits=T),
        "onetile_64x64": dict(tiles={4: (1, 1), 8: (1, 2)}, A=81, actuator_clipped=F, last_strip_only=F),
        "ragged_68x65": dict(tiles={4: (2, 2), 8: (2, 3)}, last_strip_only=T, last_row_only={4: T, 8: T}, remapped={4: F, 8: F}),
        "remap_192x64": dict(tiles={4: (3, 1), 8: (3, 2)}, grid={4: 24, 8: 48}, remapped={4: T, 8: T}, tiles_divide_8={4: F, 8: F}),
        "noremap_192x64": dict(tiles={4: (3, 1), 8: (3, 2)}, grid={4: 9, 8: 18}, remapped={4: F, 8: F}),
        "wide_260x12": dict(column_pass2=T, Sx=52, Sy=2, A=104, last_cell_actuated=F, sensor_pass2=F),
        "dense_200x8": dict(sensor_pass2=T, Sx=66, sensor_overlap=T, column_pass2=F, A=66),
        "clipped_64x20": dict(clipped=T, actuator_clipped=T, Sx=14, Sy=5, A=52),
        "permuted_100x20": dict(monotone=F, A=16, Sx=20, Sy=4, clipped=F),
        "w1_t3_64x32": dict(ns=6), "w5_t1_100x40": dict(ns=50, Sy=8), "w3_sy2_64x10": dict(Sy=2, window_revisits=T, ns=36),
        "rewardcheck_68x65": dict(last_cell_actuated=T, actuator_clipped=T), "nocheck_68x65": dict(A=90),
        "split3_68x65": dict(grid={4: 1540, 8: 2310}, parts=[128, 128, 129]),
        "split2_68x65": dict(grid={4: 1024, 8: 1536}, parts=[128, 128]),
    }
    assert set(want) == set(kc.CASES)
    for name, w in want.items():
        got = {k: geo[name][k] for k in w}
        assert got == w, (name, got)
    assert [geo[n]["parts"] for n in kc.CASES if not n.startswith("split")] == [[]] * 14
    # the box that ends on cell 260 of wide_260x12 is an actuator's (its row is not the grid's last: 12 rows, boxes 1..5 | 6..10)
    c = kc.CASES["wide_260x12"]
    assert c.sensor_x[-1] == 258 and kc.box_range(258, 260) == (255, 259) and 52 - 1 in [s % 52 for s in geo["wide_260x12"]["a2s"]]
    # dense_200x8: actuators on every other sensor of a row, sensor 66 among them, six cells apart
    d = geo["dense_200x8"]
    assert sorted({s % 66 for s in d["a2s"]}) == list(range(1, 66, 2)) and kc.CASES["dense_200x8"].sensor_x[65] == 198
    assert sorted(set(d["acnt"])) == [15, 25]
    assert sorted(set(geo["clipped_64x20"]["acnt"])) == [9, 15, 25]
    # clipped at all four edges and corners
    cl = kc.CASES["clipped_64x20"]
    assert (cl.sensor_x[0], cl.sensor_x[-1], cl.sensor_y[0], cl.sensor_y[-1]) == (1, 64, 1, 20)
    corners = {(s // 14, s % 14) for s in geo["clipped_64x20"]["a2s"]}
    assert {(0, 0), (0, 13), (4, 0), (4, 13)} <= corners
    # the shipped point, for the record: what every other full-size test runs at
    assert kc.tiles(256, 256, 4) == (4, 4) and kc.remapped(256, 256, 128, 4) and kc.parts(256, 256, 128) == [42, 43, 43]
    assert kc.parts(256, 256, 96) == [32, 32, 32] and kc.parts(256, 256, 4) == []
    # the tile order is a permutation either way; consecutive workgroups of a remapped grid belong to different trajectories
    for n, per in ((24, 3), (48, 6), (9, 3), (18, 6)):
        lid = kc.remap(n)
        assert sorted(lid) == list(range(n))
        if n % 8 == 0:
            assert len({lid[w] // per for w in range(8)}) == 8 and lid != list(range(n))
        else:
            assert lid == list(range(n))
    assert [kc.nsub2_launches(K) for K in (1, 2, 3, 4, 5)] == [[1], [2], [2, 1], [2, 2], [2, 2, 1]]
    assert kc.picks("split3_68x65") == [0, 64, 127, 128, 192, 255, 256, 320, 384] and kc.picks("remap_192x64") == list(range(8))
    assert kc.split_patched("split3_68x65") == [127, 128, 384] and kc.split_patched("split2_68x65") == [127, 128, 255]
    assert set(kc.SPLIT) == {n for n in kc.CASES if geo[n]["parts"]} and all(kc.SPLIT[n] == len(geo[n]["parts"]) - 1 for n in kc.SPLIT)
    assert all(kc.CASES[n].precs == ("f32",) for n in kc.SPLIT)
    assert all(kc.CASES[n].B == 3 for n in kc.CASES if n not in kc.SPLIT and n != "remap_192x64")


# ---- every purpose of the table, by name: (what it is there for, predicate over a row's geometry and case)
PURPOSES = {
    "the smallest grid, one box clipped on all four sides to the whole domain": lambda g, c: (c.nx, c.ny) == (4, 1) and g["acnt"] == [4] and g["S"] == 1,
    "fp32 exactly one tile, fp64 two tiles": lambda g, c: (c.nx, c.ny) == (64, 64) and g["tiles"] == {4: (1, 1), 8: (1, 2)},
    "last tile column one strip wide": lambda g, c: g["last_strip_only"] and g["tiles"][4][0] >= 2,
    "last tile row one row high, fp32": lambda g, c: g["last_row_only"][4] and g["tiles"][4][1] >= 2,
    "last tile row one row high, fp64": lambda g, c: g["last_row_only"][8] and g["tiles"][8][1] >= 2,
    "remapped grid whose tile count does not divide 8, fp32": lambda g, c: g["remapped"][4] and not g["tiles_divide_8"][4] and c.B == 8,
    "remapped grid whose tile count does not divide 8, fp64": lambda g, c: g["remapped"][8] and not g["tiles_divide_8"][8] and c.B == 8,
    "the same grid not remapped": lambda g, c: (c.nx, c.ny) == (192, 64) and not g["remapped"][4] and not g["remapped"][8],
    "second pass of the box-sum column loop, last box an actuator": lambda g, c: g["column_pass2"] and c.sensor_x[-1] + kc.HW == c.nx and c.border == 0,
    "second pass of the box-sum sensor loop, overlapping sensor boxes": lambda g, c: g["sensor_pass2"] and g["sensor_overlap"] and 65 in {s % g["Sx"] for s in g["a2s"]},
    "actuator boxes clipped at edges and corners": lambda g, c: {9, 15, 25} <= set(g["acnt"]),
    "non-monotone actuator list with punishments": lambda g, c: not g["monotone"] and c.action_punish == 0.3 and c.delta_action_punish == 0.7,
    "window 1, temporal_steps 3": lambda g, c: (c.window_size, c.temporal_steps) == (1, 3),
    "window 5, temporal_steps 1, Sy 8": lambda g, c: (c.window_size, c.temporal_steps, g["Sy"]) == (5, 1, 8),
    "Sy 2 under window 3": lambda g, c: g["Sy"] == 2 and c.window_size == 3 and g["Sx"] > 3,
    "window wraps along x and y": lambda g, c: g["window_wraps_x"] and g["window_wraps_y"],
    "check_max_value reward, the corner box an actuator's": lambda g, c: c.check_max_value == "reward" and g["last_cell_actuated"],
    "check_max_value off": lambda g, c: c.check_max_value == "off",
    "three parts with a ragged tile": lambda g, c: g["parts"] == [128, 128, 129] and g["last_strip_only"],
    "two parts with a ragged tile": lambda g, c: g["parts"] == [128, 128] and g["last_strip_only"],
}


@pytest.mark.parametrize("purpose", list(PURPOSES))
def test_every_purpose_has_its_row(geo, purpose):
    hit = [n for n in kc.CASES if PURPOSES[purpose](geo[n], kc.CASES[n])]
    assert hit, f"no row of kseg2d_geometry_cases.CASES is there for: {purpose}"


def _closed_trajectory(cfg, y0, act, prev):
    """three control steps of one trajectory in the oracle; returns max |y| and max |reward|"""
    y, state, a_prev = y0, k2.featurize(cfg, y0, None), prev
    ymax = rmax = 0.0
    for t in range(act.shape[0]):
        a = act[t]
        y = k2.do_step(cfg, y, k2.prepare_action(cfg, a))
        r = k2.reward_function(cfg, y, a, a - a_prev)
        state, a_prev = k2.featurize(cfg, y, state), a
        assert np.isfinite(y).all() and np.isfinite(r).all() and np.isfinite(state).all()
        ymax, rmax = max(ymax, float(np.abs(y).max())), max(rmax, float(np.abs(r).max()))
    return ymax, rmax


@pytest.mark.parametrize("case", CASES)
def test_inputs_stay_finite_and_tame_in_the_oracle(pkg, case):
    c = kc.CASES[case]
    setup, cfg = kc.build(pkg, k2, case)
    y0, act, prev = kc.inputs(case)
    assert y0.shape == (c.B, 2, c.ny, c.nx) and act.shape == (3, c.B, 1, cfg.A) and prev.shape == (c.B, 1, cfg.A)
    assert np.abs(act).max() <= 1 and np.abs(prev).max() <= 1 and np.abs(y0 - 1).max() < 0.3
    assert len({y0[b].tobytes() for b in range(c.B)}) == c.B                        # every trajectory has a field of its own
    reward_bound = kc.BLOWUP_REWARD_MAX if c.action_punish == 0 else None
    for b in kc.picks(case):
        ymax, rmax = _closed_trajectory(cfg, y0[b], act[:, b], prev[b])
        # tame: no blow-up flag on any row, with a margin no rounding of the device crosses
        assert ymax < 2.0, (b, ymax)
        if c.check_max_value == "reward":
            assert c.max_value == kc.BLOWUP_REWARD_MAX
        if reward_bound is not None:          # far from the reward bound of rewardcheck (rows without punishments): under a tenth
            assert rmax < 0.1 * reward_bound, (b, rmax)
        else:
            assert rmax < 0.3 + 0.7 * 4 + 0.01


@pytest.mark.parametrize("K", [3, 5])
@pytest.mark.parametrize("case", kc.BLOWUP)
def test_blowup_inputs_split_the_batch_in_the_oracle(pkg, case, K):
    """test d's inputs in the oracle: trajectory 1 (patched) is finite and past the bound after the step, 3 (one NaN cell) is NaN,
    0 / 2 / 4 are far inside the bound -- for the field test (max_value 20) and the reward test (BLOWUP_REWARD_MAX) alike"""
    c = kc.CASES[case]
    setup, cfg = kc.build(pkg, k2, case, substeps=K)
    y0, bad, act, prev = kc.blowup_inputs(case)
    assert bad.shape == (kc.BLOWUP_B, 2, c.ny, c.nx) and np.isnan(bad).sum() == 1
    assert (bad[1, 0, -1, -2:] == kc.PATCH).all() and (bad[1] == kc.PATCH).sum() == (4 if c.ny > 1 else c.nx)
    for b in range(kc.BLOWUP_B):
        with np.errstate(all="ignore"):
            y = k2.do_step(cfg, bad[b], k2.prepare_action(cfg, act[b]))
            r = k2.reward_function(cfg, y, act[b], act[b] - prev[b])
        x = r if c.check_max_value == "reward" else y
        if b == 1:
            assert np.isfinite(y).all() and 1.2 * 20.0 < np.abs(y).max() < kc.PATCH, np.abs(y).max()
            assert kc.blown(x, c.max_value) and np.abs(x).max() > 1.2 * c.max_value          # past the bound by a margin
        elif b == 3:
            assert np.isnan(x).any() and kc.blown(x, c.max_value)
        else:
            assert not kc.blown(x, c.max_value) and np.abs(x).max() < 0.5 * c.max_value, (b, np.abs(x).max())
