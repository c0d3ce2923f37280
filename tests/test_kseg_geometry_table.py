"""The case table of test_gpu_kseg_geometry.py (kseg_geometry_cases.py) held against the oracle and the setup's host tables.  Runs
without a GPU: it proves that every row reaches what it is there for (work-group size, band widths, window wrap, sense_dots'
grouping, which rollout instantiation), that the inputs stay finite and inside the blow-up bound in the oracle itself -- so the
GPU test cannot pass on NaNs -- and it fails by name when a purpose of the table loses its row."""
import numpy as np
import pytest

import kseg_geometry_cases as kc
from oracle import keller_segel as kg


@pytest.fixture(scope="module")
def geo(pkg):
    out = {}
    for name in kc.CASES:
        setup, cfg = kc.build(pkg, kg, name)
        G, Ga, a2s = setup.tables()
        out[name] = kc.geometry(G, Ga, a2s, name)
    return out


@pytest.mark.parametrize("case", list(kc.CASES))
def test_setup_tables_are_the_oracles(pkg, case):
    setup, cfg = kc.build(pkg, kg, case)
    G, Ga, a2s = setup.tables()
    c = kc.CASES[case]
    assert G.shape == (len(c.sensor_positions), c.nx) and Ga.shape == (len(c.actuators_to_sensors), c.nx)
    assert np.array_equal(G, cfg.gaussians) and np.array_equal(Ga, cfg.gaussians_actuators)
    assert np.array_equal(a2s, cfg.actuators_to_sensors - 1) and a2s.dtype == np.int32
    assert (G.sum(axis=1) == 5).all() and set(np.unique(G)) == {0.0, 1.0}          # every box whole: none leaves the grid
    assert abs(setup.dx - 0.1) < 1e-12 and abs(cfg.dx - setup.dx) == 0              # the stable cell size (module docstring)
    e = setup.env_cfg(3, 0)
    assert (e.N, e.S, e.A, e.window, e.temporal_steps, e.K) == (c.nx, G.shape[0], Ga.shape[0], c.window_size, c.temporal_steps, c.substeps)
    assert e.integrator == (1 if c.integrator == "midpoint" else 0)
    assert e.check_max_value == {"y": 1, "reward": 2, "off": 0}[c.check_max_value]
    assert (e.action_punish, e.delta_action_punish, e.max_value) == (c.action_punish, c.delta_action_punish, c.max_value)
    assert setup.state_shape == (c.window_size * 2 * c.temporal_steps, len(c.actuators_to_sensors))
    assert c.window_size <= G.shape[0] and 4 <= c.nx <= 1024                        # what pdec_env_create accepts


def _closed_trajectory(case, cfg, y0, act, prev):
    """three control steps of one trajectory in the oracle; returns max |y|, max |reward| and the states' finiteness"""
    y, state, a_prev = y0, kg.featurize(cfg, y0, None), prev[None]
    ymax = rmax = 0.0
    for t in range(act.shape[0]):
        a = act[t][None]
        y = kc.oracle_step(kg, cfg, case, y, kg.prepare_action(cfg, a))
        r = kg.reward_function(cfg, y, a, a - a_prev)
        state, a_prev = kg.featurize(cfg, y, state), a
        assert np.isfinite(y).all() and np.isfinite(r).all() and np.isfinite(state).all()
        ymax, rmax = max(ymax, float(np.abs(y).max())), max(rmax, float(np.abs(r).max()))
    return ymax, rmax


@pytest.mark.parametrize("case", list(kc.CASES))
def test_inputs_stay_finite_and_tame_in_the_oracle(pkg, case):
    setup, cfg = kc.build(pkg, kg, case)
    c = kc.CASES[case]
    y0, act, prev = kc.inputs(case, 5)
    assert np.abs(act).max() <= 1 and np.abs(prev).max() <= 1 and np.abs(y0 - 1).max() < 0.3
    for b in range(5):
        ymax, rmax = _closed_trajectory(case, cfg, y0[b], act[:, b], prev[b])
        # tame: no blow-up flag on any row, with a margin no rounding of the device crosses
        assert ymax < 2.0, (b, ymax)
        if c.check_max_value == "reward":
            assert rmax < 0.5 * c.max_value, (b, rmax)
        else:
            assert ymax < 0.5 * c.max_value


# ---- every purpose of the table, by name: (what it is there for, predicate over a row's geometry and case)
PURPOSES = {
    "one wave, no dead lane": lambda g, c: g["nthreads"] == 64 and g["dead_lanes"] == 0,
    "63 dead lanes, the last cell alone in wave 1 and actuated": lambda g, c: g["nthreads"] == 128 and g["dead_lanes"] == 63 and g["last_cell_alone"] and g["last_cell_actuated"],
    "shipped grid, window wraps at both ends": lambda g, c: c.nx == 100 and g["S"] == 20 and g["Wd"] == 5 and g["Cnt"] == 1 and g["wraps_low"] and g["wraps_high"],
    "Cnt >= 2 with Wd unchanged": lambda g, c: g["Cnt"] == 2 and g["Wd"] == 5,
    "actuator band of a cell wraps from actuator A-1 to 0": lambda g, c: g["band_wraps"] and g["Cnt"] == 2 and g["A"] == g["S"],
    "non-monotone a2s": lambda g, c: not g["monotone"] and g["A"] < g["S"],
    "fmap, two species, window 3": lambda g, c: g["fmap"] and c.window_size == 3 and g["wraps_low"] and g["wraps_high"],
    "fmap, two species, window 5": lambda g, c: g["fmap"] and c.window_size == 5 and g["wraps_low"] and g["wraps_high"],
    "general featurize path, deep stack, window 1": lambda g, c: c.temporal_steps == 3 and c.window_size == 1,
    "general featurize path, deep stack, window 5 wrapping": lambda g, c: c.temporal_steps == 3 and c.window_size == 5 and g["wraps_low"] and g["wraps_high"],
    "ng == 1 in sense_dots": lambda g, c: g["ng"] == 1 and 2 * g["S"] > g["nthreads"],
    "a sense_dots chunk of several rows that overshoots Wd": lambda g, c: g["chunk"] >= 2 and g["chunk_overshoots"],
    "five band rows per cell in actuate_cell": lambda g, c: g["Cnt"] == 5 and g["cover"] == 5,
    "nthreads 320, last cell alone in its wave": lambda g, c: g["nthreads"] == 320 and g["last_cell_alone"],
    "nthreads 1024 with dead lanes": lambda g, c: g["nthreads"] == 1024 and g["dead_lanes"] > 0,
    "nthreads 1024, 16 full waves": lambda g, c: g["nthreads"] == 1024 and g["dead_lanes"] == 0 and g["waves"] == 16,
    "smallest grid, some cell under all 4 actuators": lambda g, c: c.nx == 8 and g["cover"] == 4 and g["A"] == 4,
    "punishments on, shipped a2s subset": lambda g, c: c.action_punish == 0.3 and c.delta_action_punish == 0.7 and c.actuators_to_sensors == tuple(range(3, 19)),
    "punishments on, permuted a2s": lambda g, c: c.action_punish == 0.3 and c.delta_action_punish == 0.7 and not g["monotone"],
    "midpoint integrator at a non-default size": lambda g, c: c.integrator == "midpoint" and c.substeps == 8 and c.nx == 65,
    "check_max_value reward": lambda g, c: c.check_max_value == "reward",
    "check_max_value off": lambda g, c: c.check_max_value == "off",
    "first and last cell both actuated": lambda g, c: g["first_cell_actuated"] and g["last_cell_actuated"],
}


@pytest.mark.parametrize("purpose", list(PURPOSES))
def test_every_purpose_has_its_row(geo, purpose):
    hit = [n for n in kc.CASES if PURPOSES[purpose](geo[n], kc.CASES[n])]
    assert hit, f"no row of kseg_geometry_cases.CASES is there for: {purpose}"


def test_rows_say_what_their_names_say(pkg, geo):
    want = {"wave1_nx64": dict(nthreads=64, dead_lanes=0, Cnt=2), "dead63_nx65": dict(nthreads=128, dead_lanes=63, Cnt=1, ng=8),
            "nx257": dict(nthreads=320, S=52, ng=6), "nx1000": dict(nthreads=1024, dead_lanes=24, S=200, A=100, ng=5),
            "nx1024": dict(nthreads=1024, dead_lanes=0, S=205, A=100, ng=4, chunk=2), "smallest_nx8": dict(nthreads=64, cover=4, Wd=5),
            "overlap_nx100": dict(Cnt=2, Wd=5, S=32, ng=4, chunk=2, band_wraps=False),
            "rotated_nx100": dict(Cnt=2, Wd=5, S=32, A=32, band_wraps=True), "ng1_nx64": dict(ng=1, S=60, Cnt=5, chunk=5),
            "roll_nx320": dict(nthreads=320, A=8, S=16), "wrap_nx100": dict(nthreads=128, A=11, Cnt=1, ng=6, chunk=1)}
    for name, w in want.items():
        got = {k: geo[name][k] for k in w}
        assert got == w, (name, got)
    # the shipped point, for the record: what every other 1-D Keller-Segel test runs at
    G, Ga, a2s = pkg.KellerSegelSetup().tables()
    ship = kc.geometry(G, Ga, a2s, kc.Case(100, 10.0, (), (), 3, 2, 32, "rk4", 0.0, 0.0, "y", 20.0))
    assert (ship["nthreads"], ship["dead_lanes"], ship["Cnt"], ship["Wd"], ship["ng"], ship["chunk"]) == (128, 28, 1, 5, 6, 1)
    assert not ship["wraps_low"] and not ship["wraps_high"] and ship["monotone"] and not ship["band_wraps"]
    # no row of the table reaches sense_dots' 8-row unrolled body: a setup's boxes are 5 cells wide whatever the geometry ...
    assert {g["Wd"] for g in geo.values()} == {5} and {g["unrolled_rows"] for g in geo.values()} == {0}
    # ... so one geometry with 21-cell boxes is built beside the table (kc.build_wide): one group, two unrolled passes, a tail of 5
    setup, cfg = kc.build_wide(pkg, kg)
    G, Ga, a2s = setup.tables()
    assert np.array_equal(G, cfg.gaussians) and np.array_equal(Ga, cfg.gaussians_actuators) and (G.sum(axis=1) == 21).all()
    wide = kc.geometry(G, Ga, a2s, kc.WIDE)
    assert (wide["Wd"], wide["S"], wide["ng"], wide["chunk"], wide["unrolled_rows"], wide["Cnt"]) == (21, 80, 1, 21, 16, 3)
    y0, act, prev = kc.inputs(kc.WIDE, 3)
    for b in range(3):
        ymax, rmax = _closed_trajectory(kc.WIDE, cfg, y0[b], act[:, b], prev[b])
        assert ymax < 2.0


def test_rollout_rows_reach_both_member_instantiations_and_the_refusal(geo):
    """kseg_rollout_lds restated: which (row, dtype) the persistent launch serves, and with which work-group size"""
    served = {(n, ts): kc.rollout_served(geo[n], ts, kc.CASES[n].check_max_value) for n in kc.ROLLOUT for ts in (8, 4)}
    small = [n for n in kc.ROLLOUT if geo[n]["nthreads"] <= 256 and served[n, 8] and served[n, 4]]
    big = [n for n in kc.ROLLOUT if geo[n]["nthreads"] > 256 and served[n, 8] and served[n, 4]]
    assert small and big, served                      # kseg_rollout_kernel<T, true, 256> and <T, true, 1024>, both dtypes
    assert any(geo[n]["fmap"] for n in small) and any(not geo[n]["fmap"] for n in small)
    assert served["roll_nx320", 8] and kc.rollout_lds(geo["roll_nx320"], 8) < 32 * 1024
    # 1024 cells with 100 actuators: 125 KiB in fp64 (the step loop serves it), 62.7 KiB in fp32 (one launch of 1024 threads)
    assert not served["nx1024", 8] and served["nx1024", 4]
    assert kc.rollout_lds(geo["nx1024"], 8) == 128384 and kc.rollout_lds(geo["nx1024"], 4) == 64200
    for n in kc.ROLLOUT:
        assert kc.CASES[n].check_max_value == "y" and kc.CASES[n].action_punish == 0


@pytest.mark.parametrize("case", kc.BLOWUP)
@pytest.mark.parametrize("check", ["y", "reward", "off"])
def test_blowup_inputs_split_the_batch_in_the_oracle(pkg, case, check):
    """test 3c's inputs in the oracle: trajectory 1 (patched) and 3 (one NaN cell) are past the bound, 0 / 2 / 4 far inside it,
    for the field test (max_value 20) and for the reward test (max_value 0.5) alike"""
    mv = kc.BLOWUP_REWARD_MAX if check == "reward" else 20.0
    setup, cfg = kc.build(pkg, kg, case, check_max_value=check, max_value=mv)
    y0, bad, act, prev = kc.blowup_inputs(case)
    G, Ga, a2s = setup.tables()
    assert (Ga[:, -3:] != 0).any(axis=0).all()          # the patch lies under an actuator's box
    for b in range(5):
        with np.errstate(all="ignore"):
            y = kc.oracle_step(kg, cfg, case, bad[b], kg.prepare_action(cfg, act[b][None]))
            r = kg.reward_function(cfg, y, act[b][None], act[b][None] - prev[b][None])
        x = r if check == "reward" else y
        if b in (1, 3):
            assert kc.blown(x, mv)
            if b == 1:
                assert np.isfinite(y).all() and np.abs(x).max() > 1.2 * mv      # finite, and past the bound by a margin
            else:
                assert np.isnan(x).any()
        else:
            assert np.abs(x).max() < 0.5 * mv, (b, np.abs(x).max())
