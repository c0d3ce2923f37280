"""The case table of test_gpu_ks_geometry.py (ks_geometry_cases.py) held against oracle/ks.py and the setup's host tables.  Runs
without a GPU: it proves that every row reaches what it is there for (FFT engine and actuation branch, band widths in each dtype,
sense_dots' grouping, A != S, the rollout's LDS bill), that the inputs stay finite and far inside the blow-up bound in the oracle
itself -- so the GPU test cannot pass on NaNs or sit on a flag's edge --, that plausible mistakes move the oracle's output by at
least 100 x the GPU test's bound (the evidence that the rows discriminate), and it fails by name when a purpose loses its row."""
import copy

import numpy as np
import pytest

import ks_geometry_cases as kc
from oracle import ks

PRECS = ("f64", "f32")


@pytest.fixture(scope="module")
def built(pkg):
    return {name: kc.build(pkg, ks, name) for name in kc.CASES}


@pytest.fixture(scope="module")
def geo(built):
    out = {}
    for name, (setup, cfg) in built.items():
        G, Ga, a2s = setup.tables()
        out[name] = {prec: kc.geometry(G, Ga, a2s, name, prec) for prec in PRECS}
    return out


@pytest.mark.parametrize("case", list(kc.CASES))
def test_setup_tables_are_the_oracles(pkg, built, case):
    setup, cfg = built[case]
    G, Ga, a2s = setup.tables()
    c = kc.CASES[case]
    S, A = len(c.sensor_positions), kc.n_actuators(case)
    assert G.shape == (S, c.nx) and Ga.shape == (A, c.nx) and setup.n_actuators == A == len(cfg.actuator_positions)
    assert np.array_equal(G, cfg.gaussians) and np.array_equal(Ga, cfg.gaussians_actuators)
    assert np.array_equal(a2s, cfg.actuators_to_sensors - 1) and a2s.dtype == np.int32 and a2s.min() >= 0 and a2s.max() < S
    assert np.abs(G.sum(axis=1) - 1).max() < 1e-12 and G.min() >= 0 and np.abs(Ga.max(axis=1) - 1).max() < 1e-12
    assert abs(setup.dx - (22 / 192 if c.nx == 192 else 200 / 240)) < 1e-12 and cfg.dx == setup.dx     # the tame cell sizes
    e = setup.env_cfg(5, 0)
    assert (e.N, e.S, e.A, e.window, e.temporal_steps, e.K, e.mono) == (c.nx, S, A, c.window_size, c.temporal_steps, 30, int(c.mono))
    assert e.pde_kind == (pkg._lib.PDE_KS_CNAB2 if c.integrator == "cnab2" else pkg._lib.PDE_KS_RK4_FD)
    assert e.integrator == (1 if c.integrator == "midpoint_fd" else 0)
    assert e.check_max_value == {"y": 1, "reward": 2, "off": 0}[c.check_max_value]
    assert (e.action_punish, e.delta_action_punish, e.max_value, e.mu) == \
        (c.action_punish, c.delta_action_punish, c.max_value, 0.0 if c.mono else c.mu)
    assert (e.sensor_scale, e.reward_denom) == (1 / c.max_value, 3 * c.max_value)
    assert setup.state_shape == ((S, 1) if c.mono else (c.window_size * c.temporal_steps, A))
    assert c.window_size <= S or c.mono                                            # what pdec_env_create accepts
    if not c.mono and c.actuators_to_sensors is not None:      # the actuators sit on their sensors (KSSetup.jl:113)
        assert np.array_equal(setup.actuator_positions, setup.sensor_positions[a2s])
        alone = pkg.KSSetup(c.nx, c.Lx, np.array(c.sensor_positions), actuators_to_sensors=np.array(c.actuators_to_sensors),
                            sigma_sensors=c.sigma_sensors, sigma_actuators=c.sigma_actuators)
        assert alone.n_actuators == A and np.array_equal(alone.gaussians_actuators, Ga)


def _closed_trajectory(case, cfg, y0, act, prev):
    """three control steps of one trajectory in the oracle; returns max |y| and max |reward|"""
    y, state, a_prev = y0, ks.featurize(cfg, y0, None), prev
    ymax = rmax = 0.0
    for t in range(act.shape[0]):
        a = act[t]
        y = kc.oracle_step(ks, cfg, case, y, ks.prepare_action(cfg, a[None]))
        r = ks.reward_function(cfg, y, a[None], (a - a_prev)[None])
        state, a_prev = ks.featurize(cfg, y, state), a
        assert np.isfinite(y).all() and np.isfinite(r).all() and np.isfinite(state).all()
        ymax, rmax = max(ymax, float(np.abs(y).max())), max(rmax, float(np.abs(r).max()))
    return ymax, rmax


@pytest.mark.parametrize("case", list(kc.CASES))
def test_inputs_stay_finite_and_tame_in_the_oracle(built, case):
    setup, cfg = built[case]
    c = kc.CASES[case]
    y0, act, prev = kc.inputs(case, 5)
    assert np.abs(act).max() <= 1 and np.abs(prev).max() <= 1 and abs(np.linalg.norm(y0[0]) - 4.5) < 1e-9
    for b in range(5):
        ymax, rmax = _closed_trajectory(case, cfg, y0[b], act[:, b], prev[b])
        # tame: no blow-up flag on any row, with a margin no rounding of the device crosses
        assert ymax < 6.0, (b, ymax)
        assert (rmax if c.check_max_value == "reward" else ymax) < 0.5 * c.max_value, (b, ymax, rmax)


# ---- every purpose of the table, by name.  "each": predicate(geometry, case, prec) must hold for some row in EACH dtype;
# "pair": predicate(fp64 geometry, fp32 geometry, case) for some row that runs in both
def _acts_apart(g, c):
    return not g["mono"] and not g["identity"]


PURPOSES = {
    # the actuation branch each engine does not meet at the shipped layouts
    "FftFixed192 with actuate_consecutive": ("each", lambda g, c, p: g["engine"] == "FftFixed192" and g["consecutive"] and not c.mono),
    "FftFixed240 with actuate_cells": ("each", lambda g, c, p: g["engine"] == "FftFixed240" and g["cells"]),
    "FftFixed600 with actuate_cells": ("each", lambda g, c, p: g["engine"] == "FftFixed600" and g["cells"]),
    "FftWave256 with actuate_cells": ("each", lambda g, c, p: g["engine"] == "FftWave256" and g["cells"]),
    "FftWave1024 with A << S": ("each", lambda g, c, p: g["engine"] == "FftWave1024" and 5 * g["A"] <= g["S"] and g["consecutive"]),
    "generic engine with actuate_consecutive": ("each", lambda g, c, p: g["engine"] == "FftGeneric" and g["consecutive"]),
    "generic engine with actuate_cells": ("each", lambda g, c, p: g["engine"] == "FftGeneric" and g["cells"]),
    # A != S, odd A, non-monotone a2s
    "odd A < S, non-monotone a2s, window wrapping at both ends": (
        "each", lambda g, c, p: g["A"] % 2 == 1 and g["A"] < g["S"] and not g["monotone"] and g["wraps_low"] and g["wraps_high"]
        and g["fmap"] and g["engine"] == "FftWave256"),
    "LDS carve-up with A != S in the form that has a SIMD-sharing twin": (
        "each", lambda g, c, p: g["engine"] == "FftWave256" and g["A"] != g["S"] and not c.mono and c.check_max_value == "y"),
    "sensors adjacent and on both sides of the seam": (
        "each", lambda g, c, p: {1, 2, c.nx - 1, c.nx} <= set(c.sensor_positions) and np.diff(c.sensor_positions).max() > 40),
    # narrow bands
    "Wd < 8: no pass of the unrolled body": ("each", lambda g, c, p: g["Wd"] < 8 and g["engine"] == "FftWave256"),
    "one unrolled pass and a tail": ("each", lambda g, c, p: g["unrolled_rows"] == 8 and g["tail_rows"] > 0),
    "one unrolled pass + tail in fp64, none in fp32": ("pair", lambda g, h, c: g["unrolled_rows"] == 8 and g["tail_rows"] and h["unrolled_rows"] == 0),
    "cells that no actuator reaches": ("each", lambda g, c, p: g["uncovered"] > 0 and g["engine"].startswith("Fft")),
    "cells with fewer band rows than Cnt (zero rows of GaC)": ("each", lambda g, c, p: g["zero_rows"] > 0 and g["min_cover"] > 0),
    "Cnt differs between the fp64 and the fp32 table": ("pair", lambda g, h, c: g["Cnt"] > h["Cnt"] >= 1),
    "Cnt = 1 in fp32 with cells the fp64 table covers left out": ("pair", lambda g, h, c: h["Cnt"] == 1 and h["uncovered"] > 0 and g["uncovered"] == 0),
    # sense_dots' grouping
    "1 < ng < 8 with a chunk that overshoots Wd": ("each", lambda g, c, p: 1 < g["ng"] < 8 and g["chunk_overshoots"] and g["chunk"] >= 2),
    "ng = 8 with a chunk that overshoots Wd": ("each", lambda g, c, p: g["ng"] == 8 and g["chunk_overshoots"]),
    "ng = 1 over the whole ring: Wd = N, Cnt = A, 24 unrolled passes": (
        "each", lambda g, c, p: g["ng"] == 1 and g["Wd"] == c.nx and g["Cnt"] == g["A"] and g["unrolled_rows"] == 192 and not c.mono),
    "largest grid of the dtype: ng = 4 overshooting, actuate_cells, >= 512 threads": (
        "each", lambda g, c, p: c.nx == (2048 if p == "f64" else 4096) and g["nthreads"] == c.nx // 4 and g["ng"] == 4
        and g["chunk_overshoots"] and g["cells"]),
    # the global agent
    "mono with A < S, ng = 2 overshooting": ("each", lambda g, c, p: c.mono and g["A"] < g["S"] and g["ng"] == 2 and g["chunk_overshoots"]),
    "mono with A > S and a repeated a2s": ("each", lambda g, c, p: c.mono and g["A"] > g["S"] and g["repeated"]),
    # featurize
    "general featurize path (temporal stack) with a non-identity a2s": (
        "each", lambda g, c, p: c.temporal_steps == 2 and not g["fmap"] and _acts_apart(g, c) and not g["monotone"] and c.window_size == 5),
    # flags and reward terms
    "check_max_value reward": ("each", lambda g, c, p: c.check_max_value == "reward" and _acts_apart(g, c)),
    "check_max_value off": ("each", lambda g, c, p: c.check_max_value == "off" and _acts_apart(g, c)),
    "visible punishments with a permuted a2s": (
        "each", lambda g, c, p: c.action_punish >= 0.3 and c.delta_action_punish >= 0.7 and not g["monotone"] and c.integrator == "cnab2"),
    "mu != 0 in the fused packed-pair step": ("each", lambda g, c, p: c.mu != 0 and c.integrator == "cnab2" and not c.mono),
    "mu != 0 and visible punishments in a served rollout with odd A (a column pair straddles the packed trajectories)": (
        "each", lambda g, c, p: c.mu != 0 and c.action_punish >= 0.3 and g["A"] % 2 == 1 and kc.rollout_served(g, c, p)),
    # the finite-difference twins
    "ksfd_wave_step_kernel with odd A < S, permuted": ("each", lambda g, c, p: g["engine"] == "ksfd_wave" and g["A"] % 2 and not g["monotone"]),
    "ksfd_wave_step_kernel with uncovered cells": ("each", lambda g, c, p: g["engine"] == "ksfd_wave" and g["uncovered"] > 0),
    "ksfd_env_step_kernel with A < S, uncovered cells, midpoint": (
        "each", lambda g, c, p: g["engine"] == "ksfd_lds" and g["A"] < g["S"] and g["uncovered"] > 0 and c.integrator == "midpoint_fd"),
}


@pytest.mark.parametrize("purpose", list(PURPOSES))
def test_every_purpose_has_its_row(geo, purpose):
    kind, pred = PURPOSES[purpose]
    if kind == "each":
        for prec in PRECS:
            hit = [n for n, c in kc.CASES.items() if prec in c.precs and pred(geo[n][prec], c, prec)]
            assert hit, f"no {prec} row of ks_geometry_cases.CASES is there for: {purpose}"
    else:
        hit = [n for n, c in kc.CASES.items() if set(c.precs) == set(PRECS) and pred(geo[n]["f64"], geo[n]["f32"], c)]
        assert hit, f"no row of ks_geometry_cases.CASES is there for: {purpose}"


def test_rows_say_what_their_names_say(pkg, geo):
    """(fp64, fp32) where the two tables differ"""
    want = {
        "perm_oddA_256": dict(engine="FftWave256", consecutive=True, S=64, A=23, Wd=(93, 35), Cnt=(20, 18), min_cover=(6, 1), ng=1),
        "narrow_256": dict(Wd=(15, 5), Cnt=(4, 2), unrolled_rows=(8, 0), tail_rows=(7, 5)),
        "narrower_256": dict(Wd=(7, 3), Cnt=(2, 1), uncovered=(0, 64)),
        "irregular_256": dict(engine="FftWave256", cells=True, S=12, A=5, ng=5, chunk=(7, 3), chunk_overshoots=True, uncovered=(132, 211)),
        "dense_192": dict(engine="FftFixed192", consecutive=True, Wd=192, Cnt=48, ng=1, unrolled_rows=192),
        "sparse_240": dict(engine="FftFixed240", cells=True, nthreads=128, ng=8, chunk=(12, 5), chunk_overshoots=True),
        "sparse_600": dict(engine="FftFixed600", cells=True, nthreads=320, ng=8, Cnt=(3, 1), uncovered=(0, 75)),
        "generic_60": dict(engine="FftGeneric", consecutive=True, ng=4, chunk=(8, 3), chunk_overshoots=True),
        "subset_1024": dict(engine="FftWave1024", nthreads=256, S=256, A=51, Wd=(23, 9), uncovered=(1, 565)),
        "mono_256": dict(S=32, A=13, ng=2, chunk=(47, 18), chunk_overshoots=True),
        "mono_192_wide": dict(S=4, A=16, repeated=True, ng=8),
        "fd_perm_256": dict(engine="ksfd_wave", nthreads=64, A=23, ng=1), "fd_irregular_256": dict(engine="ksfd_wave", ng=5, chunk=(7, 3)), "fd_midpoint_100": dict(engine="ksfd_lds", nthreads=128, A=7, S=25),
    }
    for name, w in want.items():
        for k, v in w.items():
            v = v if isinstance(v, tuple) else (v, v)
            assert (geo[name]["f64"][k], geo[name]["f32"][k]) == v, (name, k, geo[name]["f64"][k], geo[name]["f32"][k])
    g = geo["ng4_4096"]["f32"]
    assert (g["nthreads"], g["ng"], g["chunk"], g["Wd"], g["chunk_overshoots"], g["cells"]) == (1024, 4, 9, 35, True, True)
    g = geo["ng4_2048"]["f64"]       # the fp64 twin: 4096 complex fp64 points do not fit the LDS
    assert (g["nthreads"], g["ng"], g["chunk"], g["Wd"], g["chunk_overshoots"], g["cells"]) == (512, 4, 24, 93, True, True)
    assert kc.CASES["ng4_4096"].precs == ("f32",) and kc.CASES["ng4_2048"].precs == ("f64",)
    assert geo["ng4_4096"]["f64"]["lds_bytes"] > 160 * 1024 >= geo["ng4_4096"]["f32"]["lds_bytes"]
    assert all(geo[n][p]["lds_bytes"] <= 160 * 1024 for n, c in kc.CASES.items() for p in c.precs)
    # for the record: what the three shipped layouts reach -- every other KS test of the suite runs at one of them
    ship = {"KS22": pkg.KSSetup.KS22(), "KS200": pkg.KSSetup.KS200(), "bench_C2": pkg.KSSetup.bench_C2(256, window_size=3)}
    reached = {}
    for name, s in ship.items():
        case = kc._case(s.nx, s.sensor_positions, sigma=s.sigma_sensors, window_size=s.window_size, Lx=s.Lx)
        for prec in PRECS:
            g = kc.geometry(*s.tables(), case, prec)
            assert g["identity"] and g["A"] == g["S"] and g["A"] % 2 == 0 and g["uncovered"] == 0 and g["min_cover"] >= 1
            assert len(set(np.diff(s.sensor_positions))) == 1 and g["Cnt"] >= 2 and g["Wd"] >= 35
            reached[name, prec] = (g["engine"], "consecutive" if g["consecutive"] else "cells", g["ng"])
    assert reached == {("KS22", "f64"): ("FftFixed192", "cells", 8), ("KS22", "f32"): ("FftFixed192", "cells", 8),
                       ("KS200", "f64"): ("FftFixed240", "consecutive", 1), ("KS200", "f32"): ("FftFixed240", "consecutive", 1),
                       ("bench_C2", "f64"): ("FftWave256", "consecutive", 1), ("bench_C2", "f32"): ("FftWave256", "consecutive", 1)}


def test_rollout_rows_served_and_refused(geo):
    """ks_rollout_lds / ks_rollout_shape_ok restated: which (row, dtype) the persistent launch serves with its actor [ns, H, 1]"""
    served = {(n, p): kc.rollout_served(geo[n][p], n, p) for n, c in kc.CASES.items() for p in c.precs}
    for n in kc.ROLL_MUST_SERVE:
        assert served[n, "f64"] and served[n, "f32"], (n, served)
    g = geo["perm_oddA_256"]["f64"]
    assert kc.roll_h("perm_oddA_256") == 20 and kc.ks_rollout_lds(g, 8, [3, 20, 1]) == 63392 <= 64 * 1024     # 63.4 KB of 64 KiB
    assert kc.ks_rollout_lds(geo["narrow_256"]["f64"], 8, [5, 20, 1]) > 64 * 1024 >= kc.ks_rollout_lds(geo["narrow_256"]["f64"], 8, [5, 8, 1])
    assert any(served[n, p] and geo[n][p]["A"] % 2 for (n, p) in served)            # a column pair straddles the two trajectories
    assert any(served[n, p] and geo[n][p]["cells"] for (n, p) in served) and any(served[n, p] and geo[n][p]["consecutive"] for (n, p) in served)
    assert {geo[n][p]["engine"] for (n, p) in served if served[n, p]} == {"FftWave256", "FftFixed192", "FftFixed240", "FftGeneric"}
    # refused, each for its own reason
    for n in ("stack2_perm_256", "rewardcheck_256", "mono_256", "mono_192_wide", "fd_perm_256", "fd_irregular_256", "fd_midpoint_100"):
        assert not served[n, "f64"] and not served[n, "f32"], n
    for n in ("sparse_600", "subset_1024"):                                         # more than 64 KiB
        for p in PRECS:
            assert not served[n, p] and kc.ks_rollout_lds(geo[n][p], 8 if p == "f64" else 4, [3, 20, 1]) > 64 * 1024
    assert not served["ng4_4096", "f32"] and not served["ng4_2048", "f64"]
    assert served["nocheck_256", "f64"] and served["nocheck_256", "f32"]


@pytest.mark.parametrize("case", kc.BLOWUP)
def test_blowup_inputs_split_the_batch_in_the_oracle(built, case):
    """the blow-up test's inputs in the oracle: trajectory 1 (patched) ends the step finite and past max_value, trajectory 4 (one
    NaN cell) is NaN, the others are far inside the bound -- on the field, or on the reward under check_max_value "reward" """
    setup, cfg = built[case]
    c = kc.CASES[case]
    y0, bad, act, prev = kc.blowup_inputs(case)
    for b in range(5):
        with np.errstate(all="ignore"):
            y = kc.oracle_step(ks, cfg, case, bad[b], ks.prepare_action(cfg, act[b][None]))
            r = ks.reward_function(cfg, y, act[b][None], (act[b] - prev[b])[None])
        x = r if c.check_max_value == "reward" else y
        if b == 1:
            assert np.isfinite(y).all() and np.isfinite(r).all() and np.abs(x).max() > 1.2 * c.max_value
            assert np.abs(y).max() > 1.2 * 30 and np.abs(y).max() < 2 * kc.BLOWUP_PATCH
        elif b == 4:
            assert np.isnan(x).any() and kc.blown(x, c.max_value)
        else:
            assert np.abs(x).max() < 0.5 * c.max_value, (b, np.abs(x).max())
        assert kc.want_done(case, y, r) == (c.check_max_value != "off" and b in (1, 4))


def test_blowup_rows_cover_every_form_of_the_flag(geo):
    """the blow-up test patches the second half of a pair: its rows hold both actuation branches of the packed-pair step, an
    engine with more than one wave (block_max over waves), the global agent (one terminal column), all three check_max_value
    forms, and the one-trajectory-per-work-group finite-difference step"""
    rows = [(kc.CASES[n], geo[n]["f64"]) for n in kc.BLOWUP]
    assert {c.check_max_value for c, g in rows} == {"y", "reward", "off"}
    assert any(g["consecutive"] and not c.mono for c, g in rows) and any(g["cells"] for c, g in rows)
    assert any(g["nthreads"] > 64 and g["engine"].startswith("Fft") for c, g in rows) and any(c.mono for c, g in rows)
    assert any(c.integrator != "cnab2" for c, g in rows) and all(c.temporal_steps == 1 for c, g in rows)
    for n in kc.BLOWUP:                       # the patch on the last three cells lies under acting sensors
        setup_a2s = np.array(kc.CASES[n].actuators_to_sensors or range(1, geo[n]["f64"]["A"] + 1)) - 1
        pos = np.array(kc.CASES[n].sensor_positions)[setup_a2s if not kc.CASES[n].mono else slice(None)]
        d = np.abs(pos[:, None] - np.array([kc.CASES[n].nx - 2, kc.CASES[n].nx - 1, kc.CASES[n].nx])[None, :])
        assert np.minimum(d, kc.CASES[n].nx - d).min() <= 3, n


# ------------------------------------------------------------------ sensitivity: what a wrong kernel would move
def _one_step(case, cfg, y0, a, prev, cfg_step=None):
    y = kc.oracle_step(ks, cfg_step or cfg, case, y0, ks.prepare_action(cfg, a[None]))
    return y, ks.featurize(cfg, y, None), ks.reward_function(cfg, y, a[None], (a - prev)[None])


def _gpu_bounds(case, geo, y):
    """the GPU test's bounds at this field, the larger of the two dtypes"""
    ymax = float(np.abs(y).max())
    return dict(y=kc.tol_y("f32", case, y), state=max(kc.tol_state(p, case, geo[case][p], ymax) for p in PRECS),
                reward=max(kc.tol_reward(p, case, geo[case][p], ymax) for p in PRECS))


def test_wrong_but_plausible_variants_move_the_oracle_by_100_bounds(pkg, built, geo):
    margin, seen = 100.0, {}
    case = "perm_oddA_256"
    setup, cfg = built[case]
    c = kc.CASES[case]
    y0, act, prev = kc.inputs(case, 5)
    for b in range(5):
        a, ap = act[0, b], prev[b]
        y, st, r = _one_step(case, cfg, y0[b], a, ap)
        tol = _gpu_bounds(case, geo, y)
        p_tol = kc.tol_p("f32", ks.prepare_action(cfg, a[None]))
        # a2s sorted instead of permuted: sensing reads other sensors, actuation drives other cells
        srt = kc.build(pkg, ks, c._replace(actuators_to_sensors=tuple(sorted(c.actuators_to_sensors)),
                                           actuator_positions=tuple(sorted(c.actuator_positions))))[1]
        seen["a2s sorted: state"] = np.abs(ks.featurize(srt, y, None) - st).max() / tol["state"]
        seen["a2s sorted: reward"] = np.abs(ks.reward_function(srt, y, a[None], (a - ap)[None]) - r).max() / tol["reward"]
        seen["a2s sorted: p"] = np.abs(ks.prepare_action(srt, a[None]) - ks.prepare_action(cfg, a[None])).max() / p_tol
        # the window shift with its sign flipped: rows -w .. w of the state in the other order
        seen["window sign: state"] = np.abs(st[::-1] - st).max() / tol["state"]
        # action and previous action swapped in the reward
        seen["action <-> previous: reward"] = np.abs(ks.reward_function(cfg, y, ap[None], (ap - a)[None]) - r).max() / tol["reward"]
        # the two trajectories of a packed pair swapped
        partner = b ^ 1 if (b ^ 1) < 5 else 0
        y2, st2, r2 = _one_step(case, cfg, y0[partner], act[0, partner], prev[partner])
        seen["pair swapped: y"] = np.abs(y2 - y).max() / tol["y"]
        seen["pair swapped: state"] = np.abs(st2 - st).max() / tol["state"]
        seen["pair swapped: reward"] = np.abs(r2 - r).max() / tol["reward"]
        # mu with its sign flipped
        neg = copy.copy(cfg)
        neg.mu = -cfg.mu
        seen["mu sign: y"] = np.abs(_one_step(case, cfg, y0[b], a, ap, cfg_step=neg)[0] - y).max() / tol["y"]
        for k, v in seen.items():
            assert v >= margin, (b, k, v)
    # the general featurize path: a sorted a2s and the flipped window in the stacked state
    case = "stack2_perm_256"
    setup, cfg = built[case]
    c = kc.CASES[case]
    y0, act, prev = kc.inputs(case, 5)
    srt = kc.build(pkg, ks, c._replace(actuators_to_sensors=tuple(sorted(c.actuators_to_sensors)),
                                       actuator_positions=tuple(sorted(c.actuator_positions))))[1]
    for b in range(5):
        y, st, r = _one_step(case, cfg, y0[b], act[0, b], prev[b])
        tol = _gpu_bounds(case, geo, y)
        assert np.abs(ks.featurize(srt, y, None) - st).max() >= margin * tol["state"]
        assert np.abs(st[:5][::-1] - st[:5]).max() >= margin * tol["state"]
    # mono: the reward sum divided by S instead of A
    for case in ("mono_256", "mono_192_wide"):
        setup, cfg = built[case]
        y0, act, prev = kc.inputs(case, 5)
        S, A = len(cfg.sensor_positions), len(cfg.actuator_positions)
        for b in range(5):
            y, st, r = _one_step(case, cfg, y0[b], act[0, b], prev[b])
            tol = _gpu_bounds(case, geo, y)
            assert abs(r[0] * A / S - r[0]) >= margin * tol["reward"], (case, b, r, tol)
    print("[ks-geometry sensitivity] variant / bound, perm_oddA_256, last trajectory:", {k: round(float(v)) for k, v in seen.items()})
