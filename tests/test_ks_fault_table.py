"""The table of test_gpu_ks_faults.py (ks_fault_cases.py) and its reference (ks_fault_ref.py) held against oracle/ks.py, without a
GPU: the rows reach what the feature has to reach, the fault arrays are what the GPU test needs, the reference with gains of one
and a bias of zero IS the oracle's env_step, the inputs stay tame, and every mistake the feature invites -- the partner's or the
neighbour's arrays, sensor faults indexed by the actuator, the bias added behind the scale, the faults let into the reward's dots or
into the punished action -- moves ONE control step of the reference by a stated multiple of the GPU test's fp32 bound.  And the host
side of the feature: the entry is declared, exported and bound, KSSetup.fault_scenario, the block layout of
evaluate_actors(faults=...)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import ks_fault_cases as fc
import ks_fault_ref as fr
import ks_geometry_cases as kc
from oracle import ks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built(pkg):
    out = {}
    for case in fc.STEP_ROWS:
        setup, cfg = kc.build(pkg, ks, case)
        # the cases file and the product agree on what a row's sizes are and on what "healthy" is
        sc, h = setup.fault_scenario(), fc.healthy(case)
        assert fc.sizes(case) == (setup.n_actuators, setup.n_sensors)
        assert all(np.array_equal(sc[k], h[k][0]) and sc[k].dtype == np.float64 for k in fc.KEYS), case
        assert all(np.array_equal(sc[k], np.full_like(sc[k], fc.HEALTHY_VALUE[k])) for k in fc.KEYS)
        out[case] = (setup, cfg, kc.geometry(*setup.tables(), case, "f32"))
    return out


def _rows(f, b):
    return tuple(f[k][b] for k in fc.KEYS)


# ------------------------------------------------------------------ the table
def test_the_rows_are_what_the_gpu_test_needs(built):
    rows = [kc.CASES[c] for c in fc.STEP_ROWS]
    assert set(fc.STEP_ROWS) <= set(kc.CASES) and not any(c.mono for c in rows)
    assert {c.integrator for c in rows} == {"cnab2", "rk4_fd", "midpoint_fd"}
    assert {kc.engine(c.nx) for c in rows if c.integrator == "cnab2"} == {"FftWave256", "FftFixed192", "FftGeneric", "FftWave1024"}
    fd = [c for c in rows if c.integrator != "cnab2"]
    assert {kc.nthreads(c.nx, c.integrator) == 64 for c in fd} == {True, False}       # the one-wave kernel and the general one

    def permuted(c):
        a2s = c.actuators_to_sensors
        return a2s is not None and len(a2s) != len(c.sensor_positions) and not np.all(np.diff(a2s) > 0)
    assert any(permuted(c) for c in rows)                              # A != S and a non-monotone actuators_to_sensors
    assert any(c.window_size > 1 for c in rows)                        # a window row reads a neighbouring sensor
    assert any(c.temporal_steps == 2 for c in rows)                    # rows copied from the previous state
    assert any(c.temporal_steps == 1 for c in rows if c.integrator == "cnab2")         # featurize_pair / the fmap gather
    assert kc.CASES[fc.ROLL_CASE].integrator == "cnab2" and fc.ROLL_CASE in kc.ROLL_MUST_SERVE and fc.ROLL_CASE in fc.STEP_ROWS
    assert 0 < fc.ROLL_FROM < fc.ROLL_T == 8 and fc.STEPS == 3
    for case in fc.STEP_ROWS:
        A, S = built[case][0].n_actuators, built[case][0].n_sensors
        assert 4 <= A <= S, case                                       # fr.featurize(wrong="actuator_index") reads entry a < S


@pytest.mark.parametrize("case", fc.STEP_ROWS)
def test_the_fault_arrays_are_what_the_gpu_test_needs(built, case):
    f, B = fc.faults(case), fc.batch(case)
    A, S = built[case][0].n_actuators, built[case][0].n_sensors
    assert B % 2 == 1 and B == (3 if kc.CASES[case].nx == 1024 else 5)          # the last trajectory is alone in its work-group
    assert [f[k].shape for k in fc.KEYS] == [(B, A), (B, S), (B, S)]
    h = fc.healthy(case)
    for k in fc.KEYS:
        x = f[k]
        assert np.array_equal(x[fc.HEALTHY], h[k][fc.HEALTHY])                  # one trajectory is fully healthy
        # within a packed pair the two trajectories differ in every ENTRY of every array, the lone last one from both of its
        # neighbours (the one before it and, around the batch, the first) -- every two trajectories do
        for a in range(B):
            for b in range(a + 1, B):
                assert np.abs(x[a] - x[b]).min() >= fc.APART - 1e-12, (k, a, b)
        # no trajectory carries the batch mean of any array, entry by entry (the healthy one is not asked: its values are given)
        off = np.abs(x - x.mean(axis=0))
        assert np.delete(off, fc.HEALTHY, axis=0).min() >= fc.APART - 1e-12, k
        assert not np.allclose(x[fc.HEALTHY], x.mean(axis=0))
    assert len(fc.pairs(case)) == B // 2 and all(b == a + 1 for a, b in fc.pairs(case)) and fc.HEALTHY < B
    ag, sg, sb = (f[k] for k in fc.KEYS)
    assert (ag == 0).any() and (sg == 0).any()                                  # dead
    assert (ag > 1).any() and (sg > 1).any() and (ag < 0).any()                 # above 1, reversed
    assert (sb > 0).any() and (sb < 0).any()                                    # biases of both signs
    # the same arrays every time
    g = fc.faults(case)
    assert all(np.array_equal(f[k], g[k]) for k in fc.KEYS)


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("case", fc.STEP_ROWS)
def test_healthy_arrays_are_the_oracle_exactly(built, case):
    """gains of one and a bias of zero: ks_fault_ref.env_step equals oracle/ks.py's env_step, every bit (the finite-difference
    rows: the same pieces with the row's integrator, which env_step does not take)"""
    setup, cfg, _ = built[case]
    B = fc.batch(case)
    y0, act, prev = kc.inputs(case, B, steps=2)
    h = fc.healthy(case)
    for b in range(B):
        st = None
        y, ap = y0[b], prev[b]
        for t in range(2):
            got = fr.env_step(ks, cfg, case, y, ap, act[t, b], *_rows(h, b), prev_state=st)
            if kc.CASES[case].integrator == "cnab2":
                want = ks.env_step(cfg, y, ap[None], act[t, b][None], 0.0, prev_state=st)
            else:
                p = ks.prepare_action(cfg, act[t, b][None])
                yn = kc.oracle_step(ks, cfg, case, y, p)
                want = dict(y=yn, p=p, reward=ks.reward_function(cfg, yn, act[t, b][None], (act[t, b] - ap)[None]),
                            state=ks.featurize(cfg, yn, st))
            for k in ("y", "p", "reward", "state"):
                assert np.array_equal(got[k], want[k]), (b, t, k)
            y, ap, st = got["y"], act[t, b], got["state"]


@pytest.mark.parametrize("case", fc.STEP_ROWS)
def test_inputs_stay_tame_under_the_faults(built, case):
    """free-running in the reference for the longest run of the GPU test (ROLL_T steps: the step tests' STEPS actions, then zero
    actions), every trajectory through its own actuator gains"""
    setup, cfg, _ = built[case]
    B, f = fc.batch(case), fc.faults(case)
    y0, act, prev = kc.inputs(case, B, steps=fc.STEPS)
    for b in range(B):
        y, ap = y0[b], prev[b]
        for t in range(fc.ROLL_T):
            a = act[t, b] if t < fc.STEPS else np.zeros_like(prev[b])
            y, ap = fr.env_step(ks, cfg, case, y, ap, a, *_rows(f, b))["y"], a
            assert np.isfinite(y).all() and np.abs(y).max() < 6.0, (b, t, float(np.abs(y).max()))
        assert np.abs(y).max() < 0.5 * kc.CASES[case].max_value


@pytest.mark.parametrize("case", fc.STEP_ROWS)
def test_every_mistake_moves_one_step_by_many_bounds(built, case):
    setup, cfg, geo = built[case]
    B, f = fc.batch(case), fc.faults(case)
    y0, act, prev = kc.inputs(case, B, steps=1)
    need = fc.MIN_BOUNDS

    def step(b, rows, wrong=None):
        return fr.env_step(ks, cfg, case, y0[b], prev[b], act[0, b], *rows, wrong=wrong)

    ref = [step(b, _rows(f, b)) for b in range(B)]
    ymax = [float(np.abs(r["y"]).max()) for r in ref]
    # the bounds of the fp32 comparison at the reference's own new field
    t_p = [kc.tol_p("f32", r["p"]) for r in ref]
    t_y = [kc.tol_y("f32", case, r["y"]) for r in ref]
    t_s = [fc.tol_state("f32", case, geo, ymax[b], float(np.abs(f["sensor_gain"][b]).max()), float(np.abs(f["sensor_bias"][b]).max()))
           for b in range(B)]
    t_r = [kc.tol_reward("f32", case, geo, ymax[b]) for b in range(B)]

    def moved(a, b, key):
        return float(np.abs(a[key] - b[key]).max())

    worst = {}

    def hold(name, value, bound, who):
        worst[name] = min(worst.get(name, np.inf), value / bound)
        assert value >= need * bound, (name, who, value, bound)

    # 1. another trajectory's arrays: the partner of the packed pair, the neighbours of the lone last one (and, where a work-group
    # holds one trajectory, of everyone), one array at a time
    others = set()
    for a, b in fc.pairs(case):
        others |= {(a, b), (b, a)}
    others |= {(B - 1, B - 2), (B - 1, 0), (B - 2, B - 1)}
    for me, other in sorted(others):
        for i, k in enumerate(fc.KEYS):
            rows = list(_rows(f, me))
            rows[i] = f[k][other]
            got = step(me, tuple(rows))
            if k == "actuator_gain":
                hold("other:p", moved(got, ref[me], "p"), t_p[me], (me, other))
                hold("other:y", moved(got, ref[me], "y"), t_y[me], (me, other))
            else:
                hold("other:state:" + k, moved(got, ref[me], "state"), t_s[me], (me, other))
    # 2. - 5. the four mistakes of ks_fault_ref.WRONG, on every trajectory that carries faults
    for b in range(B):
        if b == fc.HEALTHY:
            for w in fr.WRONG:          # nothing to get wrong: the healthy trajectory is the oracle under every one of them
                got = step(b, _rows(f, b), w)
                assert all(moved(got, ref[b], k) < 1e-12 for k in ("p", "y", "state", "reward")), w
            continue
        hold("actuator_index", moved(step(b, _rows(f, b), "actuator_index"), ref[b], "state"), t_s[b], b)
        hold("bias_after_scale", moved(step(b, _rows(f, b), "bias_after_scale"), ref[b], "state"), t_s[b], b)
        hold("reward_sees_faults", moved(step(b, _rows(f, b), "reward_sees_faults"), ref[b], "reward"), t_r[b], b)
        hold("punish_applied_action", moved(step(b, _rows(f, b), "punish_applied_action"), ref[b], "reward"), t_r[b], b)
    print(f"[ks-fault table {case}] movement in fp32 bounds, least per mistake:", {k: round(v, 1) for k, v in worst.items()})


def test_the_state_bound_extends_the_healthy_one(built):
    for case in fc.STEP_ROWS:
        geo = built[case][2]
        for prec in ("f64", "f32"):
            base = kc.tol_state(prec, case, geo, 2.0)
            assert fc.tol_state(prec, case, geo, 2.0, 1.0, 0.0) == pytest.approx(base * (geo["Wd"] + 5) / (geo["Wd"] + 3))
            assert fc.tol_state(prec, case, geo, 2.0, 1.5, 0.5) == pytest.approx(base * (geo["Wd"] + 5) / (geo["Wd"] + 3) * 3.5 / 2.0)


# ------------------------------------------------------------------ the host side
def test_entry_is_declared_exported_and_bound(pkg):
    lib = ctypes.CDLL(pkg._lib.LIB_PATH)
    raw = open(os.path.join(ROOT, "include", "pdeconv.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    name = "pdec_env_set_faults"
    assert hasattr(lib, name)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)
    assert m and len(m.group(1).split(",")) == 4 == len(pkg._lib.SIGNATURES[name])
    # the comment in front of it cites the closures it modifies
    before = raw[:raw.index("int " + name)]
    assert "KSSetup.jl:190-245" in before[before.rindex("/*"):]
    jl = open(os.path.join(ROOT, "julia", "PDEenvHIP.jl")).read()
    cc = re.search(r"ccall\(\(:" + name + r", LIB\), Cint, \(([^)]*)\)", jl)
    assert cc and [t.strip() for t in cc.group(1).split(",")] == ["UInt64", "Ptr{Cvoid}", "Ptr{Cvoid}", "Ptr{Cvoid}"]
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sig = inspect.signature(pkg.PDEenv.set_faults).parameters
    assert [k for k in sig if k != "self"] == list(fc.KEYS) and all(sig[k].default is None for k in fc.KEYS)
    assert inspect.signature(pkg.evaluate_actors).parameters["faults"].default is None


def test_fault_scenario(pkg):
    setup, _ = kc.build(pkg, ks, "perm_oddA_256")
    A, S = fc.sizes("perm_oddA_256")
    sc = setup.fault_scenario()
    assert sorted(sc) == sorted(fc.KEYS)
    assert np.array_equal(sc["actuator_gain"], np.ones(A)) and np.array_equal(sc["sensor_gain"], np.ones(S))
    assert np.array_equal(sc["sensor_bias"], np.zeros(S)) and all(v.dtype == np.float64 for v in sc.values())
    # numbered from 1, as actuators_to_sensors is
    sc = setup.fault_scenario(dead_actuators=(1, A), dead_sensors=[17])
    assert np.flatnonzero(sc["actuator_gain"] == 0).tolist() == [0, A - 1] and np.flatnonzero(sc["sensor_gain"] == 0).tolist() == [16]
    assert sc["actuator_gain"].sum() == A - 2 and sc["sensor_gain"].sum() == S - 1 and not sc["sensor_bias"].any()
    # given arrays are the base (copied), the dead ones are zeroed on top
    g = np.full(S, 1.2)
    sc = setup.fault_scenario(sensor_gain=g, sensor_bias=np.arange(S) * 0.01, dead_sensors=(2,))
    assert sc["sensor_gain"][1] == 0 and sc["sensor_gain"][0] == 1.2 and g[1] == 1.2 and sc["sensor_bias"][3] == 0.03
    for kw, word in ((dict(dead_actuators=(0,)), "dead_actuators"), (dict(dead_actuators=(A + 1,)), "dead_actuators"),
                     (dict(dead_sensors=(S + 1,)), "dead_sensors"), (dict(dead_sensors=(-1,)), "dead_sensors"),
                     (dict(actuator_gain=np.ones(A + 1)), "actuator_gain"), (dict(sensor_gain=np.ones((1, S))), "sensor_gain"),
                     (dict(sensor_bias=np.zeros(A)), "sensor_bias")):
        with pytest.raises(pkg.PdecError, match=word):
            setup.fault_scenario(**kw)


class _StubEnv:
    """what evaluate_actors asks of its B = M n_f K environment, recorded"""
    made = []

    def __init__(self, setup, B, **kw):
        self.setup, self.B, self.calls = setup, B, []
        _StubEnv.made.append(self)

    def set_faults(self, **kw):
        self.calls.append(("set_faults", {k: np.asarray(v) for k, v in kw.items()}))
        raise _Stop()

    def close(self):
        pass


class _Stop(Exception):
    pass


def test_evaluate_actors_lays_the_scenarios_out_as_mu_is(pkg, monkeypatch):
    """B = M n_f K, member m's block [n_f][K]: trajectory (m, f, k) carries scenario f -- seen on a stub environment, no GPU"""
    import types
    pop = __import__(pkg.__name__ + ".population_eval", fromlist=["x"])     # (the module whose names evaluate_actors reads)
    torch = pytest.importorskip("torch")
    setup, _ = kc.build(pkg, ks, "perm_oddA_256")
    A, S = fc.sizes("perm_oddA_256")
    M, K = 3, 2
    scen = [setup.fault_scenario(), setup.fault_scenario(dead_actuators=(2,), sensor_bias=np.full(S, 0.5)),
            dict(sensor_gain=np.full(S, 1.2))]
    _StubEnv.made = []
    monkeypatch.setattr(pop, "PDEenv", _StubEnv)
    monkeypatch.setattr(pop, "_model", lambda a: a)
    monkeypatch.setattr(pop, "_has_persistent_rollout", lambda s: True)
    actors = [types.SimpleNamespace(dims=[3, 4, 1], acts=["relu", "tanh"]) for _ in range(M)]
    y0 = torch.zeros((K, setup.nx), dtype=torch.float64)
    with pytest.raises(_Stop):
        pop.evaluate_actors(setup, actors, y0=y0, device="cpu", steps=2, faults=scen)
    env = _StubEnv.made[-1]
    assert env.B == M * len(scen) * K
    (name, arrs), = env.calls
    assert name == "set_faults" and sorted(arrs) == sorted(fc.KEYS)
    full = [setup.fault_scenario(**s) for s in scen]
    for k in fc.KEYS:
        assert arrs[k].shape == (env.B, A if k == "actuator_gain" else S)
        for m in range(M):
            for f in range(len(scen)):
                for j in range(K):
                    assert np.array_equal(arrs[k][(m * len(scen) + f) * K + j], full[f][k]), (k, m, f, j)
    # refusals by name, before any environment is made
    n = len(_StubEnv.made)
    with pytest.raises(pkg.PdecError, match="faults together with mu"):
        pop.evaluate_actors(setup, actors, y0=y0, device="cpu", faults=scen, mu=[0.0])
    with pytest.raises(pkg.PdecError, match="faults is empty"):
        pop.evaluate_actors(setup, actors, y0=y0, device="cpu", faults=[])
    with pytest.raises(pkg.PdecError, match="unknown keys"):
        pop.evaluate_actors(setup, actors, y0=y0, device="cpu", faults=[dict(gain=np.ones(A))])
    with pytest.raises(pkg.PdecError, match="sensor_gain"):
        pop.evaluate_actors(setup, actors, y0=y0, device="cpu", faults=[dict(sensor_gain=np.ones(A))])
    assert len(_StubEnv.made) == n
