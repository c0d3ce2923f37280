"""GPU tests of TrainPipeline(telemetry=N): KS22 geometry, fp32, episodes of E = 7 (the shape of the n-step tests).  The
teacher-forced run of tests/pipeline_ref.py with every step row held to telemetry_ref.step_row of that step's recorded arrays and
every update row to telemetry_ref.update_row of the consecutive parameter snapshots and losses; recorded steps and captured graphs
against it, bit for bit; telemetry_every; per-trajectory episodes with a trajectory that blows up; the default path; a NaN written
into a weight between two run() calls; one Keller-Segel and one fluid pipeline; refusals."""
import warnings

import numpy as np
import pytest
import torch

from nstep_ref import first_update_steps
from pipeline_ref import _same_snap, record_step, run_teacher_forced
from telemetry_ref import STEP_COLUMNS, UPDATE_COLUMNS, mismatches, step_row, update_row

pytestmark = pytest.mark.gpu

E, LAG = 7, 2
STEPS = 3 * E + 5
CAP = 64


def _make(pkg, B=64, E=E, graphs=False, y0=None, setup_kw=None, act_noise=0.3, **kw):
    setup = pkg.KSSetup.KS22(**(setup_kw or {}))
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    if y0 is None:
        y0 = setup.generate_random_init(np.random.default_rng(0), B) * 0.15
    env = pkg.PDEenv(setup, B=B, dtype=torch.float32, y0=y0, stream=s_env, autoreset=False)
    agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                             noise_seed=7, trajectory_length=1)
    agent.policy.act_noise = act_noise
    torch.cuda.synchronize()
    return pkg.TrainPipeline(env, agent, lag=LAG, episode_steps=E, stream_env=s_env, stream_upd=s_upd, use_graphs=graphs,
                             chunks=(6, 1), noise_seed=99, **kw)


def _reset_field(pipe, seed):
    y = pipe.env.setup.generate_random_init(np.random.default_rng(seed), pipe.env.B) * 0.15
    t = torch.as_tensor(y, dtype=pipe.env.dtype, device=pipe.env.device)
    torch.cuda.synchronize()
    return t


def _row(cols, i):
    return {k: v[i] for k, v in cols.items()}


def _same_rings(a, b):
    """two telemetry() results, bit for bit"""
    assert {k: v for k, v in a.items() if k not in ("step", "update")} == {k: v for k, v in b.items() if k not in ("step", "update")}
    for ring in ("step", "update"):
        assert set(a[ring]) == set(b[ring])
        for k in a[ring]:
            assert a[ring][k].tobytes() == b[ring][k].tobytes(), (ring, k)


def _same_state(pkg, rec, pipe, k):
    got = record_step(pkg, pipe, k)
    assert _same_snap(rec.snap, got.snap)                                  # four networks, ADAM moments, beta powers
    assert np.array_equal(np.asarray(rec.snap.losses), np.asarray(got.snap.losses), equal_nan=True)
    assert rec.ctr == got.ctr                                              # the noise counter
    for name in ("y_in", "y_out", "s_in", "s_out", "a", "r", "t", "flags"):
        assert np.array_equal(getattr(rec, name), getattr(got, name)), name


def _check_trace(pipe, trace, tel, updating, every=1):
    """every row of both rings against the model fed with the trace's arrays; `updating`: the steps that carried an update"""
    bad = []
    lim = float(pipe.policy.act_limit)
    assert tel["dropped_steps"] == 0 and tel["step"]["step"].tolist() == list(range(len(trace.steps)))
    for k, rec in enumerate(trace.steps):
        want, tol = step_row(rec.s_out, rec.a, rec.r, rec.t, rec.flags, lim, step=k)
        bad += mismatches(_row(tel["step"], k), want, tol, STEP_COLUMNS, f"step {k}: ")
    assert np.array_equal(tel["step"]["action_saturated_fraction"], tel["step"]["action_saturated"] / pipe.cols)
    recorded = [k for k in updating if k % every == 0]
    assert tel["dropped_updates"] == 0 and tel["update"]["update"].tolist() == list(range(len(recorded)))
    prev = None
    for u, k in enumerate(recorded):
        snap = trace.steps[k].snap
        want, tol = update_row(snap.losses, snap.A, snap.C, snap.At, snap.Ct, None if prev is None else prev.A,
                               None if prev is None else prev.C, update=u)
        bad += mismatches(_row(tel["update"], u), want, tol, UPDATE_COLUMNS, f"update {u} (step {k}): ")
        prev = snap
    return bad


@pytest.mark.parametrize("B,n_step", [(64, 1), (3, 1), (64, 3), (3, 3)])
def test_teacher_forced_run(pkg, B, n_step):
    """3 E + 5 steps with a reset_from in mid-episode (tick 10), every step and every update row held to the model; `update` counts
    only the steps that updated (n_step = 3: two steps later after every restart), `step` counts on across reset_from; then the same
    run without a synchronisation between the steps (recorded steps): the same rings bit for bit"""
    p = _make(pkg, B=B, n_step=n_step, telemetry=CAP)
    trace = run_teacher_forced(pkg, p, STEPS, {10: _reset_field(p, 3)})
    tel = p.telemetry()
    updating = first_update_steps(trace.resets, STEPS, LAG, n_step)
    assert updating == (list(range(2, 10)) + list(range(12, STEPS)) if n_step == 1 else list(range(4, 10)) + list(range(14, STEPS)))
    bad = _check_trace(p, trace, tel, updating)
    assert bad == [], bad[:10]
    assert tel["first_nonfinite_step"] is None and tel["first_nonfinite_update"] is None
    up = tel["update"]
    assert up["actor_step2"][0] == 0 == up["critic_step2"][0] and (up["actor_step2"][1:] > 0).all() and (up["critic_step2"][1:] > 0).all()
    # time-out rows: the last step of every lock-stepped episode is terminal in every column
    ends = [k for k in range(STEPS) if (k < 10 and k % E == E - 1) or (k >= 10 and (k - 10) % E == E - 1)]
    assert [k for k in range(STEPS) if tel["step"]["terminal"][k] == p.cols] == ends
    q = _make(pkg, B=B, n_step=n_step, telemetry=CAP)
    q.run(10)
    q.reset_from(_reset_field(q, 3))
    q.run(STEPS - 10)
    assert q._progs and any("telemetry_update" in f.__name__ for f, _ in q._progs[max(q._progs)])
    _same_rings(tel, q.telemetry())
    p.close()
    q.close()


@pytest.mark.parametrize("every", [1, 2])
def test_graphs_equal_eager_steps(pkg, every):
    """captured chunks of 6 and 1 steps (per-trajectory episodes, as the n-step graph test: capture() needs lock-stepped episodes
    longer than two ring periods) against eager steps: the learner, the fields and both rings bit for bit.  telemetry_every = 2 puts an
    odd number of update calls into a six-step chunk, which the rings' device counters must not care about."""
    kw = dict(E=7, episodes="per_trajectory", stagger=True, log_episodes=8, telemetry=CAP, telemetry_every=every)
    pg = _make(pkg, graphs=True, **kw)
    pe = _make(pkg, graphs=False, **kw)
    assert pg.use_graphs
    pg.run(3)
    pg.capture()
    assert pg._captured and pg.graphs
    launched, t0 = pg.n_graph_launches, pg.tick
    pg.run(STEPS)
    assert pg.n_graph_launches > launched
    n = pg.tick
    assert n == t0 + STEPS
    pe.fast_eager = False
    pe.run(n)
    pg.sync(); pe.sync()
    _same_state(pkg, record_step(pkg, pe, n - 1), pg, n - 1)
    tg, te = pg.telemetry(), pe.telemetry()
    _same_rings(tg, te)
    assert tg["dropped_steps"] == n - CAP and tg["step"]["step"][-1] == n - 1
    assert tg["update"]["update"][-1] == len([k for k in range(LAG, n) if k % every == 0]) - 1
    assert np.isfinite(tg["update"]["critic_loss"]).all() and (tg["update"]["actor_step2"][1:] > 0).all()
    pg.close()
    pe.close()


def test_lockstep_graphs_on_the_fused_route(pkg):
    """C2 geometry (fused 3-layer nets: the events the env stream waits for ride on the update's own launches), B = 64, lock-stepped
    episodes of E = 14, chunks of 6 and 1 with eager first and last steps between them: the teacher-forced run of as many steps,
    every row held to the model, and the run through captured graphs gives its rings bit for bit -- every eager step that is
    followed by a chunk leaves a telemetry launch behind its update that the chunk must be ordered behind"""
    def make(graphs):
        setup = pkg.KSSetup.bench_C2(256)
        s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
        y0 = setup.generate_random_init(np.random.default_rng(0), 64) * 0.15
        env = pkg.PDEenv(setup, B=64, dtype=torch.float32, y0=y0, stream=s_env, autoreset=False)
        agent = pkg.create_agent(setup=setup, B=64, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                                 noise_seed=7, trajectory_length=1)
        agent.policy.act_noise = 0.3
        torch.cuda.synchronize()
        return pkg.TrainPipeline(env, agent, lag=LAG, episode_steps=14, stream_env=s_env, stream_upd=s_upd, use_graphs=graphs,
                                 chunks=(6, 1), noise_seed=99, telemetry=256)

    pg = make(True)
    assert pg.use_graphs and pg.rpart is not None and pg.stop_events
    pg.run(3)
    pg.capture()
    launched = pg.n_graph_launches
    pg.run(2 * 14 + 5)
    assert pg.n_graph_launches > launched and pg.n_eager_steps > 3
    n = pg.tick
    assert n <= 256
    tg = pg.telemetry()
    p = make(False)
    trace = run_teacher_forced(pkg, p, n, None)
    tel = p.telemetry()
    bad = _check_trace(p, trace, tel, list(range(LAG, n)))
    assert bad == [], bad[:10]
    _same_rings(tel, tg)
    _same_state(pkg, trace.steps[-1], pg, n - 1)
    assert [k for k in range(n) if tel["step"]["terminal"][k] == p.cols] == list(range(13, n, 14))
    pg.close()
    p.close()


def test_every_third_step(pkg):
    """telemetry_every = 3: an update row at the updating steps k with k % 3 == 0 only, step2 against the snapshot of the previous
    recorded update -- three updates back; the step row at every step"""
    p = _make(pkg, B=3, telemetry=CAP, telemetry_every=3)
    trace = run_teacher_forced(pkg, p, STEPS, None)
    tel = p.telemetry()
    updating = list(range(LAG, STEPS))
    bad = _check_trace(p, trace, tel, updating, every=3)
    assert bad == [], bad[:10]
    assert len(tel["update"]["update"]) == len(range(3, STEPS, 3)) == 8
    p.close()


def test_per_trajectory_episodes_show_a_blow_up(pkg):
    """B = 8, staggered clocks, max_value = 1.5 (rows 5 and 7 blow up after a step: tests/test_gpu_episode_clock.py): every step
    row equals the model of the ring slots as the clock leaves them; blown_up and terminal show the blow-up in its step, and the
    reward the clock has sanitised leaves reward_nonfinite = 0"""
    B = 8
    setup = pkg.KSSetup.KS22(max_value=1.5)
    y0 = setup.generate_random_init(np.random.default_rng(0), B) * (0.05 * (np.arange(B) % 8 + 1))[:, None]
    p = _make(pkg, B=B, y0=y0, setup_kw=dict(max_value=1.5), act_noise=0.1, episodes="per_trajectory", stagger=True,
              log_episodes=8, telemetry=CAP)
    rows = []
    for k in range(STEPS):
        p.run(1)
        p.sync()
        rows.append(record_step(pkg, p, k))
    tel = p.telemetry()
    bad = []
    for k, rec in enumerate(rows):
        want, tol = step_row(rec.s_out, rec.a, rec.r, rec.t, rec.flags, float(p.policy.act_limit), step=k)
        bad += mismatches(_row(tel["step"], k), want, tol, STEP_COLUMNS, f"step {k}: ")
    assert bad == [], bad[:10]
    st = tel["step"]
    blew = np.array([int((r.flags != 0).sum()) for r in rows])
    assert blew.max() > 0 and np.array_equal(st["blown_up"], blew)
    A = p.cols // B
    for k in np.nonzero(blew)[0]:
        assert st["terminal"][k] >= blew[k] * A                      # every column of a blown-up trajectory is terminal in that step
    assert (st["reward_nonfinite"] == 0).all() and tel["first_nonfinite_step"] is None
    fin = p.finished_episodes()
    assert fin["blew_up"].any() and st["terminal"].sum() == A * (len(fin["ret"]) + fin["dropped"])      # one terminal row per finished episode
    p.close()


def test_default_path_builds_nothing_and_telemetry_changes_nothing(pkg):
    on, off, dflt = _make(pkg, telemetry=CAP), _make(pkg, telemetry=0), _make(pkg)
    for p in (off, dflt):
        assert p._telem is None and p.telemetry_capacity == 0
        with pytest.raises(pkg.PdecError, match=r"telemetry is off \(telemetry=0\)"):
            p.telemetry()
    for p in (on, off, dflt):
        p.run(STEPS)
        p.sync()
    # the networks, the ADAM state, the fields and the noise counter: bit for bit the run without telemetry
    rec = record_step(pkg, off, STEPS - 1)
    _same_state(pkg, rec, on, STEPS - 1)
    _same_state(pkg, rec, dflt, STEPS - 1)
    assert len(on._progs) == len(off._progs) == len(dflt._progs) > 0
    for k in off._progs:
        names = [f.__name__ for f, _ in off._progs[k]]
        assert names == [f.__name__ for f, _ in dflt._progs[k]] and not any("telemetry" in n for n in names)
        with_tel = [f.__name__ for f, _ in on._progs[k]]
        assert [n for n in with_tel if "telemetry" not in n] == names
        assert sorted(n for n in with_tel if "telemetry" in n) == ["pdec_telemetry_step", "pdec_telemetry_update"]
    for p in (on, off, dflt):
        p.close()


def test_a_nan_written_into_a_weight_is_seen(pkg):
    """divergence is seen, not provoked: between two run() calls the host writes a NaN into one critic weight.  The next update's
    row counts it, first_nonfinite_update names that update and stays"""
    p = _make(pkg, B=3, telemetry=CAP)
    p.run(12)
    before = p.telemetry()
    assert before["first_nonfinite_update"] is None and len(before["update"]["update"]) == 12 - LAG
    m = p.policy.behavior_critic.model
    par = m.params()
    par[0][0, 0] = np.nan
    m.set_params(par)
    p.run(4)
    tel = p.telemetry()
    u = 12 - LAG
    assert tel["first_nonfinite_update"] == u
    assert tel["update"]["critic_nonfinite"][u] >= 1 and (tel["update"]["critic_nonfinite"][:u] == 0).all()
    assert np.isfinite(tel["update"]["critic_norm2"]).all()          # the NaN entries are left out of the sums
    # reset clears it (the parameters repaired first, so that nothing non-finite is left behind for a later test's eyes)
    for net in ("behavior_actor", "behavior_critic", "target_actor", "target_critic"):
        mdl = getattr(p.policy, net).model
        mdl.set_params([np.nan_to_num(x, nan=0.01) for x in mdl.params()])
    p.sync()
    p.telemetry_reset()
    assert p.telemetry()["first_nonfinite_update"] is None and len(p.telemetry()["step"]["step"]) == 0
    p.close()


def test_keller_segel_and_fluid_fill_their_rings(pkg):
    """one short 2-D Keller-Segel and one small fluid pipeline (eager only): finite rows of the right counts"""
    from fluid_ic_ref import fields_of, mem, pair, vortex_table
    from pipeline_fluid_ref import fluid_config

    def check(p, n):
        p.run(n)
        tel = p.telemetry()
        assert tel["step"]["step"].tolist() == list(range(n)) and tel["update"]["update"].tolist() == list(range(n - LAG))
        for ring in ("step", "update"):
            for k, v in tel[ring].items():
                assert np.isfinite(v).all(), (ring, k)
        assert tel["first_nonfinite_step"] is None and tel["first_nonfinite_update"] is None
        assert (tel["step"]["state_abs_max"] > 0).all() and (tel["update"]["actor_norm2"] > 0).all()
        assert (tel["step"]["terminal"] == np.where(np.arange(n) % 7 == 6, p.cols, 0)).all()
        p.close()

    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    setup = pkg.KellerSegel2DSetup(nx=64, ny=64)
    env = pkg.PDEenv(setup, B=4, dtype=torch.float32, stream=s_env, autoreset=False)
    agent = pkg.create_agent(setup=setup, B=4, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                             noise_seed=7, trajectory_length=1)
    agent.policy.act_noise = 0.3
    torch.cuda.synchronize()
    check(pkg.TrainPipeline(env, agent, lag=LAG, episode_steps=7, stream_env=s_env, stream_upd=s_upd, use_graphs=False,
                            noise_seed=99, telemetry=16), 9)

    setup, _ = pair(pkg, 32, 4)
    cfg = fluid_config(setup)
    y0 = mem(fields_of(cfg, vortex_table(21, 0, 4, 3, cfg.Lx))).astype(np.float32)
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    env = pkg.PDEenv(setup, B=4, dtype=torch.float32, y0=torch.as_tensor(y0, dtype=torch.float32, device="cuda:0"), stream=s_env,
                     autoreset=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        agent = pkg.create_agent(setup=setup, B=4, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                                 noise_seed=7, trajectory_length=1)
    agent.policy.act_noise = 0.3
    torch.cuda.synchronize()
    check(pkg.TrainPipeline(env, agent, lag=LAG, episode_steps=7, stream_env=s_env, stream_upd=s_upd, use_graphs=True,
                            noise_seed=99, telemetry=16), 9)


def test_refusals_by_name(pkg):
    setup = pkg.KSSetup.KS22()
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    env = pkg.PDEenv(setup, B=2, dtype=torch.float32, stream=s_env, autoreset=False)
    agent = pkg.create_agent(setup=setup, B=2, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                             noise_seed=7, trajectory_length=1)
    kw = dict(lag=LAG, episode_steps=E, stream_env=s_env, stream_upd=s_upd, use_graphs=False)
    for bad in (-1, 2.5, "8", True):
        with pytest.raises(pkg.PdecError, match=r"telemetry=.*an integer >= 0"):
            pkg.TrainPipeline(env, agent, telemetry=bad, **kw)
    for bad in (0, 4, 12, 1.0):
        with pytest.raises(pkg.PdecError, match=r"telemetry_every=.*one of 1, 2, 3, 6"):
            pkg.TrainPipeline(env, agent, telemetry=8, telemetry_every=bad, **kw)
    red = pkg.distributed.NativeGradReducer(pkg._lib.init(0), rank=0, world_size=1, reduce_critic=False, force_split=True)
    ragent = pkg.create_agent(setup=setup, B=2, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                              noise_seed=7, trajectory_length=1, reducer=red)
    with pytest.raises(pkg.PdecError, match=r"telemetry=8.*not available with an active reducer"):
        pkg.TrainPipeline(env, ragent, telemetry=8, **kw)
    pkg.TrainPipeline(env, ragent, telemetry=0, **kw).close()       # off: the reducer's pipeline as it always was
    red.close()
