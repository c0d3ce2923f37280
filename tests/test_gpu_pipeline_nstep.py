"""GPU tests of TrainPipeline(n_step=...): KS22 geometry, fp32, episodes of E = 7.  The teacher-forced run of tests/pipeline_ref.py
with every assembled batch held exactly to tests/nstep_ref.py and every update judged by small_update_ref.check_launch on that
minibatch with gamma_n in the place of gamma; graphs against eager steps; the default path; per-trajectory episodes; the split
update of a one-rank reducer; refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from nstep_ref import NStepModel, first_update_steps, gamma_n, nstep_transition
from pipeline_ref import (KSEnv, _same_snap, check_act, check_env, config_of, episode_y0, ks_config, record_step,
                          run_teacher_forced, schedule)
from small_update_ref import check_launch

pytestmark = pytest.mark.gpu

N, E, LAG = 3, 7, 2
STEPS = 3 * E + 5
NAMES = ("state", "action", "reward", "terminal", "next_state")


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


def _keep_batches(pipe):
    """every assembled batch, read back behind the synchronisation that follows its step and before the next step is issued"""
    kept, sync = {}, pipe.sync

    def sync_and_keep():
        sync()
        k = pipe.tick - 1
        if k >= 0 and k not in kept:
            kept[k] = [x.detach().cpu().numpy().copy() for x in pipe.nstep_batch(k)]
    pipe.sync = sync_and_keep
    return kept


def _same_state(pkg, rec, pipe, k):
    got = record_step(pkg, pipe, k)
    assert _same_snap(rec.snap, got.snap)                                  # four networks, ADAM moments, beta powers
    assert np.array_equal(np.asarray(rec.snap.losses), np.asarray(got.snap.losses), equal_nan=True)
    assert rec.ctr == got.ctr                                              # the noise counter
    for name in ("y_in", "y_out", "s_in", "s_out", "a", "r", "t", "flags"):
        assert np.array_equal(getattr(rec, name), getattr(got, name)), name


def _check_trace(cfg, trace, n, batches):
    """pipeline_ref.check_trace with the update of step k judged on the n-step minibatch assembled at step k - LAG"""
    steps = len(trace.steps)
    sch = schedule(cfg, trace, steps)
    y0s = episode_y0(cfg, trace, steps)
    gn = gamma_n(cfg.gamma, n)
    errs, worst, updates = [], {}, []
    for k, rec in enumerate(trace.steps):
        first, last, first_tick, _start = sch[k]
        prev = trace.steps[k - 1] if k > 0 else trace.init
        if first:
            y_k = np.asarray(np.asarray(y0s[k], np.float64), dtype=rec.y_in.dtype).astype(np.float64)
            s_k = cfg.env.featurize(y_k)
            a_prev = np.zeros_like(rec.a)
            if not float(np.abs(rec.s_in - s_k).max()) <= cfg.env.tol["state"]:
                errs.append(f"act s_k (step {k}): the first state is not featurize(y0)")
        else:
            y_k, s_k, a_prev = prev.y_out.astype(np.float64), prev.s_out, prev.a
            if not np.array_equal(rec.s_in, s_k):
                errs.append(f"act s_k (step {k}): the acting kernel's state is not the s_(k+1) step {k - 1} left")
        errs += check_act(cfg, k, prev, rec, s_k, worst)
        errs += check_env(cfg, k, rec, y_k, s_k, a_prev, first, last, False, worst)[0]
        # the assembled batch of step k: exact (windows that start before step 0 are nobody's)
        if k >= n - 1:
            want = nstep_transition(trace, k, n, cfg.gamma)
            for name, g, w in zip(NAMES, batches[k], want):
                if not (g.dtype == w.dtype and np.array_equal(g.reshape(w.shape), w)):
                    errs.append(f"n-step batch (step {k}): {name} differs from the model")
        j = k - cfg.lag
        if j < first_tick + n - 1:
            if not _same_snap(prev.snap, rec.snap):
                errs.append(f"update (step {k}): the learner changed, but the window of transition {j} starts before the restart")
            continue
        updates.append(k)
        s, a, R, T, sn = nstep_transition(trace, j, n, cfg.gamma)
        e = check_launch(prev.snap, rec.snap, [(s.T, a.T, R, T, sn.T)], cfg.acts_a, cfg.acts_c, gn, cfg.rho, cfg.quirk, cfg.eta_a,
                         cfg.eta_c, group=cfg.group, kinks=cfg.kinks, worst=worst)
        errs += [f"update (step {k}, window {j - n + 1} .. {j}): {x}" for x in e]
    return errs, worst, updates


@pytest.mark.parametrize("B", [64, 3])
def test_teacher_forced_run(pkg, B):
    """3 E + 5 steps with a reset_from in mid-episode (tick 10): act_k and env_k as pipeline_ref checks them, every assembled batch
    exact, every update -- and its absence before F + n - 1 + LAG -- by check_launch at pipeline_ref's tolerances"""
    p = _make(pkg, B=B, n_step=N)
    assert p.n_step == N and p.gamma_n == gamma_n(p.policy.y, N) and p.rpart is None
    cfg = config_of(p, KSEnv(ks_config(p.env.setup), B))
    batches = _keep_batches(p)
    trace = run_teacher_forced(pkg, p, STEPS, {10: _reset_field(p, 3)})
    assert sorted(batches) == list(range(STEPS))
    errs, worst, updates = _check_trace(cfg, trace, N, batches)
    print(f"\n[n-step pipeline] B = {B}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))
    assert errs == [], errs[:10]
    assert updates == first_update_steps(trace.resets, STEPS, LAG, N) == list(range(4, 10)) + list(range(14, STEPS))
    assert np.allclose(trace.steps[-1].snap.bpA, trace.init.snap.bpA * np.array([0.9, 0.999]) ** len(updates), rtol=1e-12)
    # windows cut at the lock-stepped episode ends: the batches of the first n - 1 steps of an episode are terminal, full ones not
    for k in (7, 8, 17, 18, 24, 25):
        assert (batches[k][3] == 1).all(), k
    for k in (2, 5, 12, 15, 19, 22):
        assert (batches[k][3] == 0).all(), k
    # the same run without a synchronisation between the steps (recorded steps) ends in the same state
    q = _make(pkg, B=B, n_step=N)
    q.run(10)
    q.reset_from(_reset_field(q, 3))
    q.run(STEPS - 10)
    q.sync()
    assert q._progs
    _same_state(pkg, trace.steps[-1], q, STEPS - 1)
    for g, w in zip(q.nstep_batch(STEPS - 1), batches[STEPS - 1]):
        assert np.array_equal(g.cpu().numpy(), w)
    p.close()
    q.close()


@pytest.mark.parametrize("mode", ["per_trajectory_E7", "lockstep_E14"])
def test_graphs_equal_eager_steps(pkg, mode):
    """capture() needs lock-stepped episodes longer than two ring periods (E > 12), so the E = 7 run is captured with per-trajectory
    episodes -- the host then schedules one endless episode and every step of a chunk carries an update -- and the lock-stepped
    one with E = 14.  Networks, ADAM moments, losses, y, the rings, the assembled batches and the noise counter: bit-identical."""
    kw = dict(E=7, episodes="per_trajectory", stagger=True, log_episodes=8) if mode == "per_trajectory_E7" else dict(E=14)
    pg = _make(pkg, graphs=True, n_step=N, **kw)
    pe = _make(pkg, graphs=False, n_step=N, **kw)
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
    for k in (n - 3, n - 2, n - 1):
        for g, w in zip(pg.nstep_batch(k), pe.nstep_batch(k)):
            assert torch.equal(g, w), k
    pos = [C.c_int64(), C.c_int64()]
    for p, v in zip((pg, pe), pos):
        pkg._lib.check(p.lib.pdec_nstep_read(p.nstep.h, C.byref(v), None, None, None, None))
    assert pos[0].value == pos[1].value == n
    pg.close()
    pe.close()


def test_default_path_builds_nothing(pkg):
    pa = _make(pkg, n_step=1)
    pb = _make(pkg)
    for p in (pa, pb):
        assert p.nstep is None and p.nbatch is None and p.n_step == 1 and p.gamma_n == float(p.policy.y)
        with pytest.raises(pkg.PdecError, match="n_step = 1 assembles nothing"):
            p.nstep_batch(0)
        p.run(STEPS)
        p.sync()
    _same_state(pkg, record_step(pkg, pa, STEPS - 1), pb, STEPS - 1)
    assert len(pa._progs) == len(pb._progs) > 0
    for k in pa._progs:
        assert [f.__name__ for f, _ in pa._progs[k]] == [f.__name__ for f, _ in pb._progs[k]]
        assert not any("nstep" in f.__name__ for f, _ in pa._progs[k])
    pa.close()
    pb.close()


def test_per_trajectory_episodes(pkg):
    """B = 8, staggered clocks, max_value = 1.5 (rows 5 and 7 blow up after a step: tests/test_gpu_episode_clock.py): the model is
    fed the rows the device's rings hold behind the clock call -- sanitised rewards, the clock's terminal rows -- and every assembled
    batch equals it exactly; some window was cut by a restart, and the restarted trajectory's next window starts from its new state"""
    B = 8
    setup = pkg.KSSetup.KS22(max_value=1.5)
    y0 = setup.generate_random_init(np.random.default_rng(0), B) * (0.05 * (np.arange(B) % 8 + 1))[:, None]
    p = _make(pkg, B=B, y0=y0, setup_kw=dict(max_value=1.5), act_noise=0.1, episodes="per_trajectory", stagger=True,
              log_episodes=8, n_step=N)
    cols = p.cols
    mdl = NStepModel(N, float(p.policy.y))
    cut = restarted = 0
    before = [x.copy() for x in p.policy.behavior_critic.model.params()]
    for k in range(STEPS):
        p.run(1)
        p.sync()
        row = [t.detach().cpu().numpy().reshape(shape).copy() for t, shape in
               ((p.sring[k % 6], (cols, p.ns)), (p.aring[k % 3], (cols, p.na)), (p.rring[k % 3], (cols,)), (p.tring[k % 3], (cols,)))]
        want = mdl.push(*row)
        got = [x.detach().cpu().numpy() for x in p.nstep_batch(k)]
        assert np.array_equal(got[4], p.sring[(k + 1) % 6].cpu().numpy().reshape(cols, p.ns))
        if k < N - 1:
            continue
        for name, g in zip(NAMES[:4], got):
            assert np.array_equal(g, want[name]), (name, k)
        short = want["m"] < N - 1
        cut += int(short.sum())
        assert (want["terminal"][short] == 1).all()
        # a window whose first row follows a terminal row starts from the restart state the clock wrote
        u = k - N + 1
        if u >= 1:
            after = mdl.t[u - 1] != 0
            restarted += int(after.sum())
            assert np.array_equal(got[0][after], mdl.s[u][after])
    assert cut > 0 and restarted > 0
    fin = p.finished_episodes()
    assert (fin["length"] < 7).any() and fin["blew_up"].any()
    after = p.policy.behavior_critic.model.params()
    assert not all(np.array_equal(x, y) for x, y in zip(before, after)) and all(np.isfinite(x).all() for x in after)
    p.close()


def test_refusals_by_name(pkg):
    setup = pkg.KSSetup.KS22()
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    env = pkg.PDEenv(setup, B=2, dtype=torch.float32, stream=s_env, autoreset=False)
    agent = pkg.create_agent(setup=setup, B=2, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                             noise_seed=7, trajectory_length=8 * setup.n_actuators)
    kw = dict(lag=LAG, episode_steps=E, stream_env=s_env, stream_upd=s_upd, use_graphs=False)
    with pytest.raises(pkg.PdecError, match=r"n_step=3.*use_replay=True is not covered \(the replay route pushes one-step rows\)"):
        pkg.TrainPipeline(env, agent, use_replay=True, n_step=3, **kw)
    for bad in (0, 33, 2.5, "2"):
        with pytest.raises(pkg.PdecError, match=r"n_step=.*an integer from 1 to 32"):
            pkg.TrainPipeline(env, agent, n_step=bad, **kw)


@pytest.mark.parametrize("order", ["critic_exchanged", "on_chain", "off_chain", "off_chain_one_stream"])
def test_split_update_on_one_rank_equals_the_fused_finish(pkg, order):
    """a reducer: C2 geometry (the fused 3-layer family), B = 64, E = 17, n_step = 3.  The data-parallel launch sequence through a
    one-rank communicator -- whose all-reduce is the identity -- hands gamma_n to the critic half in each of its orders (critic
    gradients exchanged; policy gradient only with the collective on the update stream, on a side stream, and on a side stream with
    env and update on one stream) and leaves the networks and the field of the fused single-GPU n-step run, bit for bit."""
    def make(red=None, serial=False, **kw):
        setup = pkg.KSSetup.bench_C2(256)
        s_env = torch.cuda.Stream()
        s_upd = s_env if serial else torch.cuda.Stream()
        y0 = setup.generate_random_init(np.random.default_rng(0), 64) * 0.15
        env = pkg.PDEenv(setup, B=64, dtype=torch.float32, y0=y0, stream=s_env, autoreset=False)
        agent = pkg.create_agent(setup=setup, B=64, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                                 noise_seed=7, trajectory_length=1, **({} if red is None else dict(reducer=red)))
        agent.policy.act_noise = 0.3
        torch.cuda.synchronize()
        return pkg.TrainPipeline(env, agent, lag=LAG, episode_steps=17, stream_env=s_env, stream_upd=s_upd, use_graphs=False,
                                 noise_seed=99, n_step=N, **kw)

    red = pkg.distributed.NativeGradReducer(pkg._lib.init(0), rank=0, world_size=1, reduce_critic=(order == "critic_exchanged"),
                                            force_split=True)
    kw = {}
    if order != "critic_exchanged":
        kw = dict(stream_ar=torch.cuda.Stream(), ar_off_chain=order.startswith("off_chain"))
    pb = make(red, serial=(order == "off_chain_one_stream"), **kw)
    pf = make()
    assert pb.multi_rank and pb.ar_off_chain == order.startswith("off_chain") and not pf.multi_rank
    pf.run(40); pb.run(40)
    pf.sync(); pb.sync()
    assert torch.equal(pf.y, pb.y) and bool(torch.isfinite(pb.y).all())
    for name in ("behavior_actor", "behavior_critic", "target_actor", "target_critic"):
        for x, y in zip(getattr(pf.policy, name).model.params(), getattr(pb.policy, name).model.params()):
            assert np.array_equal(x, y), name
    for g, w in zip(pb.nstep_batch(39), pf.nstep_batch(39)):
        assert torch.equal(g, w)
    pb.close(); pf.close()
    red.close()
