"""TrainPipeline on a 2-D fluid environment (the environment's dtype = the networks').

Teacher-forced against tests/pipeline_fluid_ref.py (FluidEnvRef in tests/pipeline_ref.py's check_trace): every step of a 20-step
run over two episode boundaries (E = 7), then the same run issued without per-step synchronisation and with use_graphs=True
requested, which must end bit-identical with pipe.use_graphs False.  Also: the rank split of the device draw, the episode ledger
and best actor, the greedy evaluation, a batch stepped in parts (child process), the mixed-dtype refusal.

Grids: tests/fluid_ic_ref.py::pair -- FluidSetup(nx = 64 | 32, oversampling 2, dt = 2 / (16 nx), variance 0.08).  Fields: ic(3) by
the device draw's rule from the host table, rounded to fp32.

The case `reset_blowup` (reset_from at tick 10, max_value 0.5, trajectory 2 multiplied by 10): the issue's factor, 30, holds for
one step only -- on the CPU oracle that trajectory gives max |reward| 2.9 - 3.0 at its first step, 5e5 (n = 64) at its second and
NaN from its third on, which the fp32 device cannot follow and which turns the learner into NaN two updates later, so nothing
behind it could be judged (the one-step tests of tests/test_gpu_fluid_terminal_rows.py keep x 30).  x 10 of the same field gives,
on the oracle under N(0, 0.3^2) actions, max |reward| 0.92 .. 0.99 over the eight steps an episode can take against <= 0.096 of the
other trajectories: past max_value = 0.5 by a factor 1.8, under it by a factor 5, finite.  All 20 steps go to check_trace -- the
updates from step 12 on train on transitions whose terminal rows are 1 for one trajectory only --, and from step 10 on flags and
terminal rows are exactly that trajectory's at every step but an episode's last, where all rows are 1."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from fluid_ic_ref import fields_of, mem, pair, vortex_table
from pipeline_fluid_ref import FluidEnvRef, fluid_config
from pipeline_ref import check_trace, config_of, n_updates, record_step, run_teacher_forced

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F32, F64 = torch.float32, torch.float64
N, E = 20, 7          # steps 0-6, 7-13, 14-19: two episode boundaries
NETS = ("behavior_actor", "behavior_critic", "target_actor", "target_critic")


def _fields(cfg, B, seed=21, scaled=None, factor=30.0):
    y = mem(fields_of(cfg, vortex_table(seed, 0, B, 3, cfg.Lx)))
    if scaled is not None:
        y[scaled] *= factor
    return y.astype(np.float32).astype(np.float64)


def _make(pkg, n=64, spa=4, B=6, dt=F32, lag=2, serial=False, E=E, use_graphs=False, setup_kw=None, streams=None, scaled=None,
          factor=30.0, part_streams=None, **kw):
    setup, _ = pair(pkg, n, spa, **(setup_kw or {}))
    if streams is None:
        s_env = torch.cuda.Stream()
        streams = (s_env, s_env if serial else torch.cuda.Stream())
    s_env, s_upd = streams[:2]
    y0 = _fields(fluid_config(setup), B, scaled=scaled, factor=factor)
    env = pkg.PDEenv(setup, B=B, dtype=dt, y0=torch.as_tensor(y0, dtype=dt, device="cuda:0"), stream=s_env, autoreset=False,
                     part_streams=part_streams)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(1), dtype=dt, stream=s_upd, start_steps=-1,
                                 noise_seed=7, trajectory_length=1)
    agent.policy.act_noise = 0.3
    torch.cuda.synchronize()
    return pkg.TrainPipeline(env, agent, lag=lag, episode_steps=E, stream_env=s_env, stream_upd=s_upd, use_graphs=use_graphs,
                             chunks=(6, 1), noise_seed=99, **kw)


def _env_ref(p):
    return FluidEnvRef(fluid_config(p.env.setup), p.env.B, fp64=p.env.dtype == F64)


def _same_as(pkg, rec, pipe, k):
    """bit-identical (every case is finite: asserted on the checked run)"""
    got = record_step(pkg, pipe, k)
    a, b = rec.snap, got.snap
    for name in ("A", "C", "At", "Ct", "mA", "vA", "mC", "vC"):
        for x, y in zip(getattr(a, name), getattr(b, name)):
            assert np.array_equal(x, y), name
    assert np.array_equal(a.bpA, b.bpA) and np.array_equal(a.bpC, b.bpC)
    assert rec.ctr == got.ctr
    for name in ("y_out", "s_out", "a", "r", "t", "flags"):
        assert np.array_equal(getattr(rec, name), getattr(got, name)), name


def _report(case, worst):
    print(f"\n[fluid pipeline reference] {case}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))


BLOWN = 2
CASES = {
    "default": dict(),                                        # n = 64, 4 sensors per axis, B = 6: 96 columns, two streams, lag 2
    "wide": dict(spa=8, B=4),                                 # 256 columns: the width from which the 2-layer acting kernel serves
    "lag1": dict(lag=1),
    "serial": dict(serial=True),
    "n32": dict(n=32),
    "f64": dict(dt=F64),
    "random_init": dict(random_init=True, init_seed=5, log_episodes=4),
    "reset_blowup": dict(setup_kw=dict(max_value=0.5), _reset=10),
}


def _reset_field(p, spec):
    if spec is None:
        return {}
    y = _fields(fluid_config(p.env.setup), p.env.B, seed=33, scaled=BLOWN, factor=10.0)
    out = {spec: torch.as_tensor(y, dtype=p.env.dtype, device="cuda:0")}
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_pipeline_step_matches_the_reference(pkg, case):
    kw = dict(CASES[case])
    reset = kw.pop("_reset", None)
    p = _make(pkg, **kw)
    assert p.use_graphs is False and p.env.is_fluid and p.env.dtype == p.actor.dtype
    assert p.rpart is None and p.pre_rbar == (p.env.dtype == F32)         # no reward partials for the fluid: pdec_reward_mean
    if case == "serial":
        assert p.serial
    if case == "wide":
        assert p.cols == 256
    cfg = config_of(p, _env_ref(p))
    trace = run_teacher_forced(pkg, p, N, _reset_field(p, reset))
    errs, worst = check_trace(cfg, trace)
    _report(case, worst)
    assert errs == [], errs[:10]
    if case == "random_init":
        per = p.env.B * 30
        assert cfg.random_init == (5, per) and p.init_offsets == [0, per, 2 * per]
    nu = n_updates(cfg, trace, N)
    assert nu == (N - cfg.lag if reset is None else N - 2 * cfg.lag)      # (a restart cuts off the lag transitions before it)
    assert np.allclose(trace.steps[-1].snap.bpA, trace.init.snap.bpA * np.array([0.9, 0.999]) ** nu, rtol=1e-12)
    assert all(np.isfinite(x).all() for st in trace.steps for x in st.snap.A + st.snap.C + [st.y_out, st.r])
    if reset is not None:
        A, B = p.env.setup.n_actuators, p.env.B
        one = np.zeros(B, dtype=bool)
        one[BLOWN] = True
        for k in range(reset, N):
            st = trace.steps[k]
            last = (k - reset) % E == E - 1
            rows = st.t.reshape(B, A)
            assert np.array_equal(st.flags != 0, one), (k, st.flags)
            if last:
                assert bool((rows == 1).all()), k
            else:
                assert np.array_equal(rows, np.repeat(one.astype(rows.dtype), A).reshape(B, A)), k
        for k in range(reset):
            assert not trace.steps[k].flags.any(), k
    # the same run as it is timed: no per-step synchronisation, graphs requested (and resolved away)
    q = _make(pkg, **dict(kw, use_graphs=True))
    assert q.use_graphs is False
    if reset is not None:
        q.run(reset)
        q.reset_from(_reset_field(q, reset)[reset])
    else:
        q.run(4)
        q.capture()                                   # returns: nothing to capture
        assert not q._captured and not q.graphs
    q.run(N - q.tick)
    q.sync()
    assert q.n_graph_launches == 0
    _same_as(pkg, trace.steps[-1], q, N - 1)
    p.close()
    q.close()


def test_ranks_share_one_draw(pkg):
    """the fluid twin of tests/test_gpu_pipeline_episodes.py::test_ranks_share_one_draw"""
    kw = dict(n=32, E=3, random_init=True, init_seed=3)
    one = _make(pkg, B=4, **kw)
    half = [_make(pkg, B=2, init_rank=(r, 2), **kw) for r in range(2)]
    for p in [one] + half:
        p.drain_between = True
    for e in range(3):
        fields = []
        for p in [one] + half:
            k = p.tick
            p.step()
            torch.cuda.synchronize()
            fields.append(p.ybuf[k % 2].clone())
            p.run(2)
            p.sync()
        assert torch.equal(fields[0], torch.cat(fields[1:])) and bool(torch.isfinite(fields[0]).all())
    assert one.init_offsets == [0, 120, 240] and half[1].init_offsets == [60, 180, 300]


def _restate(rews, flags, E):
    """the ledger's rule in NumPy (tests/test_gpu_pipeline_episodes.py::_restate)"""
    rets, blews, means = [], [], []
    for e in range(len(rews) // E):
        ret = np.zeros(rews[0].shape[0])
        blew = np.zeros(rews[0].shape[0], dtype=bool)
        for k in range(e * E, (e + 1) * E):
            r = rews[k].astype(np.float64)
            s = np.zeros(r.shape[0])
            for a in range(r.shape[1]):
                s = s + r[:, a]
            ret = ret + s / r.shape[1]
            blew |= flags[k] != 0
        t = 0.0
        for v in ret:
            t += v
        rets.append(ret)
        blews.append(blew)
        means.append(t / ret.shape[0])
    return np.array(rets), np.array(blews), means


def _drained(p, n, before_last=None):
    p.drain_between = True
    rews, flags = [], []
    for _ in range(n):
        k = p.tick
        if before_last is not None and (k - p.ep_start) % p.E == p.E - 1:
            torch.cuda.synchronize()
            before_last((k - p.ep_start) // p.E)
        p.step()
        torch.cuda.synchronize()
        rews.append(p.rring[k % 3].cpu().numpy())
        flags.append(p.fring[k % 3].cpu().numpy())
    return rews, flags


def test_ledger_and_best_actor(pkg):
    """trajectory 2 is multiplied by 10: past max_value = 0.5 at every step (oracle: max |reward| 1.1 .. 0.8 over an episode
    against <= 0.14 of the others) and finite, so the episodes' means are finite; a last episode from a NaN field is not"""
    mbe = 2
    p = _make(pkg, setup_kw=dict(max_value=0.5), scaled=BLOWN, factor=10.0, log_episodes=8, min_best_episode=mbe)
    clones = []
    rews, flags = _drained(p, 3 * E, before_last=lambda e: clones.append(p.actor.params()))
    y0 = p.env.y0.clone()
    y0[0] = float("nan")
    p.reset_from(y0)
    r2, f2 = _drained(p, E, before_last=lambda e: clones.append(p.actor.params()))
    ret, blew, means = _restate(rews + r2, flags + f2, E)
    g_ret, g_blew, dropped = p.episode_returns()
    assert dropped == 0 and g_ret.shape == (4, p.env.B)
    assert np.array_equal(g_ret, ret, equal_nan=True) and np.array_equal(g_blew, blew)
    assert np.array_equal(np.array(p.rewards), np.array(means), equal_nan=True)
    assert np.isfinite(means[:3]).all() and np.isnan(means[3])
    want = np.zeros(p.env.B, dtype=bool)
    want[BLOWN] = True
    for e in range(3):
        assert np.array_equal(g_blew[e], want), (e, g_blew[e])
    best, best_e, seen = -1e6, 0, []
    for e, m in enumerate(means):
        if e + 1 >= mbe and not np.isnan(m):
            seen.append(m)
            if m >= max(seen):
                best, best_e = m, e + 1
    assert best_e in (2, 3) and p.bestepisode == best_e and p.bestreward == best
    for x, y in zip(p.best_actor().params(), clones[best_e - 1]):
        assert np.array_equal(x, y)
    p.close()


def _solo(pkg, p, params):
    env, m = p.env, p.actor
    s = torch.cuda.Stream()
    K = int(p.eval_y0.shape[0])
    with torch.cuda.stream(s):
        fresh = pkg.PDEenv(env.setup, B=K, dtype=env.dtype, y0=p.eval_y0, stream=s, autoreset=False)
        clone = pkg.nna.HipMLP(m.dims, m.acts, params, env.dtype, m.device, m.max_cols, s)
        out = fresh.rollout(clone, p.E, act_limit=p.policy.act_limit, learning=False)
    s.synchronize()
    res = out["reward_sum"].cpu().numpy(), out["done_step"].cpu().numpy()
    fresh.close()
    return res


def _train_bits(p):
    p.sync()
    ret, blew, _ = p.episode_returns()
    nets = [x for n in NETS for x in getattr(p.policy, n).model.params()]
    return [ret, blew.astype(np.int8), np.array(p.rewards), p.y.cpu().numpy()] + nets + [r.cpu().numpy() for r in p.rring + p.tring]


def test_evaluation_rows_scores_and_no_side_effects(pkg):
    """eval_every = 1, 3 held-out fields, on the env stream and on a third stream of one make_streams call"""
    from pipeline_eval_ref import best_rule
    n_ep, K = 3, 3
    plain = _make(pkg, log_episodes=8)
    plain.run(n_ep * E)
    ref_bits = _train_bits(plain)
    plain.close()
    for third in (False, True):
        streams = tuple(pkg.make_streams((-1, 0, 0))) if third else None
        kw = dict(eval_stream=streams[2]) if third else {}
        p = _make(pkg, streams=streams, log_episodes=8, min_best_episode=1, eval_every=1, eval_inits=K, eval_seed=5,
                  best_by="eval", **kw)
        assert (p.s_eval.cuda_stream != p.s_env.cuda_stream) == third
        # the held-out fields: what evaluate_actors draws -- random_init_device with default_rng(eval_seed)
        ee = pkg.PDEenv(p.env.setup, B=K, dtype=p.env.dtype, autoreset=False)
        assert torch.equal(p.eval_y0, p.env.setup.random_init_device(ee, np.random.default_rng(5)))
        read = {}
        p.drain_between = True
        for _ in range(n_ep * E):
            k = p.tick
            if (k - p.ep_start) % E == E - 1:
                torch.cuda.synchronize()
                read[(k - p.ep_start) // E + 1] = p.actor.params()
            p.step()
            torch.cuda.synchronize()
        eps, ret, blew, dropped = p.eval_returns()
        scores = p.eval_scores
        assert dropped == 0 and eps.tolist() == [1, 2, 3]
        for i, e in enumerate(eps):
            w_ret, w_blew, w_score = pkg.pipeline.eval_score(*_solo(pkg, p, read[int(e)]))
            print("third" if third else "env stream", "episode", int(e), "score", scores[i], "solo", w_score)
            assert np.array_equal(ret[i], w_ret, equal_nan=True) and np.array_equal(blew[i], w_blew)
            assert np.array_equal(scores[i:i + 1], np.array([w_score]), equal_nan=True)
        zero = pkg.pipeline.eval_score(*_solo(pkg, p, None))[2]
        assert np.array_equal(np.array([p.eval_zero_score]), np.array([zero]), equal_nan=True) and np.isfinite(zero)
        best, best_e = best_rule(eps, scores, 1)
        assert best_e >= 1 and p.bestepisode == best_e and p.bestreward == best
        for x, y in zip(p.best_actor().params(), read[best_e]):
            assert np.array_equal(x, y)
        for a, b in zip(ref_bits, _train_bits(p)):
            assert np.array_equal(a, b, equal_nan=True)
        p.close()


def final_state(p):
    """what a run leaves, as host arrays (the split-batch child writes these, the parent compares)"""
    p.sync()
    out = {f"net{i}": x for i, x in enumerate(x for n in NETS for x in getattr(p.policy, n).model.params())}
    out.update(y=p.y.cpu().numpy(), state=p.state.cpu().numpy())
    for i in range(3):
        out.update({f"a{i}": p.aring[i].cpu().numpy(), f"r{i}": p.rring[i].cpu().numpy(), f"t{i}": p.tring[i].cpu().numpy(),
                    f"f{i}": p.fring[i].cpu().numpy()})
    return out


def split_run(pkg, part_streams=None, streams=None):
    """twelve steps over one episode boundary at B = 5 (parts of 2 + 3) with a flagged trajectory, unsynchronised"""
    p = _make(pkg, B=5, setup_kw=dict(max_value=0.5), scaled=BLOWN, factor=10.0, streams=streams, part_streams=part_streams,
              log_episodes=2)
    p.run(12)
    return p


def test_split_batch_ends_where_the_unsplit_run_does(pkg, tmp_path):
    p = split_run(pkg)
    assert p.env.n_part_streams == 0
    want = final_state(p)
    assert want["f2"].tolist() == [0, 0, 1, 0, 0]           # (step 11: the scaled trajectory, and only it, is flagged)
    p.close()
    here = os.path.dirname(os.path.abspath(__file__))
    out = str(tmp_path / "split.npz")
    r = subprocess.run([sys.executable, os.path.join(here, "pipeline_fluid_child.py"), out], env=dict(os.environ, PDEC_FLUID_SPLIT="2"),
                       capture_output=True, text=True, timeout=120, cwd=os.path.dirname(here))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "part streams 1" in r.stdout
    got = np.load(out)
    assert sorted(got.files) == sorted(want)
    for k, v in want.items():
        assert got[k].tobytes() == v.tobytes(), k


def test_mixed_dtypes_are_refused_by_name(pkg):
    """fp64 environment, Float32 networks (the C5 shape): the acting kernel reads the state ring in the actor's type.  The
    object may be constructed (tests/test_gpu_pipeline_episodes.py::test_random_inits_fluid asks one for its draw); the first
    run() / capture() refuses"""
    setup, _ = pair(pkg, 32)
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    env = pkg.PDEenv(setup, B=2, dtype=F64, stream=s_env, autoreset=False)
    agent = pkg.create_agent(setup=setup, B=2, rng=np.random.default_rng(1), dtype=F32, stream=s_upd, start_steps=-1, noise_seed=7,
                             trajectory_length=1)
    torch.cuda.synchronize()
    p = pkg.TrainPipeline(env, agent, episode_steps=E, stream_env=s_env, stream_upd=s_upd)
    for call in (lambda: p.run(1), p.step, p.capture):
        with pytest.raises(pkg.PdecError, match=r"fluid environment \(torch\.float64\) and the networks \(torch\.float32\)"):
            call()
    assert p.tick == 0
    # other kinds are untouched: an fp64 KS environment with Float32 networks steps
    ks = pkg.KSSetup.KS22()
    kenv = pkg.PDEenv(ks, B=4, dtype=F64, stream=s_env, autoreset=False)
    kag = pkg.create_agent(setup=ks, B=4, rng=np.random.default_rng(1), dtype=F32, stream=s_upd, start_steps=-1, noise_seed=7,
                           trajectory_length=1)
    q = pkg.TrainPipeline(kenv, kag, episode_steps=E, stream_env=s_env, stream_upd=s_upd, use_graphs=False)
    q.run(3)
    q.sync()
    assert q.tick == 3
