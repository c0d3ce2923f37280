"""GPU tests of TrainPipeline's greedy held-out evaluation (eval_every): the device rows against a solo env.rollout of the
parameters the evaluated step's acting kernel read, restated in NumPy (pipeline_eval_ref.py); no side effects on the training
run; the best actor by evaluation score; the ring and the schedule; the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from pipeline_eval_ref import best_rule, restate_eval

pytestmark = pytest.mark.gpu

NETS = ("behavior_actor", "behavior_critic", "target_actor", "target_critic")


def _setup(pkg, geom, **kw):
    if geom == "ks22":
        return pkg.KSSetup.KS22(**kw)
    if geom == "c2":
        return pkg.KSSetup.bench_C2(256, **kw)
    if geom == "kseg":
        return pkg.KellerSegelSetup(**kw)
    if geom == "kseg2d":
        return pkg.KellerSegel2DSetup(nx=64, ny=64, **kw)
    raise ValueError(geom)


def _make(pkg, geom, B=64, E=17, dtype=torch.float32, graphs=False, setup_kw=None, third=False, **kw):
    setup = _setup(pkg, geom, **(setup_kw or {}))
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    y0 = None
    if geom in ("ks22", "c2"):                   # (the Keller-Segel setups: their standard field)
        y0 = setup.generate_random_init(np.random.default_rng(0), B) * 0.15
    env = pkg.PDEenv(setup, B=B, dtype=dtype, y0=y0, stream=s_env, autoreset=False)
    agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                             noise_seed=7, trajectory_length=1)
    agent.policy.act_noise = 0.3
    torch.cuda.synchronize()
    if third:
        kw["eval_stream"] = torch.cuda.Stream()
    return pkg.TrainPipeline(env, agent, lag=2, episode_steps=E, stream_env=s_env, stream_upd=s_upd, use_graphs=graphs,
                             chunks=(6, 1), noise_seed=99, **kw)


def _drained(p, n, before_last=None, after_last=None):
    """n eager steps, the device drained after each.  before_last(e) / after_last(e): called, the device idle, before / behind
    the last step of 0-based episode e"""
    p.drain_between = True
    for _ in range(n):
        k = p.tick
        last = (k - p.ep_start) % p.E == p.E - 1
        if last and before_last is not None:
            torch.cuda.synchronize()
            before_last((k - p.ep_start) // p.E)
        p.step()
        torch.cuda.synchronize()
        if last and after_last is not None:
            after_last((k - p.ep_start) // p.E)


def _solo(pkg, p, params):
    """a fresh B = K environment from p.eval_y0, one greedy episode of a clone of the actor holding `params` (None: all zero):
    the rollout's (reward_sum, done_step) on the host"""
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


ROW_CASES = {
    "ks22_f32_k5": dict(geom="ks22", K=5),
    "ks22_f64_env_f32_nets_k5": dict(geom="ks22", K=5, dtype=torch.float64),
    "c2_fused_k4": dict(geom="c2", K=4),
    "ks22_k1": dict(geom="ks22", K=1),
    "ks22_k300": dict(geom="ks22", K=300),
    "kseg_f64_k3": dict(geom="kseg", K=3, dtype=torch.float64, E=5, B=8),
    "kseg2d_f32_k3": dict(geom="kseg2d", K=3, E=5, B=8),
}


@pytest.mark.parametrize("case", sorted(ROW_CASES))
def test_rows_are_a_solo_rollout(pkg, case):
    c = dict(ROW_CASES[case])
    K, E, n_ep = c.pop("K"), c.pop("E", 17), 4
    p = _make(pkg, c.pop("geom"), E=E, log_episodes=8, eval_every=2, eval_inits=K, eval_seed=5, **c)
    assert tuple(p.eval_y0.shape) == (K,) + tuple(p.env._yshape[1:]) and p.eval_y0.dtype == p.env.dtype
    if case == "c2_fused_k4":
        assert not p.act_in_place                  # the snapshot is the unpacked published image
    read = {}
    _drained(p, n_ep * E, before_last=lambda e: read.__setitem__(e + 1, p.actor.params()))
    eps, ret, blew, dropped = p.eval_returns()
    scores = p.eval_scores
    assert dropped == 0 and eps.tolist() == [2, 4] and p.n_evals == 2
    assert ret.shape == (2, K) and blew.shape == (2, K) and scores.shape == (2,)
    for i, e in enumerate(eps):
        w_ret, w_blew, w_score = restate_eval(*_solo(pkg, p, read[int(e)]))
        print(case, "episode", int(e), "score", scores[i], "solo", w_score)
        assert np.array_equal(ret[i], w_ret, equal_nan=True)
        assert np.array_equal(blew[i], w_blew)
        assert np.array_equal(scores[i:i + 1], np.array([w_score]), equal_nan=True)
    zero = restate_eval(*_solo(pkg, p, None))[2]
    print(case, "zero action", p.eval_zero_score, "solo", zero)
    assert np.array_equal(np.array([p.eval_zero_score]), np.array([zero]), equal_nan=True)
    p.close()


def _adam(nna):
    m = nna.model
    k = m.num_params
    a, b, bp = (C.c_float * k)(), (C.c_float * k)(), (C.c_double * 2)()
    assert m.lib.pdec_adam_get_state(m.handle, a, b, bp) == 0
    return np.frombuffer(bytes(a), dtype=np.uint32), np.frombuffer(bytes(b), dtype=np.uint32), np.array([bp[0], bp[1]])


def _train_state(p):
    p.sync()
    ret, blew, _ = p.episode_returns()
    nets = {n: getattr(p.policy, n).model.params() for n in NETS}
    adam = {n: _adam(getattr(p.policy, n)) for n in ("behavior_actor", "behavior_critic")}
    return dict(ret=ret, blew=blew, rewards=np.array(p.rewards), best=(p.bestreward, p.bestepisode),
                best_params=p.best_actor().params(), nets=nets, adam=adam, y=p.y.cpu().numpy(), env_y=p.env.y.cpu().numpy())


@pytest.mark.parametrize("geom,graphs", [("c2", False), ("c2", True), ("ks22", False), ("ks22", True)])
def test_evaluation_has_no_side_effects(pkg, geom, graphs):
    E, n_ep = 17, 6
    states = []
    for kw in (dict(eval_every=0), dict(eval_every=1, eval_inits=4), dict(eval_every=1, eval_inits=4, third=True)):
        p = _make(pkg, geom, E=E, graphs=graphs, log_episodes=8, min_best_episode=2, **kw)
        if graphs:
            assert p.use_graphs
            p.run(5)
            p.capture()
            assert p._captured and p.graphs
        p.run(n_ep * E - p.tick)
        states.append(_train_state(p))
        assert p.n_episodes == n_ep and p.n_evals == (n_ep if kw["eval_every"] else 0)
        if kw["eval_every"]:
            assert p.eval_returns()[0].tolist() == list(range(1, n_ep + 1)) and np.isfinite(p.eval_scores).all()
            assert (p.s_eval.cuda_stream != p.s_env.cuda_stream) == bool(kw.get("third"))
        else:
            assert p.eval_env is None and p.eval_actor is None and p.s_eval is None      # nothing new is allocated
        p.close()
    a = states[0]
    for b in states[1:]:
        for key in ("ret", "blew", "rewards", "y", "env_y"):
            assert np.array_equal(a[key], b[key], equal_nan=True), key
        assert a["best"] == b["best"] and a["best"][1] >= 2
        for x, y in zip(a["best_params"], b["best_params"]):
            assert np.array_equal(x, y)
        for n in NETS:
            for x, y in zip(a["nets"][n], b["nets"][n]):
                assert np.array_equal(x, y), n
        for n in a["adam"]:
            for x, y in zip(a["adam"][n], b["adam"][n]):
                assert np.array_equal(x, y), n


@pytest.mark.parametrize("third", [False, True])
def test_best_actor_by_evaluation(pkg, third):
    E, n_ep, mbe = 13, 6, 3
    p = _make(pkg, "c2", E=E, log_episodes=8, min_best_episode=mbe, eval_every=1, eval_inits=4, best_by="eval", third=third)
    read = {}
    _drained(p, n_ep * E, before_last=lambda e: read.__setitem__(e + 1, p.actor.params()))
    eps, _, blew, _ = p.eval_returns()
    scores = p.eval_scores
    assert eps.tolist() == list(range(1, n_ep + 1)) and np.isfinite(scores).all() and not blew.any()
    best, best_e = best_rule(eps, scores, mbe)
    print("scores", scores.tolist(), "best", best, best_e)
    assert best_e >= mbe and p.bestepisode == best_e and p.bestreward == best
    got = p.best_actor()
    assert isinstance(got, pkg.nna.CustomNeuralNetworkApproximator) and got.model.dtype == p.actor.dtype
    for x, y in zip(got.params(), read[best_e]):
        assert np.array_equal(x, y)
    p.close()


def test_best_actor_by_evaluation_skips_stopped_evaluations(pkg):
    """max_value = 1 (the existing ledger test's way to make trajectories stop).  The actors of episodes 3 and 6 are replaced,
    for their last step, by one whose output bias saturates the action: at agent_power 7.5 the forcing carries the field past
    max_value within the episode, the evaluation's bits are raised and its score is NaN.  The other evaluations run the actor
    as training left it, on fields of amplitude 0.05 (some of those stop too; the host restatement decides which)."""
    E, n_ep, mbe, K = 7, 6, 3, 4
    setup = pkg.KSSetup.KS22(max_value=1.0)
    y0 = torch.as_tensor(setup.generate_random_init(np.random.default_rng(3), K) * 0.05, dtype=torch.float32)
    p = _make(pkg, "ks22", E=E, setup_kw=dict(max_value=1.0), log_episodes=8, min_best_episode=mbe, eval_every=1, eval_y0=y0,
              best_by="eval")
    assert torch.equal(p.eval_y0.cpu(), y0)
    read, kept = {}, {}

    def before_last(e):
        if e + 1 in (3, 6):
            kept[e] = p.actor.params()
            sat = [np.zeros_like(x) for x in kept[e]]
            sat[-1][:] = 50.0
            p.actor.set_params(sat)
        read[e + 1] = p.actor.params()

    def after_last(e):
        if e in kept:
            p.actor.set_params(kept.pop(e))

    _drained(p, n_ep * E, before_last=before_last, after_last=after_last)
    eps, ret, blew, _ = p.eval_returns()
    scores = p.eval_scores
    want = [restate_eval(*_solo(pkg, p, read[int(e)])) for e in eps]
    w_scores = np.array([w[2] for w in want])
    print("scores", scores.tolist(), "restated", w_scores.tolist())
    assert np.isnan(w_scores).any() and np.isfinite(w_scores).any()        # otherwise the case shows nothing
    assert np.array_equal(scores, w_scores, equal_nan=True)
    for i, w in enumerate(want):
        assert np.array_equal(ret[i], w[0], equal_nan=True) and np.array_equal(blew[i], w[1])
        if blew[i].any():
            assert np.isnan(scores[i])
    best, best_e = best_rule(eps, scores, mbe)
    assert p.bestepisode == best_e and p.bestreward == best and best_e >= mbe
    assert np.isfinite(scores[best_e - 1]) and not blew[best_e - 1].any()
    nan_eps = [int(e) for e, s in zip(eps, scores) if np.isnan(s)]
    assert best_e not in nan_eps and best_e > min(e for e in nan_eps if e >= mbe)      # a finite one behind a NaN is chosen
    for x, y in zip(p.best_actor().params(), read[best_e]):
        assert np.array_equal(x, y)
    p.close()


def test_ring_and_schedule(pkg):
    E = 13
    p = _make(pkg, "ks22", E=E, log_episodes=8, eval_every=3, eval_inits=2, eval_capacity=1)
    read = {}
    _drained(p, 7 * E, before_last=lambda e: read.__setitem__(e + 1, p.actor.params()))
    eps, ret, blew, dropped = p.eval_returns()
    assert p.n_episodes == 7 and p.n_evals == 2
    assert eps.tolist() == [6] and dropped == 1 and ret.shape == (1, 2) and p.eval_scores.shape == (1,)
    w_ret, w_blew, w_score = restate_eval(*_solo(pkg, p, read[6]))
    assert np.array_equal(ret[0], w_ret) and np.array_equal(blew[0], w_blew) and p.eval_scores[0] == w_score
    # a cut episode is neither logged nor evaluated; sync() drains the evaluation as well
    p.run(5)
    p.reset_from(p.env.y0)
    p.run(E)
    p.sync()
    assert p.n_episodes == 8 and p.n_evals == 2
    p.run(E)
    p.sync()
    assert p.n_episodes == 9 and p.n_evals == 3 and p.eval_returns()[0].tolist() == [9] and p.eval_returns()[3] == 2
    p.close()


def test_refusals(pkg):
    Err = pkg._lib.PdecError
    with pytest.raises(Err, match="log_episodes"):
        _make(pkg, "ks22", eval_every=2)
    with pytest.raises(Err, match="episode_steps"):
        _make(pkg, "ks22", E=0, log_episodes=4, eval_every=2)
    with pytest.raises(Err, match="eval_inits"):
        _make(pkg, "ks22", log_episodes=4, eval_every=2, eval_inits=0)
    with pytest.raises(Err, match="eval_capacity"):
        _make(pkg, "ks22", log_episodes=4, eval_every=2, eval_capacity=0)
    with pytest.raises(Err, match="eval_y0"):
        _make(pkg, "ks22", log_episodes=4, eval_every=2, eval_y0=torch.zeros(3, 191))
    with pytest.raises(Err, match="eval_y0"):
        _make(pkg, "ks22", log_episodes=4, eval_every=2, eval_y0=torch.zeros(192))
    with pytest.raises(Err, match="best_by"):
        _make(pkg, "ks22", log_episodes=4, best_by="eval")
    with pytest.raises(Err, match="best_by"):
        _make(pkg, "ks22", log_episodes=4, eval_every=2, best_by="evaluation")
    # eval_stream equal to the update stream
    setup = pkg.KSSetup.KS22()
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    env = pkg.PDEenv(setup, B=8, dtype=torch.float32, stream=s_env, autoreset=False)
    agent = pkg.create_agent(setup=setup, B=8, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                             noise_seed=7, trajectory_length=1)
    torch.cuda.synchronize()
    kw = dict(lag=2, episode_steps=13, stream_env=s_env, stream_upd=s_upd, use_graphs=False, log_episodes=4, eval_every=2)
    with pytest.raises(Err, match="eval_stream"):
        pkg.TrainPipeline(env, agent, eval_stream=s_upd, **kw)
    # an active reducer
    lib = pkg._lib.load()
    red = pkg.distributed.NativeGradReducer(lib, rank=0, world_size=1, reduce_critic=False, force_split=True)
    agent_r = pkg.create_agent(setup=setup, B=8, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                               noise_seed=7, trajectory_length=1, reducer=red)
    torch.cuda.synchronize()
    with pytest.raises(Err, match="reducer"):
        pkg.TrainPipeline(env, agent_r, **kw)
    # the accessors of a pipeline without evaluations
    q = _make(pkg, "ks22", log_episodes=2)
    with pytest.raises(Err, match="eval_every"):
        q.eval_returns()
    with pytest.raises(Err, match="eval_every"):
        q.eval_scores
