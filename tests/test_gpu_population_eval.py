"""Selection after population training (population.py: evaluate_actors, Population.evaluate; include/pdeconv.h:
pdec_rollout_members): M actors scored on the same held-out initial fields in ONE persistent launch.  Every member's rows
must be bit for bit those of its solo rollout, follow the fp64 oracle's closed loop, and the call must leave training alone."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

M, K = 6, 4


def _actors(pkg, setup, n=M, stream=None):
    """distinct random fp32 actors as the members of a population have them; the agents are returned to keep them alive"""
    agents = [pkg.create_agent(setup=setup, B=1, rng=np.random.default_rng(100 + m), stream=stream) for m in range(n)]
    return agents, [a.policy.behavior_actor for a in agents]


def _bits(t):
    t = t.contiguous()
    return t.view({8: torch.int64, 4: torch.int32}[t.element_size()])


def _same(a, b):
    """torch.equal on the bit patterns (NaN-safe, and -0.0 != 0.0)"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _solo(pkg, setup, actor, y0, T, dtype):
    env = pkg.PDEenv(setup, B=y0.shape[0], dtype=dtype, y0=y0, autoreset=False)
    out = env.rollout(actor.model.clone(dtype=env.dtype, max_cols=y0.shape[0] * setup.state_shape[1]), T, learning=False, log=True)
    torch.cuda.synchronize()
    return out


def _assert_members_equal_solo(pkg, setup, nnas, y0, res, dtype):
    T = res["y"].shape[0]
    for m, nna in enumerate(nnas):
        solo = _solo(pkg, setup, nna, y0, T, dtype)
        for k in ("y", "p", "action", "reward"):
            assert _same(res[k][:, m], solo[k]), (m, k)
        assert _same(res["reward_sum"][m], solo["reward_sum"]), m
        assert torch.equal(res["done_step"][m], solo["done_step"]), m
        assert _same(res["episode_reward"][m], solo["reward_sum"].mean(dim=1)), m


@pytest.mark.parametrize("which", ["ks22_fp64", "ks22_fp32_env", "keller_segel_fp64", "ks22_fp64_odd"])
def test_every_member_equals_its_solo_rollout(pkg, monkeypatch, which):
    """bit identity per member: the [T, m] rows of y / p / action / reward, reward_sum and done_step of the one launch
    against PDEenv(B = K).rollout(actor.clone(dtype = env.dtype)) on the persistent solo launch (K = 3: the odd pair)"""
    monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", "1")
    setup = pkg.KellerSegelSetup() if which.startswith("keller") else pkg.KSSetup.KS22()
    dtype = torch.float32 if "fp32" in which else torch.float64
    k = 3 if which.endswith("odd") else K
    agents, nnas = _actors(pkg, setup)
    draw = pkg.PDEenv(setup, B=k, dtype=dtype, autoreset=False)
    y0 = torch.empty_like(draw.y)
    draw.random_init(7, 0, out=y0)
    torch.cuda.synchronize()
    res = pkg.evaluate_actors(setup, nnas, y0=y0, dtype=dtype, log=True)
    assert res["one_launch"] is True
    assert res["y"].shape[:3] == (int(round(setup.te / setup.dt)) + 1, M, k)
    assert res["workgroups"] == (M * k if which.startswith("keller") else M * ((k + 1) // 2))
    _assert_members_equal_solo(pkg, setup, nnas, y0, res, dtype)
    # the members differ: a table that handed every workgroup member 0's actor would not pass unnoticed
    assert not _same(res["action"][:, 0], res["action"][:, 1])


def _oracle_loops(pkg, setup, nnas, y0):
    """oracle.ks + oracle.nn closed loops of every (member, init) pair, as test_rollout_follows_the_oracle_closed_loop builds
    them: rows[m][k] = list over steps of (action, y, p, reward), ret[m][k] = the return, ymax = max |y| over everything"""
    from oracle import ks, nn
    cfg = ks.KSConfig(192, 22.0, np.arange(1, 193, 24), sigma_sensors=0.7, sigma_actuators=0.7)
    T = int(round(setup.te / setup.dt)) + 1
    rows, ret, ymax = [], np.zeros((len(nnas), y0.shape[0])), 0.0
    for m, nna in enumerate(nnas):
        P = [p.astype(np.float64) for p in nna.model.params()]
        rows.append([])
        for k in range(y0.shape[0]):
            y, a_prev, r_sum, steps = y0[k].copy(), np.zeros((1, 8)), 0.0, []
            for _ in range(T):
                a = np.clip(nn.forward(P, [nn.RELU, nn.TANH], ks.featurize(cfg, y)), -1, 1)
                o = ks.env_step(cfg, y, a_prev, a, 0.0)
                y, a_prev = o["y"], a
                r_sum += o["reward"].mean()
                ymax = max(ymax, float(np.abs(y).max()))
                steps.append((a[0], y, o["p"], o["reward"]))
            rows[m].append(steps)
            ret[m, k] = r_sum
    return T, rows, ret, ymax


def _oracle_inits():
    from oracle import ks
    cfg = ks.KSConfig(192, 22.0, np.arange(1, 193, 24), sigma_sensors=0.7, sigma_actuators=0.7)
    rng = np.random.default_rng(2024)
    return np.stack([ks.generate_random_init(cfg, rng) for _ in range(K)])


def test_members_follow_the_oracle_closed_loop_and_rank_as_it_ranks(pkg, monkeypatch):
    """KS22 fp64, 6 members x 4 initial fields, 51 steps, against oracle.ks + oracle.nn directly with the tolerances of
    test_rollout_follows_the_oracle_closed_loop (actions, p, rewards 1e-9; y and the return 1e-8), no (member, init) pair left
    out; no blow-up on either side; `order` is the oracle's ordering of the member mean returns"""
    monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", "1")
    setup = pkg.KSSetup.KS22()
    agents, nnas = _actors(pkg, setup)
    y0 = _oracle_inits()
    T, rows, ret, ymax = _oracle_loops(pkg, setup, nnas, y0)
    assert ymax < setup.max_value, ymax                   # (the oracle's own fields stay inside the blow-up bound)
    res = pkg.evaluate_actors(setup, nnas, y0=torch.as_tensor(y0), log=True)
    assert res["one_launch"] is True and T == 51 and res["y"].shape[0] == T
    assert bool((res["done_step"] == -1).all())
    out = {k: res[k].cpu().numpy() for k in ("y", "p", "action", "reward", "reward_sum", "episode_reward")}
    worst = dict(action=0.0, y=0.0, p=0.0, reward=0.0, ret=0.0)
    for m in range(M):
        for k in range(K):
            for t, (a, y, p, r) in enumerate(rows[m][k]):
                worst["action"] = max(worst["action"], np.abs(out["action"][t, m, k, :, 0] - a).max())
                worst["y"] = max(worst["y"], np.abs(out["y"][t, m, k] - y).max())
                worst["p"] = max(worst["p"], np.abs(out["p"][t, m, k] - p).max())
                worst["reward"] = max(worst["reward"], np.abs(out["reward"][t, m, k] - r).max())
            worst["ret"] = max(worst["ret"], abs(out["reward_sum"][m, k].mean() - ret[m, k]),
                               abs(out["episode_reward"][m, k] - ret[m, k]))
    print("worst deviations from the oracle:", worst, "oracle max|y|:", ymax)
    assert worst["action"] <= 1e-9 and worst["p"] <= 1e-9 and worst["reward"] <= 1e-9, worst
    assert worst["y"] <= 1e-8 and worst["ret"] <= 1e-8, worst
    # ranking: the oracle's member means are apart by far more than the tolerance of a return, so its order is THE order
    means = ret.mean(axis=1)
    gaps = np.diff(np.sort(means))
    print("oracle member mean returns:", means, "smallest gap:", gaps.min())
    assert gaps.min() > 1e-6, gaps
    assert res["order"] == [int(i) for i in np.argsort(-means, kind="stable")]
    assert np.abs(res["score"] - means).max() <= 1e-8


def test_blown_up_members_score_nan_and_come_last(pkg, monkeypatch):
    monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", "1")
    setup = pkg.KSSetup.KS22()
    agents, nnas = _actors(pkg, setup)
    y0 = torch.as_tensor(_oracle_inits())
    ok = pkg.evaluate_actors(setup, nnas, y0=y0)
    assert ok["one_launch"] and not np.isnan(ok["score"]).any() and bool((ok["done_step"] == -1).all())
    # an initial field past max_value: flagged at step 0 for EVERY member (they share the fields), as the rollout test of
    # tests/test_gpu_agent.py does it.  Field 0 shares a complex FFT with field 1 in every member's block, as in a solo
    # B = 4 rollout, so the overflow reaches it too; the other pair's trajectories are untouched, bit for bit
    y_bad = y0.clone()
    y_bad[1, 5] = 1e3
    bad = pkg.evaluate_actors(setup, nnas, y0=y_bad)
    assert bad["one_launch"]
    assert bool((bad["done_step"][:, 1] == 0).all()) and bool((bad["done_step"][:, [2, 3]] == -1).all())
    assert _same(bad["reward_sum"][:, [2, 3]], ok["reward_sum"][:, [2, 3]])
    assert np.isnan(bad["score"]).all() and bad["order"] == list(range(M))
    # member 2's actor overwritten so that its block leaves the bound.  (The actor ends in tanh and the action is clamped, so
    # no FINITE weights, however large, push a KS22 field past max_value within an episode: the overwritten output layer is
    # huge AND its bias is not finite, which makes the member's first action, and with it its fields, NaN.)
    P = nnas[2].model.params()
    nnas[2].model.set_params([P[0], P[1], np.full_like(P[2], 3e38), np.full_like(P[3], np.nan)])
    hot = pkg.evaluate_actors(setup, nnas, y0=y0)
    assert hot["one_launch"]
    assert bool((hot["done_step"][2] == 0).all()) and np.isnan(hot["score"][2]) and hot["order"][-1] == 2
    keep = [0, 1, 3, 4, 5]
    assert np.array_equal(hot["score"][keep], ok["score"][keep]) and hot["order"][:-1] == [m for m in ok["order"] if m != 2]


@pytest.mark.parametrize("which", ["persistent_off", "ks22_global"])
def test_fallback_gives_the_members_solo_rollouts(pkg, monkeypatch, which):
    """where the library does not serve the one launch -- PDEC_ROLLOUT_PERSISTENT=0, the global agent -- the call loops over
    env.rollout: one_launch is False and the results are the per-member rollouts"""
    if which == "persistent_off":
        monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", "0")
        setup = pkg.KSSetup.KS22()
    else:
        monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", "1")
        setup = pkg.KSSetup.KS22_global()
    agents, nnas = _actors(pkg, setup, n=3)
    draw = pkg.PDEenv(setup, B=K, dtype=torch.float64, autoreset=False)
    y0 = torch.empty_like(draw.y)
    draw.random_init(11, 0, out=y0)
    torch.cuda.synchronize()
    res = pkg.evaluate_actors(setup, nnas, y0=y0, log=True)
    assert res["one_launch"] is False and res["workgroups"] is None
    _assert_members_equal_solo(pkg, setup, nnas, y0, res, torch.float64)
    # the default fields: n_inits draws from (init_seed, 0), shared by all members
    res2 = pkg.evaluate_actors(setup, nnas, n_inits=K, init_seed=11, log=True)
    for k in ("y", "reward_sum", "done_step"):
        assert _same(res2[k], res[k]), k


def _beta_powers(nna):
    bp = (C.c_double * 2)()
    assert nna.model.lib.pdec_adam_get_state(nna.model.handle, None, None, bp) == 0
    return np.array([bp[0], bp[1]])


def _train(pkg, evaluate):
    setup = pkg.KSSetup.KS22()
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    members = []
    for seed in (3, 11, 29):
        agent = pkg.create_agent(setup=setup, B=1, rng=np.random.default_rng(seed), noise_seed=seed, stream=s_upd)
        agent.policy.act_noise = setup.act_noise
        members.append((agent, pkg.PDEhook(min_best_episode=1, use_random_init=True, init_seed=seed)))
    pop = pkg.Population(setup, [a for a, _ in members], [h for _, h in members], stream_env=s_env, dtype=torch.float64)
    evals = []
    pop.run([pkg.StopAfterEpisode(1) for _ in members])
    if evaluate:
        evals = [pop.evaluate(), pop.evaluate(which="best", n_inits=3, init_seed=5)]
    pop.run([pkg.StopAfterEpisode(1) for _ in members])
    torch.cuda.synchronize()
    return pop, evals


def test_evaluation_leaves_training_alone(pkg, monkeypatch):
    """two identical populations (KS22, M = 3, 2 episodes); one evaluates its current and its best actors between the
    episodes: the four networks, ADAM state, trajectory counters and traces and hook.rewards of every member end identical"""
    monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", "1")
    pa, _ = _train(pkg, False)
    pb, evals = _train(pkg, True)
    assert all(e["one_launch"] for e in evals) and evals[0]["episode_reward"].shape == (3, 8) and evals[1]["done_step"].shape == (3, 3)
    for m in range(3):
        aa, ab, ha, hb = pa.agents[m], pb.agents[m], pa.hooks[m], pb.hooks[m]
        ta, tb = aa.trajectory, ab.trajectory
        assert (ta.n_sa, ta.n_rt, aa.policy.update_step, aa.policy._noise_off, aa.policy._sample_off) == \
            (tb.n_sa, tb.n_rt, ab.policy.update_step, ab.policy._noise_off, ab.policy._sample_off), m
        for name in ("state", "action", "reward", "terminal"):
            assert torch.equal(getattr(ta, name), getattr(tb, name)), (m, name)
        for n in ("behavior_actor", "behavior_critic", "target_actor", "target_critic"):
            na, nb = getattr(aa.policy, n), getattr(ab.policy, n)
            for x, y in zip(na.model.params(), nb.model.params()):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (m, n)
            assert np.array_equal(_beta_powers(na).view(np.uint64), _beta_powers(nb).view(np.uint64)), (m, n)
        for n in ("behavior_actor", "behavior_critic"):
            ma, mb = getattr(aa.policy, n).model, getattr(ab.policy, n).model
            buf = [(C.c_float * ma.num_params)() for _ in range(4)]
            assert ma.lib.pdec_adam_get_state(ma.handle, buf[0], buf[1], None) == 0
            assert mb.lib.pdec_adam_get_state(mb.handle, buf[2], buf[3], None) == 0
            assert bytes(buf[0]) == bytes(buf[2]) and bytes(buf[1]) == bytes(buf[3]), (m, n)
        assert np.array_equal(np.asarray(ha.rewards), np.asarray(hb.rewards)) and len(hb.rewards) == 2, m
        assert torch.equal(pa.env.y[m], pb.env.y[m]) and torch.equal(pa.env.state[m], pb.env.state[m]), m
        for x, y in zip(ha.bestNNA.model.params(), hb.bestNNA.model.params()):
            assert np.array_equal(x, y), m


def test_refusals(pkg, monkeypatch):
    monkeypatch.setenv("PDEC_ROLLOUT_PERSISTENT", "1")
    setup = pkg.KSSetup.KS22()
    agents, nnas = _actors(pkg, setup, n=2)
    # differing actor shapes
    wide = pkg.create_agent(setup=pkg.KSSetup.KS22(drop_middle_layer=False), B=1, rng=np.random.default_rng(1))
    with pytest.raises(pkg.PdecError, match="same shape"):
        pkg.evaluate_actors(setup, nnas + [wide.policy.behavior_actor], n_inits=2)
    # learning = 1 through the C call
    env = pkg.PDEenv(setup, B=4, dtype=torch.float64, autoreset=False)
    handles = (pkg._lib.Handle * 2)(*[int(getattr(n.model.handle, "value", n.model.handle)) for n in nnas])
    served = C.c_int(1)
    P = pkg._lib.ptr
    y_before = env.y.clone()
    rc = env.lib.pdec_rollout_members(env.handle, handles, 2, 2, 5, P(env.y), P(env.state), P(env.action), 1.0, 1, None, None, None,
                                      None, None, None, None, C.byref(served))
    assert rc != 0 and served.value == 0
    with pytest.raises(pkg.PdecError, match="learning = 1"):
        pkg._lib.check(rc)
    torch.cuda.synchronize()
    assert torch.equal(env.y, y_before)
    # ... and the C call itself answers served = 0 for differing shapes, without an error and without touching anything
    h2 = (pkg._lib.Handle * 2)(handles[0], int(getattr(wide.policy.behavior_actor.model.handle, "value", 0)))
    served = C.c_int(1)
    assert env.lib.pdec_rollout_members(env.handle, h2, 2, 2, 5, P(env.y), P(env.state), P(env.action), 1.0, 0, None, None, None,
                                        None, None, None, None, C.byref(served)) == 0
    torch.cuda.synchronize()
    assert served.value == 0 and torch.equal(env.y, y_before)
    # which = "best" without kept actors
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    ags = [pkg.create_agent(setup=setup, B=1, rng=np.random.default_rng(i), noise_seed=i, stream=s_upd) for i in range(2)]
    pop = pkg.Population(setup, ags, [pkg.PDEhook(init_seed=i, collect_NNA=False) for i in range(2)], stream_env=s_env)
    with pytest.raises(pkg.PdecError, match="best actor"):
        pop.evaluate(which="best")
    with pytest.raises(pkg.PdecError, match="current"):
        pop.evaluate(which="latest")
