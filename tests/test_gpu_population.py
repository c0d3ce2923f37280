"""Populations (population.py): M independently seeded single-trajectory learners trained side by side, each of the three
per-step launches one launch of M workgroups.  Every member must end bit for bit where its solo `run` ends."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _beta_powers(nna):
    bp = (C.c_double * 2)()
    m = nna.model
    assert m.lib.pdec_adam_get_state(m.handle, None, None, bp) == 0
    return np.array([bp[0], bp[1]])


def _make(pkg, setup, seed, s_upd, random_init=True):
    agent = pkg.create_agent(setup=setup, B=1, rng=np.random.default_rng(seed), noise_seed=seed, stream=s_upd)
    hook = pkg.PDEhook(min_best_episode=1, use_random_init=random_init, init_seed=seed)
    agent.policy.act_noise = setup.act_noise
    return agent, hook


def _solo(pkg, setup, seed, stops, decay, random_init=True):
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    env = pkg.PDEenv(setup, B=1, dtype=torch.float64, stream=s_env)
    agent, hook = _make(pkg, setup, seed, s_upd, random_init)
    for stop in stops:
        pkg.run(agent, env, stop, hook)
        agent.policy.act_noise *= decay
    torch.cuda.synchronize()
    return env, agent, hook


def _population(pkg, setup, seeds, stop_lists, decay, random_init=None):
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    members = [_make(pkg, setup, s, s_upd, True if random_init is None else random_init[i]) for i, s in enumerate(seeds)]
    pop = pkg.Population(setup, [a for a, _ in members], [h for _, h in members], stream_env=s_env, dtype=torch.float64)
    for k in range(len(stop_lists[0])):
        pop.run([sl[k] for sl in stop_lists])
        for a in pop.agents:
            a.policy.act_noise *= decay
    torch.cuda.synchronize()
    return pop


def _assert_member_equals_solo(pop, m, solo):
    es, as_, hs = solo
    ad, hd = pop.agents[m], pop.hooks[m]
    pd, ps, td, ts = ad.policy, as_.policy, ad.trajectory, as_.trajectory
    assert (td.n_sa, td.n_rt, pd.update_step, pd._noise_off, pd._sample_off) == \
        (ts.n_sa, ts.n_rt, ps.update_step, ps._noise_off, ps._sample_off), m
    for name in ("state", "action", "reward", "terminal"):
        assert torch.equal(getattr(td, name), getattr(ts, name)), (m, name)
    for n in ("behavior_actor", "behavior_critic", "target_actor", "target_critic"):
        md, ms = getattr(pd, n).model, getattr(ps, n).model
        for x, y in zip(md.params(), ms.params()):
            assert np.array_equal(x, y), (m, n)
        assert np.array_equal(_beta_powers(getattr(pd, n)).view(np.uint64), _beta_powers(getattr(ps, n)).view(np.uint64)), (m, n)
    for n in ("behavior_actor", "behavior_critic"):            # ADAM moments
        md, ms = getattr(pd, n).model, getattr(ps, n).model
        k = md.nparams if hasattr(md, "nparams") else sum(int(np.asarray(x).size) for x in md.params())
        bd, bs = [(C.c_float * k)() for _ in range(4)], None
        assert md.lib.pdec_adam_get_state(md.handle, bd[0], bd[1], None) == 0
        assert ms.lib.pdec_adam_get_state(ms.handle, bd[2], bd[3], None) == 0
        assert bytes(bd[0]) == bytes(bd[2]) and bytes(bd[1]) == bytes(bd[3]), (m, n, "adam")
    assert torch.equal(pop.env.y[m], es.y[0]) and torch.equal(pop.env.state[m], es.state[0]), m
    assert np.array_equal(np.asarray(hd.rewards), np.asarray(hs.rewards)), m
    assert (hd.bestepisode, hd.bestreward, len(hd.bestDF)) == (hs.bestepisode, hs.bestreward, len(hs.bestDF)), m
    for rd, rs in zip(hd.bestDF, hs.bestDF):
        assert rd["timestep"] == rs["timestep"]
        for k in ("action", "p", "y", "reward"):
            assert np.array_equal(rd[k], rs[k]), (m, k)
    for x, y in zip(hd.bestNNA.model.params(), hs.bestNNA.model.params()):
        assert np.array_equal(x, y), m


@pytest.mark.parametrize("which", ["ks22", "ks22_three_layer", "ks22_early_ends", "ks200", "keller_segel"])
def test_members_equal_solo_runs(pkg, which):
    seeds, steps, loops, decay = [3, 11, 29], 150, 2, 0.2
    if which == "ks22":
        setup = pkg.KSSetup.KS22()
    elif which == "ks22_three_layer":
        setup = pkg.KSSetup.KS22(drop_middle_layer=False)
    elif which == "ks22_early_ends":
        setup, steps = pkg.KSSetup.KS22(max_value=4.0), 200
    elif which == "ks200":
        setup, seeds, steps = pkg.KSSetup.KS200(), [3, 11], 60
    else:
        setup, steps, loops, decay = pkg.KellerSegelSetup(), 1400, 2, 0.6
    stop_lists = [[pkg.StopAfterEpisodeWithMinSteps(steps) for _ in range(loops)] for _ in seeds]
    pop = _population(pkg, setup, seeds, stop_lists, decay)
    for m, s in enumerate(seeds):
        solo = _solo(pkg, setup, s, [pkg.StopAfterEpisodeWithMinSteps(steps) for _ in range(loops)], decay)
        _assert_member_equals_solo(pop, m, solo)
    if which == "ks22_early_ends":       # within one lock-step episode, one member ended early while another ran to te
        T = pop._logs.T
        mixed = [n for n in pop.episode_steps if ((n > 0) & (n < T)).any() and (n == T).any()]
        assert mixed, [n.tolist() for n in pop.episode_steps]


def test_members_stop_at_different_points(pkg):
    setup = pkg.KSSetup.KS22()
    seeds, eps = [5, 6, 7], [1, 3, 2]
    pop = _population(pkg, setup, seeds, [[pkg.StopAfterEpisode(e)] for e in eps], 1.0)
    for m, (s, e) in enumerate(zip(seeds, eps)):
        assert len(pop.hooks[m].rewards) == e
        _assert_member_equals_solo(pop, m, _solo(pkg, setup, s, [pkg.StopAfterEpisode(e)], 1.0))


def test_mixed_random_inits(pkg):
    """members with and without random initial fields in one population; Keller-Segel's temporal stack makes a re-featurized
    reset state differ from the one a solo run without random inits keeps"""
    setup = pkg.KellerSegelSetup()
    seeds, rnd = [2, 8, 13], [True, False, True]
    pop = _population(pkg, setup, seeds, [[pkg.StopAfterEpisode(2)] for _ in seeds], 1.0, rnd)
    for m, (s, r) in enumerate(zip(seeds, rnd)):
        _assert_member_equals_solo(pop, m, _solo(pkg, setup, s, [pkg.StopAfterEpisode(2)], 1.0, r))


@pytest.mark.slow
def test_more_members_than_compute_units(pkg):
    setup = pkg.KSSetup.KS22()
    seeds = list(range(100, 420))
    pop = _population(pkg, setup, seeds, [[pkg.StopAfterEpisode(1)] for _ in seeds], 1.0)
    for m in (0, 161, 319):
        _assert_member_equals_solo(pop, m, _solo(pkg, setup, seeds[m], [pkg.StopAfterEpisode(1)], 1.0))


def _env_step_args(env, y, a, ap, st):
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    out = dict(y=torch.empty_like(y), p=torch.empty(env._pshape, dtype=env.dtype, device=env.device),
               state=torch.empty(env._sshape, dtype=env.dtype, device=env.device),
               reward=torch.empty((env.B, env.setup.reward_len), dtype=env.dtype, device=env.device),
               done=torch.empty(env.B, dtype=torch.int32, device=env.device))
    rc = env.lib.pdec_env_step(env.handle, P(y), P(a), P(ap), P(st), P(out["y"]), P(out["p"]), P(out["state"]), P(out["reward"]),
                               P(out["done"]))
    assert rc == 0
    return out


@pytest.mark.parametrize("which", ["ks22", "ks200", "ks500", "keller_segel"])
def test_member_layout_env_step_equals_single_trajectory_steps(pkg, which):
    setup = {"ks22": pkg.KSSetup.KS22, "ks200": pkg.KSSetup.KS200, "ks500": pkg.KSSetup.KS500,
             "keller_segel": pkg.KellerSegelSetup}[which]()
    M = 5
    big = pkg.PDEenv(setup, B=M, dtype=torch.float64, autoreset=False)
    assert big.lib.pdec_env_set_member_layout(big.handle, 1) == 0
    one = pkg.PDEenv(setup, B=1, dtype=torch.float64, autoreset=False)
    y = torch.empty_like(big.y)
    big.random_init(17, 0, out=y)
    g = torch.Generator(device="cpu").manual_seed(1)
    a = (torch.rand(big._ashape, generator=g, dtype=torch.float64) * 2 - 1).cuda()
    ap = (torch.rand(big._ashape, generator=g, dtype=torch.float64) * 2 - 1).cuda()
    st = big.featurize(y, big.state if setup.temporal_steps > 1 else None)
    y[2].fill_(float("nan"))                               # a blown-up member must not reach its neighbours
    out = _env_step_args(big, y, a, ap, st)
    torch.cuda.synchronize()
    for m in range(M):
        o1 = _env_step_args(one, y[m:m + 1].contiguous(), a[m:m + 1].contiguous(), ap[m:m + 1].contiguous(), st[m:m + 1].contiguous())
        torch.cuda.synchronize()
        for k in ("y", "p", "state", "reward", "done"):
            x, r = np.atleast_1d(out[k][m].cpu().numpy()), np.atleast_1d(o1[k][0].cpu().numpy())
            if m == 2:
                continue
            assert np.array_equal(x.view(np.uint8), r.view(np.uint8)), (which, m, k)


@pytest.mark.parametrize("which", ["ks22", "keller_segel"])
def test_member_random_inits_equal_single_trajectory_draws(pkg, which):
    setup = pkg.KSSetup.KS22() if which == "ks22" else pkg.KellerSegelSetup()
    seeds, offs = [4, 9, 4, 77], [0, 3, 6, 1]
    big = pkg.PDEenv(setup, B=len(seeds), dtype=torch.float64, autoreset=False)
    one = pkg.PDEenv(setup, B=1, dtype=torch.float64, autoreset=False)
    so = torch.tensor([seeds, offs], dtype=torch.int64, device="cuda:0")
    out = torch.empty_like(big.y)
    assert big.lib.pdec_env_random_init_members(big.handle, C.c_void_p(so[0].data_ptr()), C.c_void_p(so[1].data_ptr()),
                                                C.c_void_p(out.data_ptr())) == 0
    for m, (s, o) in enumerate(zip(seeds, offs)):
        r = torch.empty_like(one.y)
        one.random_init(s, o, out=r)
        torch.cuda.synchronize()
        assert torch.equal(out[m], r[0]), m


def test_refusals(pkg):
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    ks = pkg.KSSetup.KS22()

    def members(setup, n=2, **kw):
        ags = [pkg.create_agent(setup=setup, B=1, rng=np.random.default_rng(i), noise_seed=i, stream=s_upd, **kw) for i in range(n)]
        return ags, [pkg.PDEhook(init_seed=i) for i in range(n)]

    ags, hks = members(ks)
    ags[1].policy.update_loops += 1
    with pytest.raises(pkg.PdecError, match="update_loops"):
        pkg.Population(ks, ags, hks, stream_env=s_env)
    ags, hks = members(ks)
    ags[1].policy.sampling = "host"
    with pytest.raises(pkg.PdecError, match="host sampling"):
        pkg.Population(ks, ags, hks, stream_env=s_env)
    mem = pkg.KSSetup.KS22(memory_size=1)
    with pytest.raises(pkg.PdecError, match="memory_size"):
        pkg.Population(mem, *members(mem), stream_env=s_env)
    fl = pkg.FluidSetup(nx=64)
    with pytest.raises(pkg.PdecError, match="FluidSetup"):
        pkg.Population(fl, *members(ks), stream_env=s_env)
    k2 = pkg.KellerSegel2DSetup()
    with pytest.raises(pkg.PdecError, match="KellerSegel2DSetup"):
        pkg.Population(k2, *members(ks), stream_env=s_env)
