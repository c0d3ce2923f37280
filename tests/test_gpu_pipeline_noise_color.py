"""TrainPipeline with temporally correlated exploration noise (noise_corr=, set_noise_corr) on the KS C2 geometry at nx = 256,
B = 4, lag 2, and the solo run() at B = 1 on KS22.

1. With noise_corr set, the recorded-call issue and the captured graphs are the eager issue bit for bit -- every ring buffer, the
   four networks' parameters and the noise states.  Each form runs at the shortest episode at which it exists: eager at 3 steps,
   recorded calls at 5 (an interior step behind an interior step), graphs at 13 (longer than two ring periods of 6).
2. noise_corr = 0 is the plain pipeline bit for bit (episodes of 3 steps, two of them and a step).
3. The states are zeroed ahead of every episode's first acting launch: with learning rates 0 the first action of episodes 1 and 2
   is greedy + scale_b b z (z: the stream's normals at that step's counter), the second step of an episode carries
   a b z_0 + b z_1, and the noise states are the model's -- within the bounds of noise_color_cases.py.
4. set_noise_corr between episodes (a host array, then a device tensor) keeps the recorded programs -- the same list objects --
   and the buffers' pointers, the run stays the eager pipeline's under the same schedule bit for bit, and the actions that
   follow are the model's at the new correlations.
5. Solo run() for two episodes with set_noise_corr(0.8): the device-episode path and the stage loop leave identical networks,
   replay rows, counters, noise states and hook.rewards."""
import numpy as np
import pytest

import noise_color_cases as cc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

B, NOISE, SEED = 4, 0.3, 99
CORR = np.array([0.9, 0.0, 0.5, 0.9])
SCALE = np.array([0.3, 0.6, 0.0, 0.15])


def _bits(t):
    t = t.contiguous()
    return t.view({8: torch.int64, 4: torch.int32}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _pipe(pkg, E, use_graphs, noise_corr=None, noise_scale=None, eta=None):
    setup = pkg.KSSetup.bench_C2(256)
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    y0 = setup.generate_random_init(np.random.default_rng(0), B) * 0.15
    env = pkg.PDEenv(setup, B=B, dtype=torch.float32, y0=y0, stream=s_env, autoreset=False)
    agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                             noise_seed=7, trajectory_length=1)
    agent.policy.act_noise = NOISE
    agent.policy.act_limit = 100.0
    if eta is not None:
        agent.policy.behavior_actor.optimizer.eta = agent.policy.behavior_critic.optimizer.eta = eta
    torch.cuda.synchronize()
    return pkg.TrainPipeline(env, agent, lag=2, episode_steps=E, stream_env=s_env, stream_upd=s_upd, use_graphs=use_graphs,
                             chunks=(6, 1), noise_seed=SEED, log_episodes=8, noise_corr=noise_corr, noise_scale=noise_scale)


def _assert_same_run(pa, pb, what):
    assert pa.tick == pb.tick, what
    for ring in ("ybuf", "sring", "aring", "rring", "fring", "tring"):
        for i, (x, y) in enumerate(zip(getattr(pa, ring), getattr(pb, ring))):
            assert _same(x, y), (what, ring, i)
    for nm in ("behavior_actor", "behavior_critic", "target_actor", "target_critic"):
        for x, y in zip(getattr(pa.policy, nm).model.params(), getattr(pb.policy, nm).model.params()):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (what, nm)
    if pa.noise_state is not None and pb.noise_state is not None:
        assert _same(pa.noise_state, pb.noise_state), (what, "noise states")
    assert bool(torch.isfinite(pa.y).all())


@pytest.mark.parametrize("mode", ["recorded", "graphs"])
def test_recorded_and_captured_steps_are_the_eager_ones(pkg, monkeypatch, mode):
    E = 13 if mode == "graphs" else 5
    monkeypatch.setenv("PDEC_FAST_EAGER", "0")
    pe = _pipe(pkg, E, False, noise_corr=CORR, noise_scale=SCALE)
    monkeypatch.setenv("PDEC_FAST_EAGER", "1")
    pm = _pipe(pkg, E, mode == "graphs", noise_corr=CORR, noise_scale=SCALE)
    assert not pe.fast_eager and pm.fast_eager
    assert pm._scalar_key()[0] == "noise_scale" and "noise_corr" in pm._scalar_key()
    assert pm.noise_state.shape == (pm.cols * pm.na,) and pm.noise_ab.shape == (B, 2)
    assert np.array_equal(pm.noise_ab.cpu().numpy(), cc.ab_of(CORR))
    if mode == "graphs":
        pm.run(5)
        pm.capture()
        assert pm._captured and pm.graphs
    T = (pm.tick // E + 2) * E + 2                       # two whole episodes on, and two steps into the next
    pm.run(T - pm.tick), pe.run(T)
    pm.sync(), pe.sync()
    if mode == "graphs":
        assert pm.n_graph_launches > 0
    else:
        assert pm._progs and not pe._progs
    _assert_same_run(pe, pm, mode)
    assert bool(pm.noise_state.any())
    for p in (pe, pm):
        p.close()


def test_zero_correlation_is_the_plain_pipeline(pkg):
    E = 3
    ps, pz = _pipe(pkg, E, False), _pipe(pkg, E, False, noise_corr=0.0)
    assert "noise_corr" not in ps._scalar_key() and ps.noise_state is None and ps.actor.noise_color is None
    assert pz.noise_ab.cpu().numpy().tolist() == [[0.0, 1.0]] * B
    ps.run(2 * E + 1), pz.run(2 * E + 1)
    ps.sync(), pz.sync()
    _assert_same_run(ps, pz, "a = 0")
    # and a correlation moves the run
    pc = _pipe(pkg, E, False, noise_corr=0.9)
    pc.run(2 * E + 1)
    pc.sync()
    assert not _same(pc.y, ps.y)
    for p in (ps, pz, pc):
        p.close()


def _greedy(pkg, p, state):
    L = pkg._lib
    out = torch.empty((p.cols, 1), dtype=torch.float32, device="cuda:0")
    L.check(p.lib.pdec_policy_act_rng(p.actor.handle, L.ptr(state), p.cols, 0.0, 100.0, 0, 0, 0, L.ptr(out)))
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64).reshape(-1)


def _check_step(pkg, p, k, x_prev, corr, scale, t_in_episode):
    """step k just ran (synchronised): its action and the noise states against the model from x_prev; returns the model's x"""
    from oracle import rng
    A = p.cols // B
    inc = (p.cols * p.na + 3) // 4
    z = rng.randn(SEED, k * inc, p.cols)
    a_c, s_c = np.repeat(corr, A), np.repeat(scale, A)
    x = cc.model(x_prev.reshape(-1, 1), np.repeat(cc.ab_of(corr), A, axis=0), z.reshape(1, -1, 1))[0].reshape(-1)
    e_t = cc.state_tolerance(t_in_episode + 1, a_c)
    got_x = p.noise_state.cpu().numpy()
    assert (np.abs(got_x - x) <= e_t).all(), (k, float(np.abs(got_x - x).max()), float(e_t.min()))
    g = _greedy(pkg, p, p.sring[k % 6])
    act = p.aring[k % 3].cpu().numpy().astype(np.float64).reshape(-1)
    err, tol = np.abs(act - g - s_c * x), cc.action_tolerance(g, s_c, x, "f32", e_t)
    assert (err <= tol).all(), (k, float(err.max()), float(tol.min()))
    assert (act[s_c == 0] == g[s_c == 0]).all() and (act[s_c > 0] != g[s_c > 0]).sum() > (s_c > 0).sum() // 2
    return x


def test_states_start_every_episode_at_zero(pkg):
    E = 3
    p = _pipe(pkg, E, False, noise_corr=CORR, noise_scale=SCALE, eta=0.0)
    x = np.zeros(p.cols)
    for k in range(2 * E):
        p.run(1)
        p.sync()
        torch.cuda.synchronize()
        carried = x
        if k % E == 0:
            x = np.zeros(p.cols)                          # zeroed ahead of the episode's first acting launch
        x = _check_step(pkg, p, k, x, CORR, SCALE, k % E)
        if k == E:
            # ... and not carried over: continued from episode 1's last state, the correlated columns would be somewhere else
            a_c = np.repeat(CORR, p.cols // B)
            assert (np.abs(a_c * carried)[a_c > 0] > 1e-6).sum() > (a_c > 0).sum() // 2
    # reset_from() zeroes them too
    assert bool(p.noise_state.any())
    p.reset_from(p.env.y0)
    p.sync()
    torch.cuda.synchronize()
    assert not bool(p.noise_state.any())
    p.close()


def test_a_schedule_keeps_the_recorded_steps(pkg, monkeypatch):
    E = 5
    monkeypatch.setenv("PDEC_FAST_EAGER", "0")
    pe = _pipe(pkg, E, False, noise_corr=CORR, noise_scale=SCALE, eta=0.0)
    monkeypatch.setenv("PDEC_FAST_EAGER", "1")
    pr = _pipe(pkg, E, False, noise_corr=CORR, noise_scale=SCALE, eta=0.0)
    pr.run(2 * E), pe.run(2 * E)
    pr.sync()
    progs, items, ab, state = pr._progs, dict(pr._progs), pr.noise_ab, pr.noise_state
    assert items
    second = np.array([0.5, 0.9, 0.0, 0.2])
    third = np.array([0.0, 0.3, 0.95, 0.5])
    for new in (second, torch.as_tensor(third, device="cuda:0")):        # a host array, then a device tensor (no host wait)
        pr.set_noise_corr(new), pe.set_noise_corr(new)
        host = new if isinstance(new, np.ndarray) else third
        k0 = pr.tick
        x = np.zeros(pr.cols)
        for k in range(k0, k0 + E):
            pr.run(1), pe.run(1)
            pr.sync()
            torch.cuda.synchronize()
            x = _check_step(pkg, pr, k, x, host, SCALE, k - k0)
        got = pr.noise_ab.cpu().numpy()
        assert np.array_equal(got[:, 0], host) and np.abs(got[:, 1] - cc.ab_of(host)[:, 1]).max() <= 2.0 ** -52
    pe.sync()
    assert pr._progs is progs and all(pr._progs[k] is v for k, v in items.items()) and len(pr._progs) == len(items)
    assert pr.noise_ab is ab and pr.noise_state is state and pr.actor.noise_color[0] is state
    _assert_same_run(pe, pr, "schedule")
    # the setter's refusals, by the numbers; a refused call wrote nothing
    with pytest.raises(ValueError, match=rf"TrainPipeline.set_noise_corr: expected a scalar or {B} correlations in a 1-D array, got shape \({B + 1},\)"):
        pr.set_noise_corr(np.zeros(B + 1))
    with pytest.raises(ValueError, match=r"entry 2 is 1\.0"):
        pr.set_noise_corr([0.0, 0.1, 1.0, 0.0])
    assert np.array_equal(pr.noise_ab.cpu().numpy()[:, 0], third)
    # off: the key changes, the recorded steps go
    pr.set_noise_corr(None)
    assert pr.noise_state is None and pr.actor.noise_color is None
    pr.run(1)
    pr.sync()
    assert pr._progs is not progs
    for p in (pe, pr):
        p.close()


def test_solo_run_device_episodes_and_stage_loop_agree(pkg):
    run_mod = __import__("importlib").import_module(pkg.__name__ + ".run")
    out = []
    for dev in (True, False):
        setup = pkg.KSSetup.KS22()
        s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
        env = pkg.PDEenv(setup, B=1, dtype=torch.float64, stream=s_env)
        agent = pkg.create_agent(setup=setup, B=1, rng=np.random.default_rng(7), noise_seed=7, stream=s_upd)
        hook = pkg.PDEhook(min_best_episode=1, use_random_init=True, init_seed=7)
        agent.policy.act_noise = setup.act_noise
        agent.policy.set_noise_corr(0.8)
        stop = pkg.StopAfterEpisode(2)
        assert run_mod.device_episodes_ok(agent, env, stop, hook)
        pkg.run(agent, env, stop, hook, device_episodes=dev)
        torch.cuda.synchronize()
        out.append((env, agent, hook))
    (ed, ad, hd), (es, as_, hs) = out
    pd, ps, td, ts = ad.policy, as_.policy, ad.trajectory, as_.trajectory
    assert len(hd.rewards) == len(hs.rewards) >= 2 and pd._noise_off > 0
    assert (td.n_sa, td.n_rt, pd.update_step, pd._noise_off, pd._sample_off) == (ts.n_sa, ts.n_rt, ps.update_step, ps._noise_off, ps._sample_off)
    for name in ("state", "action", "reward", "terminal"):
        assert torch.equal(getattr(td, name), getattr(ts, name)), name
    for n in ("behavior_actor", "behavior_critic", "target_actor", "target_critic"):
        for x, y in zip(getattr(pd, n).model.params(), getattr(ps, n).model.params()):
            assert np.array_equal(x, y), n
    assert np.array_equal(np.asarray(hd.rewards), np.asarray(hs.rewards))
    assert pd.noise_state is not None and bool(pd.noise_state.any()) and _same(pd.noise_state, ps.noise_state)
    assert pd.noise_ab[:, 0].tolist() == [0.8] and torch.equal(ed.y, es.y)
    # and the correlation acts: the white run ends elsewhere
    setup = pkg.KSSetup.KS22()
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    env = pkg.PDEenv(setup, B=1, dtype=torch.float64, stream=s_env)
    agent = pkg.create_agent(setup=setup, B=1, rng=np.random.default_rng(7), noise_seed=7, stream=s_upd)
    hook = pkg.PDEhook(min_best_episode=1, use_random_init=True, init_seed=7)
    agent.policy.act_noise = setup.act_noise
    pkg.run(agent, env, pkg.StopAfterEpisode(2), hook)
    torch.cuda.synchronize()
    assert not np.array_equal(np.asarray(hook.rewards), np.asarray(hd.rewards))
