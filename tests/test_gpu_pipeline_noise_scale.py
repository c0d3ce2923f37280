"""TrainPipeline with a per-trajectory exploration amplitude (noise_scale=, set_noise_scale): the KS C2 geometry at nx = 256, B = 6,
lag 2.

1. An array of equal values is the scalar pipeline bit for bit -- every ring buffer, the four networks' parameters and
   episode_returns() -- on eager issue, on recorded-call issue (two 5-step episodes each) and on captured graphs (two 13-step
   episodes: the pipeline captures graphs only for episodes longer than two ring periods of 6).
2. A schedule: after capture(), set_noise_scale(0.2 s) between episodes keeps _captured, the recorded programs and the graph
   handles (the same objects), and the run is bit for bit an eager pipeline given the same schedule; the scalar pipeline whose
   act_noise changes at the same point drops its graphs.
3. Trajectories with amplitude 0 take clamp(actor(state)) at every step: the action ring against pdec_policy_act_rng(learning = 0)
   on the state ring, bit for bit, step by step (learning rates 0, so the actor the check calls is the one every step read)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

B, NOISE = 6, 0.3


def _bits(t):
    t = t.contiguous()
    return t.view({8: torch.int64, 4: torch.int32}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _pipe(pkg, E, use_graphs, noise_scale=None, eta=None):
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
                             chunks=(6, 1), noise_seed=99, log_episodes=8, noise_scale=noise_scale)


def _assert_same_run(pa, pb, what):
    assert pa.tick == pb.tick, what
    for ring in ("ybuf", "sring", "aring", "rring", "fring", "tring"):
        for i, (x, y) in enumerate(zip(getattr(pa, ring), getattr(pb, ring))):
            assert _same(x, y), (what, ring, i)
    for nm in ("behavior_actor", "behavior_critic", "target_actor", "target_critic"):
        for x, y in zip(getattr(pa.policy, nm).model.params(), getattr(pb.policy, nm).model.params()):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (what, nm)
    ra, rb = pa.episode_returns(), pb.episode_returns()
    assert np.array_equal(ra[0].view(np.uint64), rb[0].view(np.uint64)) and np.array_equal(ra[1], rb[1]) and ra[2] == rb[2], what
    assert ra[0].shape[0] >= 2 and bool(torch.isfinite(pa.y).all())


@pytest.mark.parametrize("mode", ["eager", "recorded", "graphs"])
def test_equal_values_are_the_scalar_pipeline(pkg, monkeypatch, mode):
    monkeypatch.setenv("PDEC_FAST_EAGER", "0" if mode == "eager" else "1")
    E = 13 if mode == "graphs" else 5
    ps = _pipe(pkg, E, mode == "graphs")
    pa = _pipe(pkg, E, mode == "graphs", noise_scale=np.full(B, NOISE))
    assert ps.fast_eager == pa.fast_eager == (mode != "eager")
    assert ps._scalar_key()[0] == NOISE and pa._scalar_key()[0] == "noise_scale" and ps._scalar_key()[1:] == pa._scalar_key()[1:]
    assert pa.noise_scale.dtype == torch.float64 and pa.noise_scale.tolist() == [NOISE] * B
    for p in (ps, pa):
        if mode == "graphs":
            p.run(5)
            p.capture()
            assert p._captured
        p.run((p.tick // E + 3) * E - p.tick)      # to an episode boundary, at least two whole episodes on
        p.sync()
    if mode == "graphs":
        assert ps.n_graph_launches > 0 and pa.n_graph_launches == ps.n_graph_launches
    if mode == "recorded":
        assert pa._progs and ps._progs
    if mode == "eager":
        assert not pa._progs
    _assert_same_run(ps, pa, mode)
    # and the amplitudes act: another level moves the run
    pb = _pipe(pkg, E, False, noise_scale=np.full(B, 2 * NOISE))
    pb.run(ps.tick)
    pb.sync()
    assert not _same(pb.y, ps.y)
    for p in (ps, pa, pb):
        p.close()


def test_a_schedule_keeps_the_recorded_steps_and_the_graphs(pkg):
    E = 13
    s = np.array([0.3, 0.05, 0.0, 0.6, 0.3, 0.15])
    pg, pe, ps = _pipe(pkg, E, True, noise_scale=s), _pipe(pkg, E, False, noise_scale=s), _pipe(pkg, E, True)
    for p in (pg, ps):
        p.run(5)
        p.capture()
        assert p._captured and p.graphs
    assert pg.tick == ps.tick
    T1 = (pg.tick // E + 2) * E                    # an episode boundary
    pg.run(T1 - pg.tick), ps.run(T1 - ps.tick), pe.run(T1)
    progs, prog_items, graphs, buf = pg._progs, dict(pg._progs), dict(pg.graphs), pg.noise_scale
    n_launches = pg.n_graph_launches
    # between episodes: a host array into the pipeline's buffer, then a device tensor (copied without a host wait)
    pg.set_noise_scale(0.2 * s), pe.set_noise_scale(0.2 * s)
    pg.run(E), pe.run(E)
    dev = torch.as_tensor(0.04 * s, device="cuda:0")
    pg.set_noise_scale(dev), pe.set_noise_scale(dev)
    pg.run(E), pe.run(E)
    pg.sync(), pe.sync()
    assert pg._captured and pg.noise_scale is buf and pg.noise_scale.data_ptr() == buf.data_ptr()
    assert pg._progs is progs and all(pg._progs[k] is v for k, v in prog_items.items())
    assert set(pg.graphs) == set(graphs) and all(pg.graphs[k] is h for k, h in graphs.items())
    assert pg.n_graph_launches > n_launches
    assert np.array_equal(pg.noise_scale.cpu().numpy(), 0.04 * s) and np.array_equal(pe.noise_scale.cpu().numpy(), 0.04 * s)
    _assert_same_run(pg, pe, "schedule")
    # the contrast: the scalar pipeline drops its graphs when act_noise changes
    ps.policy.act_noise = 0.2 * NOISE
    ps.run(1)
    assert not ps._captured and ps.graphs == {}
    # refusals of the setter, by the numbers
    with pytest.raises(ValueError, match=rf"TrainPipeline.set_noise_scale: expected {B} amplitudes in a 1-D array, got shape \({B + 1},\)"):
        pg.set_noise_scale(np.zeros(B + 1))
    with pytest.raises(ValueError, match=r"entry 2 is -0\.1"):
        pg.set_noise_scale([0.0, 0.1, -0.1, 0.0, 0.0, 0.0])
    assert np.array_equal(pg.noise_scale.cpu().numpy(), 0.04 * s)         # a refused call wrote nothing
    for p in (pg, pe, ps):
        p.sync()
        p.close()


def test_zero_amplitude_trajectories_act_greedily(pkg):
    L = pkg._lib
    E = 5
    s = np.array([0.0, 0.4, 0.0, 0.0, 1.5, 0.4])
    p = _pipe(pkg, E, False, noise_scale=s, eta=0.0)
    A = p.cols // B
    zero = torch.as_tensor(s == 0.0, device="cuda:0")
    out = torch.empty((p.cols, 1), dtype=torch.float32, device="cuda:0")
    moved = 0
    for k in range(2 * E):
        p.run(1)
        p.sync()
        torch.cuda.synchronize()
        state, act = p.sring[k % 6], p.aring[k % 3]
        L.check(p.lib.pdec_policy_act_rng(p.actor.handle, L.ptr(state), p.cols, 0.0, 100.0, 0, 0, 0, L.ptr(out)))
        torch.cuda.synchronize()
        greedy = out.view(B, A)
        got = act.reshape(B, A)
        assert torch.equal(_bits(got)[zero], _bits(greedy)[zero]), k
        moved += int((got[~zero] != greedy[~zero]).sum())
    assert moved > (B - int(zero.sum())) * A * E          # the others explore
    p.close()
