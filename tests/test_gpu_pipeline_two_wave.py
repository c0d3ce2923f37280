"""TrainPipeline with the KS step over two waves per trajectory pair (the default of the two-stream form; PDEC_TWO_WAVE=0: the
one-wave kernel) -- B = 8, 13 control steps issued eagerly, and 13 more replayed from captured graphs behind the steps a capture
takes (episodes of 13 steps, the shortest the graph periods allow, so both cross resets): the four networks, the losses,
the field, the state, action and reward rings BYTE-equal between the two.  The step is bit for bit the one-wave step
(test_gpu_ks_two_wave.py), and nothing else in the pipeline reads which kernel ran.  Pipelines the form does not serve -- one
stream, N = 1024, the finite-difference integrator, the SIMD-sharing step -- report two_wave = False and leave the setter off."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NETS = ("behavior_actor", "behavior_critic", "target_actor", "target_critic")


def make(pkg, use_graphs, B=8, serial=False, nx=256, **setup_kw):
    setup = pkg.KSSetup.bench_C2(nx, **setup_kw)
    s_env = torch.cuda.Stream()
    s_upd = s_env if serial else torch.cuda.Stream()
    y0 = setup.generate_random_init(np.random.default_rng(0), B) * 0.15
    env = pkg.PDEenv(setup, B=B, dtype=torch.float32, y0=y0, stream=s_env, autoreset=False)
    agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                             noise_seed=7, trajectory_length=1)
    agent.policy.act_noise = 0.3
    torch.cuda.synchronize()
    return pkg.TrainPipeline(env, agent, lag=2, episode_steps=13, stream_env=s_env, stream_upd=s_upd, use_graphs=use_graphs,
                             chunks=(6, 1), noise_seed=99)


def image(p):
    """everything 13 steps leave, as host arrays"""
    out = {n: [np.array(x) for x in getattr(p.policy, n).model.params()] for n in NETS}
    out["losses"] = [np.asarray(p.policy.losses())]
    out["y"], out["state"] = [p.y.cpu().numpy()], [p.state.cpu().numpy()]
    out["aring"] = [x.cpu().numpy() for x in p.aring]
    out["rring"] = [x.cpu().numpy() for x in p.rring]
    return out


@pytest.fixture(scope="module")
def one_wave(pkg):
    """the reference: the one-wave kernel, issued eagerly, after `tick` steps (where the capture leaves the captured case is
    the pipeline's business); each tick is computed once"""
    cache = {}

    def at(tick):
        if tick not in cache:
            mp = pytest.MonkeyPatch()
            mp.setenv("PDEC_TWO_WAVE", "0")
            try:
                p = make(pkg, False)
                assert not p.two_wave
                p.run(tick); p.sync()
                cache[tick] = image(p)
                p.close()
            finally:
                mp.undo()
        return cache[tick]
    return at


@pytest.mark.parametrize("graphs", [False, True])
def test_two_wave_pipeline_is_the_one_wave_pipeline(pkg, one_wave, graphs):
    p = make(pkg, graphs)
    assert p.two_wave and p.rpart is not None and not p.simd_sharing
    if graphs:
        p.run(5); p.capture()
        steps = p.tick + 13
        p.run(13); p.sync()
        assert p.n_graph_launches > 0
    else:
        steps = 13
        p.run(13); p.sync()
    got = image(p)
    assert p.tick == steps and np.isfinite(got["y"][0]).all() and np.isfinite(got["losses"][0]).all()
    for name, ref in one_wave(steps).items():
        assert len(ref) == len(got[name])
        for i, (a, b) in enumerate(zip(ref, got[name])):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (name, i)
    env = p.env
    p.close()
    assert not p.two_wave and env.set_two_wave_step(True) and not env.set_two_wave_step(False)     # close() handed it back off


def test_pipelines_the_form_does_not_serve(pkg, monkeypatch):
    for kw in (dict(serial=True), dict(nx=1024), dict(integrator="rk4_fd")):
        p = make(pkg, False, **kw)
        assert not p.two_wave, kw
        p.run(2); p.sync()
        assert bool(torch.isfinite(p.y).all())
        p.close()
    monkeypatch.setenv("PDEC_SHARE", "1")
    p = make(pkg, False)
    assert p.simd_sharing and not p.two_wave
    p.close()
