"""The 2-D fluid environment in fp32 (complex64 spectra, (re, im) interleaved): the wave FFT, the right-hand side, do_step,
the closures and the fused env step against the fp64 NumPy oracle (oracle/fluid.py); the drift of a 51-step trajectory
against the fp64 GPU path; batch independence; the Fluid_8 learning curve on an fp32 environment.

Tolerances are relative to max|reference| and about ten times a CPU estimate of the fp32 error made with single-precision
FFTs and fp32 wavenumbers (rhs 2e-7, one control step 4e-7, 51 control steps 5e-6 on the physical field)."""
import ctypes as C

import numpy as np
import pytest

from util import to_dev, train

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F32, F64 = torch.float32, torch.float64


def _mem(z):    # Julia complex [.., ny, nx] -> memory [.., nx, ny, 2]
    z = np.swapaxes(np.asarray(z, dtype=np.complex128), -1, -2)
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1))


def _jul(t):    # memory [.., nx, ny, 2] -> Julia complex [.., ny, nx] (complex128)
    a = t.detach().cpu().numpy().astype(np.float64)
    return np.swapaxes(a[..., 0] + 1j * a[..., 1], -1, -2)


_PAIRS = {}


def _pair(pkg, n, ifpad=1, spa=4, K=None, variance=0.08, physical=False):
    """(product setup, oracle config); memoised -- the sensor tables of the large grids take long to build on the host.
    physical: dt = K / (16 n), so that the K sub-steps are of the size the reference's scripts take (h = dt / floor(16 nx dt),
    FluidSetup.jl:47) -- a few sub-steps of that size instead of a whole control step.  (K sub-steps spanning dt = 0.02 violate
    the advective CFL limit by 20 - 80 x: the RK4 then amplifies every rounding error, fp64's into the 1e-12 range, fp32's
    into the 1e-4 - 1e-2 range.)"""
    from oracle import fluid
    key = (n, ifpad, spa, K, variance, physical)
    dt = {"dt": K / (16.0 * n)} if physical else {}
    if key not in _PAIRS:
        setup = pkg.FluidSetup(nx=n, ifpad=ifpad, sensors_per_axis=spa, variance=variance, oversampling=K, **dt)
        cfg = fluid.FluidConfig(nx=n, ifpad=ifpad, sensors_per_axis=spa, variance=variance, oversampling=K, **dt)
        _PAIRS[key] = (setup, cfg)
    return _PAIRS[key]


def _fields(cfg, B, seed, hermitian=True):
    """B initial conditions ic(4) (optionally made non-Hermitian) and B random forcings, rounded to complex64 so that the
    oracle sees exactly the fp32 environment's input"""
    from oracle import fluid
    rng = np.random.default_rng(seed)
    y = np.stack([fluid.ic(cfg, 4, rng) for _ in range(B)])
    if not hermitian:
        y = y + 0.05 * np.abs(y).max() * (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape))
    p = np.stack([np.fft.fft2(rng.standard_normal((cfg.ny, cfg.nx))) for _ in range(B)])
    return y.astype(np.complex64).astype(np.complex128), p.astype(np.complex64).astype(np.complex128)


def _rel(got, ref):
    return np.abs(got - ref).max() / np.abs(ref).max()


# ---------------------------------------------------------------------------------------------------------- wave FFT


@pytest.mark.parametrize("n", [64, 128, 192, 256, 384, 512, 768])
def test_wave_fft_f32_matches_numpy(pkg, n):
    """pdec_debug_wave_fft_f32 (csrc/wave_fft.hpp on complex float, 2-dword lane exchanges): forward and unnormalised inverse
    against numpy.fft in fp64, <= 2e-6 relative"""
    rng = np.random.default_rng(n)
    L = pkg._lib
    lib = L.init(0)
    nl = 9
    x = (rng.standard_normal((nl, n)) + 1j * rng.standard_normal((nl, n))).astype(np.complex64).astype(np.complex128)
    xin = to_dev(np.stack([x.real, x.imag], axis=-1), F32)
    out = torch.empty_like(xin)
    L.check(lib.pdec_debug_wave_fft_f32(L.ptr(xin), L.ptr(out), n, nl, -1))
    got = out.cpu().numpy().astype(np.float64)
    assert _rel(got[..., 0] + 1j * got[..., 1], np.fft.fft(x, axis=1)) <= 2e-6
    L.check(lib.pdec_debug_wave_fft_f32(L.ptr(xin), L.ptr(out), n, nl, +1))
    got = out.cpu().numpy().astype(np.float64)
    assert _rel(got[..., 0] + 1j * got[..., 1], np.fft.ifft(x, axis=1) * n) <= 2e-6


# ---------------------------------------------------------------------------------------------------------- right-hand side


@pytest.mark.parametrize("n,ifpad,herm", [(16, 1, True), (16, 1, False), (16, 0, False), (32, 1, False), (24, 1, True),
                                          (64, 1, True), (64, 0, True), (128, 1, True),
                                          (128, 0, False), (256, 0, False), (256, 1, False), (256, 1, True), (512, 0, True),
                                          (512, 1, False)])
def test_rhs_f32_matches_oracle(pkg, n, ifpad, herm):
    """fp32 env.rhs (src/fluid_rk4.jl:134-190) on the grid of test_gpu_fluid.test_rhs_matches_oracle: <= 2e-6 relative"""
    from oracle import fluid
    setup, cfg = _pair(pkg, n, ifpad, spa=8 if n >= 256 else 4, variance=0.04 if n >= 256 else 0.08, K=2)   # (K: no part of rhs)
    B = 3 if n < 256 else 2
    y, p = _fields(cfg, B, seed=n + ifpad, hermitian=herm)
    env = pkg.PDEenv(setup, B=B, dtype=F32)
    out = _jul(env.rhs(to_dev(_mem(y), F32), to_dev(_mem(p), F32)))
    for b in range(B):
        ref = fluid.rhs(cfg, y[b].copy(), p[b])
        assert _rel(out[b], ref) <= 2e-6, (b, _rel(out[b], ref))


@pytest.mark.parametrize("n,B", [(256, 14), (512, 5)])
def test_rhs_f32_with_several_tiles(pkg, n, B):
    """many x-pass tiles per launch, ragged over the trajectories: every trajectory's right-hand side, <= 2e-6 relative"""
    from oracle import fluid
    setup, cfg = _pair(pkg, n, 1, spa=8, variance=0.04, K=2)
    y, p = _fields(cfg, B, seed=7 * n + B, hermitian=True)
    env = pkg.PDEenv(setup, B=B, dtype=F32)
    out = _jul(env.rhs(to_dev(_mem(y), F32), to_dev(_mem(p), F32)))
    for b in range(B):
        ref = fluid.rhs(cfg, y[b].copy(), p[b])
        assert _rel(out[b], ref) <= 2e-6, (b, _rel(out[b], ref))


# ---------------------------------------------------------------------------------------------------------- do_step


@pytest.mark.parametrize("n,ifpad", [(16, 1), (32, 1), (32, 0), (256, 1), (128, 0)])
def test_do_step_f32_matches_oracle(pkg, n, ifpad):
    """K RK4 sub-steps of the reference's size (FluidSetup.jl:163-172; the fused K3 + K1 stage kernels at n = 256): <= 5e-6
    relative, input untouched"""
    from oracle import fluid
    K = 3 if n < 128 else 2
    setup, cfg = _pair(pkg, n, ifpad, K=K, spa=8 if n >= 128 else 4, variance=0.04 if n >= 128 else 0.08, physical=True)
    B = 2
    y, p = _fields(cfg, B, seed=7)
    env = pkg.PDEenv(setup, B=B, dtype=F32)
    yin = to_dev(_mem(y), F32)
    out, flags = env.do_step(yin, to_dev(_mem(p), F32))
    assert np.abs(_jul(yin) - y).max() == 0.0
    for b in range(B):
        ref = fluid.do_step(cfg, y[b], p[b], K)
        assert _rel(_jul(out)[b], ref) <= 5e-6, (b, _rel(_jul(out)[b], ref))
    assert int(flags.sum()) == 0


# ---------------------------------------------------------------------------------------------------------- closures, env step


@pytest.mark.parametrize("n,spa,variance,K,B", [(128, 8, 0.08, 4, 3), (512, 8, 0.04, 2, 2)])
def test_closures_and_env_step_f32_match_oracle(pkg, n, spa, variance, K, B):
    """featurize at reset, prepare_action and the fused (env)(action) (src/PDEenv.jl:195-241) against the oracle's closures:
    state and reward <= 1e-5 relative (to max(1, |ref|)), spectrum <= 1e-5, forcing <= 1e-6; equal done flags"""
    from oracle import fluid
    setup, cfg = _pair(pkg, n, 1, spa=spa, K=K, variance=variance, physical=True)
    rng = np.random.default_rng(3)
    y, _ = _fields(cfg, B, seed=11)
    A = spa * spa
    a0 = rng.uniform(-1, 1, (B, 1, A)).astype(np.float32).astype(np.float64)
    a1 = rng.uniform(-1, 1, (B, 1, A)).astype(np.float32).astype(np.float64)
    env = pkg.PDEenv(setup, B=B, dtype=F32, y0=y)
    for b in range(B):
        st = fluid.featurize(cfg, y[b])
        assert np.abs(env.state[b].cpu().numpy().T - st).max() <= 1e-5 * max(1.0, np.abs(st).max())
    pa = _jul(env.prepare_action(to_dev(a1.reshape(B, -1, 1), F32)))
    for b in range(B):
        ref = fluid.prepare_action(cfg, a1[b])
        assert _rel(pa[b], ref) <= 1e-6
    env.action.copy_(to_dev(a0.reshape(B, -1, 1), F32))
    env(to_dev(a1.reshape(B, -1, 1), F32))
    done = env._done_flags.cpu().numpy()
    for b in range(B):
        p = fluid.prepare_action(cfg, a1[b])
        yn = fluid.do_step(cfg, y[b], p, K)
        assert _rel(_jul(env.y)[b], yn) <= 1e-5, (b, _rel(_jul(env.y)[b], yn))
        r = fluid.reward_function(cfg, yn, a1[b], a1[b] - a0[b])
        assert np.abs(env.reward[b].cpu().numpy() - r).max() <= 1e-5 * max(1.0, np.abs(r).max())
        st = fluid.featurize(cfg, yn)
        assert np.abs(env.state[b].cpu().numpy().T - st).max() <= 1e-5 * max(1.0, np.abs(st).max())
        assert bool(done[b]) == bool((np.abs(r) > setup.max_value).any())     # check_max_value = "reward"
    rr = env.reward_function().cpu().numpy()
    assert np.abs(rr - env.reward.cpu().numpy()).max() <= 1e-6 * max(1.0, np.abs(rr).max())


def test_reward_blowup_flag_f32(pkg):
    """a field scaled far past max_value raises the done flag of its trajectory only"""
    from oracle import fluid
    setup, cfg = _pair(pkg, 32, 1, spa=4, K=2)
    y, _ = _fields(cfg, 2, seed=5)
    y[1] *= 1e4
    env = pkg.PDEenv(setup, B=2, dtype=F32, y0=y)
    env(torch.zeros(env._ashape, dtype=F32, device="cuda:0"))
    assert env._done_flags.cpu().tolist() == [0, 1]


def test_device_initialiser_f32_matches_oracle_ic(pkg):
    """pdec_fluid_ic on an fp32 environment (the host vortex table stays double, rounded once): <= 1e-6 relative"""
    from oracle import fluid
    setup, cfg = _pair(pkg, 64, 1, spa=4, K=2)
    B = 3
    env = pkg.PDEenv(setup, B=B, dtype=F32)
    for case in (3, 4, 2, 1):
        v = setup.ic_vortices(case, np.random.default_rng(7), B)
        rng = np.random.default_rng(7)
        refs = [fluid.ic(cfg, case, rng) for _ in range(B)]
        out = torch.empty_like(env.y)
        pkg._lib.check(env.lib.pdec_fluid_ic(env.handle, v.ctypes.data_as(C.POINTER(C.c_double)), v.shape[1], pkg._lib.ptr(out)))
        got = _jul(out)
        for b in range(B):
            assert _rel(got[b], refs[b]) <= 1e-6, (case, b, _rel(got[b], refs[b]))
    y0 = setup.random_init_device(env, np.random.default_rng(3))
    assert y0.shape == env.y.shape and y0.dtype == F32 and bool(torch.isfinite(y0).all())
    env.set_y0(refs[0])                                   # complex128 host array -> rounded
    env.reset()
    assert _rel(_jul(env.y)[0], refs[0]) <= 1e-7


# ---------------------------------------------------------------------------------------------------------- trajectories


def test_trajectory_drift_f32_against_f64(pkg):
    """51 control steps at the Fluid_8 geometry (128 x 128, 8 x 8 sensors, K = 40) under one fixed action sequence: the
    fp32 environment against the fp64 one on the GPU, physical field real(ifft2(y)) <= 5e-5 relative"""
    from oracle import fluid
    setup, cfg = _pair(pkg, 128, 1, spa=8, variance=0.08)
    assert setup.oversampling == 40
    y0 = fluid.ic(cfg, 3, np.random.default_rng(5)).astype(np.complex64).astype(np.complex128)
    acts = np.random.default_rng(9).uniform(-1, 1, (51, 1, 64, 1)).astype(np.float32)
    envs = {dt: pkg.PDEenv(setup, B=1, dtype=dt, y0=y0[None]) for dt in (F32, F64)}
    for k in range(51):
        for dt, env in envs.items():
            env(to_dev(acts[k], dt))
    phys = {dt: np.real(np.fft.ifft2(_jul(env.y)[0])) for dt, env in envs.items()}
    err = np.abs(phys[F32] - phys[F64]).max() / np.abs(phys[F64]).max()
    assert err <= 5e-5, err
    assert np.abs(phys[F64]).max() > 0.1 * np.abs(np.real(np.fft.ifft2(y0))).max()     # the field is still alive


def test_batch_independence_f32(pkg):
    """every trajectory of a B = 16, 512^2 fp32 step (two part-batch children, many x-pass tiles) equals the same initial
    condition stepped in a B = 2 environment, bit for bit"""
    from oracle import fluid
    setup, cfg = _pair(pkg, 512, 1, spa=8, K=2, variance=0.04)
    rng = np.random.default_rng(21)
    base = [fluid.ic(cfg, 3, rng) for _ in range(2)]
    y = np.stack([base[b % 2] * (1.0 + 0.01 * b) for b in range(16)])
    act = rng.uniform(-1, 1, (16, 64, 1))
    big = pkg.PDEenv(setup, B=16, dtype=F32, y0=y)
    assert big.n_part_streams >= 1
    big(to_dev(act, F32))
    for b0 in (0, 6, 13):
        small = pkg.PDEenv(setup, B=2, dtype=F32, y0=y[b0:b0 + 2])
        small(to_dev(act[b0:b0 + 2], F32))
        assert torch.equal(small.y, big.y[b0:b0 + 2]), b0
        assert torch.equal(small.state, big.state[b0:b0 + 2]) and torch.equal(small.reward, big.reward[b0:b0 + 2])
        small.close()


def test_error_detection_f32_and_f64_agree(pkg):
    """FluidSetup.error_detection on the environment's own (re, im) layout, fp32 and fp64 copies of a blown-up and of a
    healthy field give the same answer"""
    setup = pkg.FluidSetup.Fluid_8(nx=32)
    rng = np.random.default_rng(3)
    healthy = np.fft.fft2(rng.standard_normal((32, 32)))
    w = np.zeros((32, 32))
    w[5, :] = 10.5
    blown = np.fft.fft2(w)
    for yhat, want in ((healthy, False), (blown, True)):
        mem = _mem(yhat[None])
        for dt in (F32, F64):
            assert setup.error_detection(to_dev(mem, dt)) == want, (dt, want)
            assert setup.error_detection(torch.as_tensor(mem, dtype=dt)) == want


def test_fluid8_rollout_f32_follows_the_step_loop(pkg):
    """the reference-trained Fluid_8 actor driven by env.rollout (one library call) and by the policy/step loop on fp32
    environments: the same actions and spectra to fp32 rounding"""
    from util import load_golden
    from oracle import fluid
    g = load_golden("fluid8_hook.npz")
    best = [g["best_W1"], g["best_b1"], g["best_W2"], g["best_b2"]]
    setup, cfg = _pair(pkg, 128, 1, spa=8, variance=0.08)
    y0 = fluid.ic(cfg, 3, np.random.default_rng(5))
    agent = pkg.create_agent(setup=setup, B=1, rng=np.random.default_rng(0), dtype=F32)
    pkg.checkpoint.load_actor(agent.policy.behavior_actor, best)
    agent.policy.start_steps = -1
    env1 = pkg.PDEenv(setup, B=1, dtype=F32, y0=y0[None])
    ys, acts = [], []
    for _ in range(3):
        env1(agent.policy(env1, learning=False))
        ys.append(env1.y.clone())
        acts.append(env1.action.clone())
    env2 = pkg.PDEenv(setup, B=1, dtype=F32, y0=y0[None])
    out = env2.rollout(agent.policy._actor_for(F32, 1), 3, log=True)
    torch.cuda.synchronize()
    for k in range(3):
        assert torch.allclose(out["action"][k], acts[k], rtol=0, atol=1e-5)
        assert _rel(_jul(out["y"][k]), _jul(ys[k])) <= 1e-5
    assert bool(torch.isfinite(out["y"]).all())


def test_device_episodes_f32_equal_the_stage_loop(pkg):
    """run() at B = 1 on an fp32 fluid environment: whole episodes issued on the device (device_episodes=True) leave the same
    replay buffer, step counters and networks as the stage loop (device_episodes=False), bit for bit"""
    import importlib
    run_mod = importlib.import_module(pkg.__name__ + ".run")
    out = []
    for dev in (True, False):
        setup = pkg.FluidSetup(nx=64)
        s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
        env = pkg.PDEenv(setup, B=1, dtype=F32, stream=s_env)
        agent = pkg.create_agent(setup=setup, B=1, rng=np.random.default_rng(7), noise_seed=7, stream=s_upd)
        hook = pkg.PDEhook(min_best_episode=1, use_random_init=True, init_seed=7)
        agent.policy.act_noise = setup.act_noise
        stop = pkg.StopAfterEpisodeWithMinSteps(700)
        assert run_mod.device_episodes_ok(agent, env, stop, hook)
        pkg.run(agent, env, stop, hook, device_episodes=dev)
        torch.cuda.synchronize()
        out.append((env, agent, hook))
    (ed, ad, hd), (es, as_, hs) = out
    pd, ps, td, ts = ad.policy, as_.policy, ad.trajectory, as_.trajectory
    assert len(hd.rewards) == len(hs.rewards) >= 2 and hd.rewards == hs.rewards
    assert (td.n_sa, td.n_rt, pd.update_step) == (ts.n_sa, ts.n_rt, ps.update_step)
    for name in ("state", "action", "reward", "terminal"):
        assert torch.equal(getattr(td, name), getattr(ts, name)), name
    assert torch.equal(ed.y, es.y) and ed.y.dtype == F32
    for n in ("behavior_actor", "behavior_critic"):
        for x, y in zip(getattr(pd, n).model.params(), getattr(ps, n).model.params()):
            assert np.array_equal(x, y), n


# ---------------------------------------------------------------------------------------------------------- learning


_FLUID8_BAND = lambda r: (-14.0 <= r[0] <= -3.0, -3.2 <= r[2:6].mean() <= -1.2, -1.6 <= r[-8:].mean() <= -0.35,
                          r.max() >= -0.95)     # tests/test_gpu_training.py, test_fluid_learning_curves_need_moving_targets


def _curves(pkg, setup, seeds, frozen, loops, no_steps, decay, dtype):
    """_curves of tests/test_gpu_training.py with the environment's dtype as a parameter"""
    out = []
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    for seed in seeds:
        env = pkg.PDEenv(setup, B=1, dtype=dtype, stream=s_env)
        agent = pkg.create_agent(setup=setup, B=1, rng=np.random.default_rng(100 + seed), noise_seed=1000 + seed, stream=s_upd,
                                 quirk_frozen_targets=frozen)
        hook = pkg.PDEhook(min_best_episode=1, use_random_init=True, init_seed=2000 + seed, init_rng=np.random.default_rng(seed))
        train(pkg, agent, env, hook, loops=loops, no_steps=no_steps, decay=decay)
        torch.cuda.synchronize()
        out.append((np.asarray(hook.rewards), hook.bestreward))
    return out


@pytest.mark.slow
def test_fluid8_learning_curve_with_an_fp32_environment(pkg):
    """the Fluid_8 training (train(; loops = 10), moving targets) on an fp32 environment lands in the bands of the fp64
    test in at least 2 of 3 seeds"""
    runs = _curves(pkg, pkg.FluidSetup.Fluid_8(), range(3), False, 10, 580, 0.6, F32)
    assert all(len(r) == 20 for r, _ in runs)
    assert sum(all(_FLUID8_BAND(r)) for r, _ in runs) >= 2, [np.round(r, 2) for r, _ in runs]
