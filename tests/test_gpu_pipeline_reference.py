"""TrainPipeline's control step against the teacher-forced fp64 reference of tests/pipeline_ref.py, in the configurations
the benchmark and users run: every step of a ~20-step run over at least two episode boundaries (act_k, env_k, update_k
each judged from the state the device had before the step), then the same run issued the way it is timed -- no
per-step synchronisation, recorded steps, graphs where the episodes allow them -- which must end bit-identical to the
checked run.  Also: the device's normals are oracle.rng.randn's."""
import warnings

import numpy as np
import pytest
import torch

from oracle import rng as orng
from pipeline_ref import (KSEnv, KSeg2DEnv, check_trace, config_of, ks_config, kseg2d_config, n_updates, noise_counter,
                          record_step, run_teacher_forced)

pytestmark = pytest.mark.gpu

N, E = 20, 7          # steps 0-6, 7-13, 14-19: two episode boundaries


def _make(pkg, B=64, E=E, lag=2, serial=False, replay_steps=0, use_graphs=False, setup_kw=None, agent_kw=None, c4=False,
          **kw):
    s_env = torch.cuda.Stream()
    s_upd = s_env if serial else torch.cuda.Stream()
    if c4:
        # C4's pipeline (bench.py, bench_aux) at a reduced grid: 2-D Keller-Segel, 2-layer nets, the setup's random field
        setup = pkg.KellerSegel2DSetup(nx=64, ny=64, **(setup_kw or {}))
        y0 = np.ascontiguousarray(np.moveaxis(setup.generate_random_init(np.random.default_rng(0), B), 1, -1))
    else:
        setup = pkg.KSSetup.bench_C2(256, **(setup_kw or {}))
        y0 = setup.generate_random_init(np.random.default_rng(0), B) * 0.15
    env = pkg.PDEenv(setup, B=B, dtype=torch.float32, y0=y0, stream=s_env, autoreset=False)
    if env.n_part_streams:
        env.set_part_streams([torch.cuda.Stream() for _ in range(env.n_part_streams)])
    cols = B * setup.n_actuators
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")            # (moving targets: the setup's TargetNetworkWarning)
        agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd,
                                 start_steps=-1, noise_seed=7,
                                 trajectory_length=(replay_steps * cols // B if replay_steps else 1), **(agent_kw or {}))
    agent.policy.act_noise = 0.3
    torch.cuda.synchronize()
    return pkg.TrainPipeline(env, agent, lag=lag, episode_steps=E, stream_env=s_env, stream_upd=s_upd, use_graphs=use_graphs,
                             chunks=(6, 1), noise_seed=99, use_replay=bool(replay_steps), **kw)


def _resets(pipe, spec):
    """tick -> the field reset_from() gets there (a fresh random field, scaled like the others)"""
    out = {}
    for k, seed in (spec or {}).items():
        y = pipe.env.setup.generate_random_init(np.random.default_rng(seed), pipe.env.B) * 0.15
        out[k] = torch.as_tensor(y, dtype=pipe.env.dtype, device=pipe.env.device)
    torch.cuda.synchronize()
    return out


def _unsynced(pkg, n, resets_spec, make_kw):
    """the same run issued as it is timed: no synchronisation between steps, recorded steps (and graphs, where eligible)"""
    p = _make(pkg, **make_kw)
    resets = _resets(p, resets_spec)
    for k in sorted(resets):
        p.run(k - p.tick)
        p.reset_from(resets[k])
    p.run(n - p.tick)
    p.sync()
    return p


def _same_as(pkg, rec, pipe, k):
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
    print(f"\n[pipeline reference] {case}: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))


CASES = {
    "c2_default": dict(),
    "lag1": dict(lag=1),
    "serial": dict(serial=True),
    "moving_targets": dict(agent_kw=dict(quirk_frozen_targets=False)),
    "diagonal_target": dict(agent_kw=dict(quirk_target_broadcast=False)),
    "reward_groups": dict(B=63, agent_kw=dict(target_broadcast_group=3)),        # Bu % (g L) == 0: 63 x 64 columns
    "two_layer": dict(setup_kw=dict(drop_middle_layer=True)),
    "random_init": dict(random_init=True, init_seed=5, log_episodes=4),
    "replay": dict(replay_steps=8),
    "reset_mid_episode": dict(_resets={10: 3}),
    "c4_kseg2d": dict(c4=True, B=16),              # 16 x 16 actuators of a 64 x 64 grid: 256 columns, 36 state rows
}


def _env_ref(p):
    if getattr(p.env.setup, "is_kseg2d", False):
        return KSeg2DEnv(kseg2d_config(p.env.setup), p.env.B)
    return KSEnv(ks_config(p.env.setup), p.env.B)


def _run_case(pkg, case, make_kw, n=N):
    make_kw = dict(make_kw)
    resets_spec = make_kw.pop("_resets", None)
    p = _make(pkg, **make_kw)
    if case == "c2_default":
        # the route the bench times: reward partials from the fused env step, stop events, env kicked behind the critic
        assert p.rpart is not None and p.stop_events and p.kick_env_after_critic and not p.serial
    if case == "serial":
        assert p.serial
    if case == "two_layer":
        assert p.act_in_place
    if case == "reward_groups":
        assert p.policy.reward_group == 3 and p.reward_interleave == p.env.setup.n_actuators
    if case == "c4_kseg2d":
        assert p.act_in_place and len(p.actor.acts) == 2 and p.ns == 36
    cfg = config_of(p, _env_ref(p))
    trace = run_teacher_forced(pkg, p, n, _resets(p, resets_spec))
    errs, worst = check_trace(cfg, trace)
    _report(case, worst)
    assert errs == [], errs[:10]
    # the number of updates: one ADAM step per update on each behaviour net (beta powers advance once per update)
    nu = n_updates(cfg, trace, n)
    assert np.allclose(trace.steps[-1].snap.bpA, trace.init.snap.bpA * np.array([0.9, 0.999]) ** nu, rtol=1e-12)
    if case == "random_init":
        per = cfg.random_init[1]
        assert p.init_offsets == [0, per, 2 * per]          # episodes 0, 1, 2 each drew a field
    if case == "reset_mid_episode":
        assert nu == n - cfg.lag - cfg.lag          # transitions 8 and 9 are cut off by the restart at step 10
    else:
        assert nu == n - cfg.lag
    q = _unsynced(pkg, n, resets_spec, make_kw)
    _same_as(pkg, trace.steps[-1], q, n - 1)
    p.close()
    q.close()
    return trace


@pytest.mark.parametrize("case", list(CASES))
def test_pipeline_step_matches_the_reference(pkg, case):
    _run_case(pkg, case, CASES[case])


def test_graph_replay_of_the_checked_run(pkg):
    """the default C2 route with episodes long enough for graphs (E = 14 > two ring periods): the captured run ends where
    the teacher-forced, checked run does.  capture() itself issues the chunks it records (six ring phases of chunks 6 and
    1, with eager steps between them to reach each phase): 90 steps here, then 8 more through run(), which replays graphs;
    the checked run covers all of them (98 steps)."""
    q = _make(pkg, E=14, use_graphs=True)
    q.run(3)
    q.capture()
    n = q.tick + 8
    launched = q.n_graph_launches
    q.run(n - q.tick)
    q.sync()
    assert q.n_graph_launches > launched           # run() replayed at least one captured chunk
    p = _make(pkg, E=14)
    cfg = config_of(p, _env_ref(p))
    trace = run_teacher_forced(pkg, p, n)
    errs, worst = check_trace(cfg, trace)
    _report(f"c2_default, E = 14, {n} steps", worst)
    assert errs == [], errs[:10]
    _same_as(pkg, trace.steps[-1], q, n - 1)
    p.close()
    q.close()


@pytest.mark.slow
def test_full_size_c2_matches_the_reference(pkg):
    """B = 512 (32 768 update columns), four steps across one episode boundary"""
    p = _make(pkg, B=512, E=3)
    assert p.rpart is not None
    cfg = config_of(p, _env_ref(p))
    trace = run_teacher_forced(pkg, p, 4)
    errs, worst = check_trace(cfg, trace)
    _report("c2_full_size", worst)
    assert errs == [], errs[:10]
    assert n_updates(cfg, trace, 4) == 2
    p.close()


def test_device_normals_are_the_oracle_stream(pkg):
    """pdec_randn (fp32 and fp64) and the pipeline's acting kernel draw oracle.rng.randn's numbers at a nonzero offset:
    the moments test of test_gpu_mlp.py cannot see a shifted or permuted stream"""
    L = pkg._lib
    p = _make(pkg, B=4)
    lib, h = p.lib, p.actor.handle
    n, seed, off = 4099, 1234, 777                    # (n not a multiple of 4: the tail of the last counter)
    ref = orng.randn(seed, off, n)
    x64 = torch.empty(n, dtype=torch.float64, device="cuda:0")
    x32 = torch.empty(n, dtype=torch.float32, device="cuda:0")
    L.check(lib.pdec_randn(h, L.ptr(x64), n, L.PDEC_F64, seed, off))
    L.check(lib.pdec_randn(h, L.ptr(x32), n, L.dtype_code(torch.float32), seed, off))
    torch.cuda.synchronize()
    g64, g32 = x64.cpu().numpy(), x32.cpu().numpy()
    assert np.abs(g64 - ref).max() <= 1e-13 * np.abs(ref).max()
    assert np.all(np.abs(g32 - ref) <= np.spacing(np.abs(ref).astype(np.float32)))       # fp32 rounding of the fp64 value
    # the acting kernel: a fresh actor (zero biases) acts tanh(0) = 0 on zero states, so the action is the noise itself
    assert all(not b.any() for b in p.actor.params()[1::2])
    ctr0 = 4242
    L.check(lib.pdec_noise_counter_set(h, ctr0))
    cols = p.cols
    s = torch.zeros((cols, p.ns), dtype=torch.float32, device="cuda:0")
    out = torch.empty((cols, p.na), dtype=torch.float32, device="cuda:0")
    with torch.cuda.stream(p.s_env):
        L.check(lib.pdec_set_stream(h, p._sp_env))
        L.check(lib.pdec_policy_act_rng_dev(h, L.ptr(s), cols, 0.25, 1e6, 1, seed, L.ptr(out)))
        L.check(lib.pdec_set_stream(h, p._sp_upd))
    torch.cuda.synchronize()
    want = 0.25 * orng.randn(seed, ctr0, cols * p.na).reshape(cols, p.na)
    assert np.abs(out.cpu().numpy() - want).max() <= 2 * np.spacing(np.float32(np.abs(want).max()))
    assert noise_counter(p) == ctr0 + (cols * p.na + 3) // 4
    p.close()
