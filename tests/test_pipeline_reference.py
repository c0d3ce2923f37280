"""The teacher-forced reference of TrainPipeline's control step (tests/pipeline_ref.py) tells a right pipeline from a wrong
one: it accepts the trace of a NumPy restatement of the pipeline (rings, episode boundaries, lag, fp32 arithmetic) at a
small shape, and rejects each of a list of plausible wiring bugs built into that restatement, with a message that names
the broken check.  Host only (no GPU)."""
import numpy as np
import pytest

from oracle import keller_segel2d as k2
from oracle import ks, nn
from oracle import rng as orng
from pipeline_ref import Config, KSEnv, KSeg2DEnv, Rec, Trace, check_trace, n_updates, schedule
from small_update_ref import fresh_snap
from test_small_update_reference import GAMMA, RHO, fp32_launch

NX, B, E, LAG, N = 64, 4, 5, 2, 12          # two episode boundaries (steps 5 and 10)
SEED, NOISE, LIMIT = 99, 0.3, 1.0
ETA_A, ETA_C = 5e-4, 1e-3


def _env():
    Lx = NX * (200.0 / 240.0)                # KSSetup.bench_C2's geometry at nx = 64: 16 actuators, window 3
    return KSEnv(ks.KSConfig(NX, Lx, np.arange(1, NX + 1, 4), window_size=3), B)


def _env2d():
    """the C4 shape at 32 x 32 cells: 6 x 6 sensors, 2 x 2 actuators, temporal stack of 2 (36 state rows)"""
    return KSeg2DEnv(k2.KSeg2DConfig(nx=32, ny=32, Lx=3.2, sensor_x=np.arange(3, 33, 5), sensor_y=np.arange(3, 33, 5)), B)


def _cfg(env, rho=1.0, quirk=True, random_init=None, ns=3, scales=(1.6, 7.0), drop=False):
    da, aa = nn.layer_sizes(ns, 1, scales[0], True, drop)
    dc, ac = nn.layer_sizes(ns, 1, scales[1], False, drop)
    return Config(cols=B * env.A, ns=ns, na=1, lag=LAG, E=E, noise_seed=SEED, act_noise=NOISE, act_limit=LIMIT, gamma=GAMMA,
                  rho=rho, quirk=quirk, eta_a=ETA_A, eta_c=ETA_C, acts_a=aa, acts_c=ac, env=env,
                  random_init=random_init), da, dc


def _nets(da, dc):
    rng = np.random.default_rng(1)
    A, C = nn.glorot_uniform(rng, da), nn.glorot_uniform(rng, dc)
    return fresh_snap(A, C, [p.copy() for p in A], [p.copy() for p in C])


def simulate(cfg, da, dc, fault=None, y0=None):
    """the pipeline restated: act_k (actor after update_{k-1}, device noise counter), env_k (oracle step in fp64, stored
    in fp32), update_k on the ring slots of step k - LAG -- s' read from the state ring, which the next episode's first
    step overwrites with featurize(y0) as the device does -- as one fp32 oracle update.  `fault`: one bug built in."""
    f32 = np.float32
    env, cols = cfg.env, cfg.cols
    cfg0 = env.cfg
    if y0 is None:
        y0 = np.stack([ks.generate_random_init(cfg0, np.random.default_rng(b)) for b in range(B)]) * 0.15
    st = _nets(da, dc)
    ctr = 1000
    trace = Trace(Rec(st.copy(), ctr))
    if cfg.random_init is None:
        trace.resets[0] = y0.astype(f32).astype(np.float64)
    sring, aring, rring, tring = {}, {}, {}, {}
    A_before_last = st.A
    y_ep, draws = y0, 0
    for k, (first, last, first_tick, _s) in enumerate(schedule(cfg, trace, N)):
        prev = trace.steps[-1] if trace.steps else None
        if first:
            if cfg.random_init is not None:
                y_ep = env.random_init(cfg.random_init[0], draws * cfg.random_init[1])
                draws += 1
            y_in = prev.y_out if (fault == "first_step_from_y" and k > 0) else y_ep.astype(f32)
            s_in = env.featurize(y_ep.astype(f32)).astype(f32)
            a_prev = prev.a if (fault == "action_prev_not_zeroed" and k > 0) else np.zeros((cols, 1), f32)
        else:
            y_in, s_in, a_prev = prev.y_out, prev.s_out, prev.a
        sring[k] = s_in
        # act_k
        Aact = A_before_last if fault == "act_with_stale_actor" else st.A
        noise = orng.randn(cfg.noise_seed, ctr, cols).reshape(cols, 1).astype(f32)
        a = np.clip(nn.forward(Aact, cfg.acts_a, s_in.T).T + f32(NOISE) * noise, -LIMIT, LIMIT).astype(f32)
        if not (fault == "noise_offset_reused" and k == 3):
            ctr += (cols + 3) // 4
        # env_k
        o = env.step(y_in.astype(np.float64), a_prev, a, s_in)
        flags = o["done"].astype(np.int32)
        t = np.repeat(np.ones(B) if (last and fault != "term_missing_at_end") else flags, env.A).astype(f32)
        aring[k], rring[k], tring[k] = a, o["reward"].astype(f32), t
        sring[k + 1] = o["state"].astype(f32)
        # update_k on transition j = k - LAG
        A_before_last = st.A
        j = k - LAG
        if j >= first_tick:
            jj = j + 1 if fault == "update_on_next_transition" else (max(0, j - 1) if fault == "update_on_previous_transition" else j)
            s, sn = sring[jj], sring[jj + 1]
            if fault == "s_as_s_next":
                sn = s
            r = rring[jj]
            if fault == "rbar_from_wrong_step":
                r = r - r.mean() + rring[max(0, jj - 1) if jj > 0 else jj + 1].mean()
            mb = (s.T, aring[jj].T, r, tring[jj], sn.T)
            launch_fault = {"polyak_under_frozen_targets": "polyak_at_rho_1",
                            "actor_through_pre_update_critic": "actor_through_pre_update_critic"}.get(fault)
            st = fp32_launch(st, [mb], cfg.acts_a, cfg.acts_c, cfg.rho, cfg.quirk, ETA_A, ETA_C, fault=launch_fault)
        trace.steps.append(Rec(st.copy(), ctr, y_in=np.asarray(y_in, f32), y_out=o["y"].astype(f32), s_in=s_in,
                               s_out=sring[k + 1], a=a, r=rring[k], t=t, flags=flags))
    return trace


@pytest.mark.parametrize("rho,quirk,random_init", [(1.0, True, False), (RHO, True, False), (1.0, False, True)])
def test_checks_accept_the_restated_pipeline(rho, quirk, random_init):
    env = _env()
    cfg, da, dc = _cfg(env, rho, quirk, (7, B * 2) if random_init else None)
    trace = simulate(cfg, da, dc)
    errs, worst = check_trace(cfg, trace)
    assert errs == []
    assert n_updates(cfg, trace, N) == N - LAG
    assert worst["act"] < 1 and worst["critic gradient"] < 1 and worst["env y"] < 1


def test_checks_accept_the_restated_c4_pipeline():
    """the 2-D Keller-Segel shape of C4: 2-layer nets, a temporal state stack, u / v interleaved per cell"""
    env = _env2d()
    cfg, da, dc = _cfg(env, ns=36, scales=(2.0, 17.0), drop=True)
    rng = np.random.default_rng(4)
    y0 = np.moveaxis(1.0 + 0.05 * rng.standard_normal((B, 2, 32, 32)), 1, -1)
    errs, worst = check_trace(cfg, simulate(cfg, da, dc, y0=y0))
    assert errs == []
    assert worst["act"] < 1 and worst["critic gradient"] < 1 and worst["env state"] < 1


def test_kseg2d_env_is_the_oracle_per_trajectory():
    """KSeg2DEnv batches oracle/keller_segel2d.py over a trailing axis: the same numbers as one trajectory at a time"""
    env = _env2d()
    cfg = env.cfg
    rng = np.random.default_rng(5)
    y = 1.0 + 0.05 * rng.standard_normal((B, 2, 32, 32))
    a, ap = rng.uniform(-1, 1, (B * env.A, 1)), rng.uniform(-1, 1, (B * env.A, 1))
    s_prev = env.featurize(np.moveaxis(y, 1, -1))
    o = env.step(np.moveaxis(y, 1, -1), ap, a, s_prev)
    for b in range(B):
        ab, apb = a[b * env.A:(b + 1) * env.A].T, ap[b * env.A:(b + 1) * env.A].T
        ref = k2.do_step(cfg, y[b], k2.prepare_action(cfg, ab))
        assert np.abs(np.moveaxis(o["y"][b], -1, 0) - ref).max() <= 1e-12
        assert np.abs(o["reward"][b * env.A:(b + 1) * env.A] - k2.reward_function(cfg, ref, ab, ab - apb)).max() <= 1e-12
        st = k2.featurize(cfg, ref, k2.featurize(cfg, y[b], None))
        assert np.abs(o["state"][b * env.A:(b + 1) * env.A].T - st).max() <= 1e-12


# fault -> the check that must name it
FAULTS = [
    ("act_with_stale_actor", "act ("),
    ("noise_offset_reused", "noise counter"),
    ("update_on_next_transition", "update ("),
    ("update_on_previous_transition", "update ("),
    ("s_as_s_next", "update ("),
    ("term_missing_at_end", "env term"),
    ("rbar_from_wrong_step", "critic: gradient"),
    ("polyak_under_frozen_targets", "target actor: frozen target"),
    ("actor_through_pre_update_critic", "actor: gradient"),
    ("first_step_from_y", "env y_in"),
    ("action_prev_not_zeroed", "env reward"),
]


@pytest.mark.parametrize("fault,check", FAULTS)
def test_checks_reject_a_faulty_pipeline(fault, check):
    env = _env()
    cfg, da, dc = _cfg(env)
    errs, _ = check_trace(cfg, simulate(cfg, da, dc, fault))
    assert errs, fault
    assert any(check in e for e in errs), (fault, errs[:5])
