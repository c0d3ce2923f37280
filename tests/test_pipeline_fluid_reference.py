"""The fluid env oracle of the teacher-forced pipeline reference (tests/pipeline_fluid_ref.py) tells a right fluid pipeline from a
wrong one: check_trace accepts a NumPy restatement of the fluid pipeline at n = 32, B = 3 (16 actuators, 9 state rows, 2-layer
nets, terminal rows expanded from the per-trajectory flags, device-rule random fields) and rejects three wiring bugs of the kind
the fluid's new pipeline code could have, naming the broken check.  Host only (no GPU)."""
import numpy as np
import pytest

from fluid_ic_ref import mem
from oracle import fluid, nn
from oracle import rng as orng
from pipeline_fluid_ref import FluidEnvRef
from pipeline_ref import Config, Rec, Trace, check_trace, n_updates, schedule
from small_update_ref import fresh_snap
from test_small_update_reference import GAMMA, fp32_launch

NX, B, E, LAG, N = 32, 3, 3, 2, 7           # two episode boundaries (steps 3 and 6)
SEED, NOISE, LIMIT = 99, 0.3, 1.0
ETA_A, ETA_C = 5e-4, 1e-3
SCALED = 1


def _env(max_value=0.5):
    cfg = fluid.FluidConfig(nx=NX, sensors_per_axis=4, variance=0.08, oversampling=2, dt=2.0 / (16.0 * NX), max_value=max_value)
    return FluidEnvRef(cfg, B)


def _cfg(env, random_init=None):
    da, aa = nn.layer_sizes(9, 1, 1.8, True, True)
    dc, ac = nn.layer_sizes(9, 1, 17.0, False, True)
    return Config(cols=B * env.A, ns=9, na=1, lag=LAG, E=E, noise_seed=SEED, act_noise=NOISE, act_limit=LIMIT, gamma=GAMMA,
                  rho=1.0, quirk=True, eta_a=ETA_A, eta_c=ETA_C, acts_a=aa, acts_c=ac, env=env, random_init=random_init), da, dc


def simulate(cfg, da, dc, fault=None):
    """the fluid pipeline restated (tests/test_pipeline_reference.py::simulate with the fluid's terminal rows and draw)"""
    f32 = np.float32
    env, cols = cfg.env, cfg.cols
    rng = np.random.default_rng(1)
    A, C = nn.glorot_uniform(rng, da), nn.glorot_uniform(rng, dc)
    st = fresh_snap(A, C, [p.copy() for p in A], [p.copy() for p in C])
    ctr = 1000
    trace = Trace(Rec(st.copy(), ctr))
    y_ep = env.random_init(3, 0)
    # one trajectory past max_value = 0.5 at every step (oracle: max |reward| 0.99 .. 0.68 over eight steps against <= 0.08 of the
    # others) that stays finite; x 30, the factor of the one-step tests, overflows the integrator at its second step
    y_ep[SCALED] *= 10.0
    if cfg.random_init is None:
        trace.resets[0] = y_ep.astype(f32).astype(np.float64)
    sring, aring, rring, tring = {}, {}, {}, {}
    draws = 0
    for k, (first, last, first_tick, _s) in enumerate(schedule(cfg, trace, N)):
        prev = trace.steps[-1] if trace.steps else None
        if first:
            if cfg.random_init is not None and not (fault == "keeps_old_field" and k > 0):
                y_ep = env.random_init(cfg.random_init[0], draws * cfg.random_init[1])
            draws += 1
            y_in = y_ep.astype(f32)
            s_in = env.featurize(y_in).astype(f32)
            a_prev = np.zeros((cols, 1), f32)
        else:
            y_in, s_in, a_prev = prev.y_out, prev.s_out, prev.a
        sring[k] = s_in
        noise = orng.randn(cfg.noise_seed, ctr, cols).reshape(cols, 1).astype(f32)
        a = np.clip(nn.forward(st.A, cfg.acts_a, s_in.T).T + f32(NOISE) * noise, -LIMIT, LIMIT).astype(f32)
        ctr += (cols + 3) // 4
        o = env.step(y_in.astype(np.float64), a_prev, a, s_in)
        flags = o["done"].astype(np.int32)
        rows = flags
        if fault == "rows_from_next_trajectory":
            rows = np.roll(flags, -1)
        if fault == "rows_zero_at_blowup":
            rows = np.zeros_like(flags)
        t = np.repeat(np.ones(B) if last else rows, env.A).astype(f32)
        aring[k], rring[k], tring[k] = a, o["reward"].astype(f32), t
        sring[k + 1] = o["state"].astype(f32)
        j = k - LAG
        if j >= first_tick:
            mb = (sring[j].T, aring[j].T, rring[j], tring[j], sring[j + 1].T)
            st = fp32_launch(st, [mb], cfg.acts_a, cfg.acts_c, cfg.rho, cfg.quirk, ETA_A, ETA_C)
        trace.steps.append(Rec(st.copy(), ctr, y_in=np.asarray(y_in, f32), y_out=o["y"].astype(f32), s_in=s_in,
                               s_out=sring[k + 1], a=a, r=rring[k], t=t, flags=flags))
    return trace


def test_checks_accept_the_restated_fluid_pipeline():
    env = _env()
    cfg, da, dc = _cfg(env)
    trace = simulate(cfg, da, dc)
    errs, worst = check_trace(cfg, trace)
    assert errs == [], errs[:5]
    assert n_updates(cfg, trace, N) == N - LAG
    assert worst["act"] < 1 and worst["env y"] < 1 and worst["env reward"] < 1
    # the scaled trajectory, and only it, is flagged at every step
    assert all(s.flags.tolist() == [0, 1, 0] for s in trace.steps)


def test_checks_accept_the_device_rule_draws():
    env = _env(max_value=3.0)
    cfg, da, dc = _cfg(env, random_init=(5, B * 30))
    errs, _ = check_trace(cfg, simulate(cfg, da, dc))
    assert errs == [], errs[:5]


def test_env_ref_is_the_oracle_in_the_device_layout():
    env = _env()
    y = env.random_init(3, 0)
    assert y.shape == (B, NX, NX, 2)
    rng = np.random.default_rng(2)
    a, ap = rng.uniform(-1, 1, (B * env.A, 1)), rng.uniform(-1, 1, (B * env.A, 1))
    o = env.step(y, ap, a)
    yj = np.swapaxes(y[..., 0] + 1j * y[..., 1], -1, -2)
    for b in range(B):
        ab, apb = a[b * env.A:(b + 1) * env.A].T, ap[b * env.A:(b + 1) * env.A].T
        ref = fluid.do_step(env.cfg, yj[b], fluid.prepare_action(env.cfg, ab), 2)
        assert np.array_equal(o["y"][b], mem(ref))
        assert np.array_equal(o["reward"][b * env.A:(b + 1) * env.A], fluid.reward_function(env.cfg, ref, ab, ab - apb))
        assert np.array_equal(o["state"][b * env.A:(b + 1) * env.A].T, fluid.featurize(env.cfg, ref))
    assert np.array_equal(env.featurize(y)[:env.A].T, fluid.featurize(env.cfg, yj[0]))


FAULTS = [
    ("rows_from_next_trajectory", "env term", None),
    ("rows_zero_at_blowup", "env term", None),
    ("keeps_old_field", "env y_in", (5, B * 30)),
]


@pytest.mark.parametrize("fault,check,random_init", FAULTS)
def test_checks_reject_a_faulty_fluid_pipeline(fault, check, random_init):
    env = _env()
    cfg, da, dc = _cfg(env, random_init=random_init)
    errs, _ = check_trace(cfg, simulate(cfg, da, dc, fault))
    assert errs, fault
    assert any(check in e for e in errs), (fault, errs[:5])
