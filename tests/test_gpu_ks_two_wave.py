"""The fused fp32 N = 256 KS step over two waves per trajectory pair (pdec_env_set_two_wave_step, FftWave256x2) against the
one-wave step from the same seeded state and actions: BYTE-equal field, forcing, observation, reward, blow-up flags, per-column
terminal flags and per-workgroup reward partials after every control step.  The engine runs each radix-4 butterfly of the
one-wave engine as its two radix-2 levels with the twiddles where they were, and the step's sums stay on one wave, so there is
no tolerance.  B = 1 (a trajectory alone in its workgroup), 2, 3 (the last workgroup half empty) and 64; 1 and 51 steps with
an episode reset on the way; a trajectory that blows up (and restarts in the same step); actions at the clamp."""
import ctypes as C

import numpy as np
import pytest

from util import to_dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NAMES = ("y", "p", "state", "reward", "flags", "terminal", "partials")


def bits(t):
    return t.contiguous().view(torch.int32)


def trace(pkg, B, steps, two, y0, acts, reset_at=None):
    """every array a control step leaves, cloned after each of `steps` steps"""
    setup = pkg.KSSetup.bench_C2(256)
    env = pkg.PDEenv(setup, B=B, dtype=torch.float32)
    assert env.set_two_wave_step(two) == two
    term = torch.full((B, 64), -1.0, dtype=torch.float32, device=env.y.device)
    env.set_terminal_out(term)
    n = C.c_int()
    rpart = torch.full(((B + 1) // 2,), -1.0, dtype=torch.float32, device=env.y.device)
    pkg._lib.check(env.lib.pdec_env_set_reward_partials_out(env.handle, pkg._lib.ptr(rpart), C.byref(n)))
    assert n.value == (B + 1) // 2
    env.set_y0(to_dev(y0, torch.float32))
    env.reset()
    out = []
    for t in range(steps):
        if t == reset_at:
            env.reset_episode()
        env(to_dev(acts[t], torch.float32).reshape(env._ashape))
        out.append([x.clone() for x in (env.y, env.p, env.state, env.reward, env._done_flags, term, rpart)])
    torch.cuda.synchronize()
    assert not env.set_two_wave_step(False)
    return out


def compare(pkg, B, steps, y0, acts, reset_at=None):
    a, b = (trace(pkg, B, steps, two, y0, acts, reset_at) for two in (False, True))
    for t in range(steps):
        for name, u, v in zip(NAMES, a[t], b[t]):
            assert torch.equal(bits(u), bits(v)), (name, t, int((bits(u) != bits(v)).sum()))
    return a


def inputs(pkg, B, steps, seed):
    rng = np.random.default_rng(seed)
    setup = pkg.KSSetup.bench_C2(256)
    return setup.generate_random_init(rng, B) * 0.15, rng.uniform(-1, 1, (steps, B, 64))


@pytest.mark.parametrize("B", [1, 2, 3, 64])
@pytest.mark.parametrize("steps", [1, 51])
def test_two_wave_step_is_the_one_wave_step(pkg, B, steps):
    y0, acts = inputs(pkg, B, steps, 100 + B)
    a = compare(pkg, B, steps, y0, acts, reset_at=20 if steps > 20 else None)
    last = a[-1]
    assert bool(torch.isfinite(last[0]).all()) and int(last[4].sum()) == 0          # a live run, nothing blown up
    assert float(last[0].abs().max()) > 0 and float(last[6].abs().max()) > 0


def test_blown_up_trajectory(pkg):
    """trajectories 1 and 4 of 5 start far above max_value: Inf / NaN through the transforms of their workgroups (1 shares its
    packed pair with 0, whose half the overflow reaches too; 4 is alone in its workgroup), their flags raised, the pair (2, 3)
    untouched"""
    B, steps = 5, 3
    y0, acts = inputs(pkg, B, steps, 7)
    y0[1] *= 1e25       # finite in fp32, its square is not
    y0[4] *= 1e25
    a = compare(pkg, B, steps, y0, acts)
    flags, term = a[0][4].cpu().numpy(), a[0][5].cpu().numpy()
    assert flags[1:].tolist() == [1, 0, 0, 1] and (term[1] == 1).all() and (term[4] == 1).all() and (term[2:4] == 0).all()
    assert np.isfinite(a[0][0][2:4].cpu().numpy()).all()


def test_actions_at_the_clamp(pkg):
    B, steps = 3, 4
    y0, acts = inputs(pkg, B, steps, 8)
    compare(pkg, B, steps, y0, np.where(acts >= 0, 1.0, -1.0))


def test_other_environments_keep_their_kernel(pkg):
    """effective = 0: fp64, N = 1024, a disturbance array, faults, the SIMD-sharing form, the member layout; and back to 1 once
    they are unset.  The launch reads the same function as `effective` (ks_step_engine), so this is the check of the rule."""
    c2 = pkg.KSSetup.bench_C2
    assert not pkg.PDEenv(c2(256), B=2, dtype=torch.float64).set_two_wave_step(True)
    assert not pkg.PDEenv(c2(1024), B=2, dtype=torch.float32).set_two_wave_step(True)
    assert not pkg.PDEenv(pkg.KSSetup.KS22(), B=2, dtype=torch.float32).set_two_wave_step(True)
    env = pkg.PDEenv(c2(256), B=2, dtype=torch.float32)
    assert env.set_two_wave_step(True)
    env.set_disturbance(torch.ones(2))
    assert not env.set_two_wave_step(True)
    env.set_disturbance(None)
    assert env.set_two_wave_step(True)
    env.set_faults(actuator_gain=torch.ones(2, 64))
    assert not env.set_two_wave_step(True)
    env.set_faults()
    assert env.set_two_wave_step(True)
    assert env.set_simd_sharing(True) and not env.set_two_wave_step(True)
    assert not env.set_simd_sharing(False) and env.set_two_wave_step(True)
    pkg._lib.check(env.lib.pdec_env_set_member_layout(env.handle, 1))
    assert not env.set_two_wave_step(True)
    pkg._lib.check(env.lib.pdec_env_set_member_layout(env.handle, 0))
    assert env.set_two_wave_step(True)
