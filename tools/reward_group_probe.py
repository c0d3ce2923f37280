#!/usr/bin/env python3
"""Reward groups (pdec_ddpg_set_reward_groups) against the two existing readings of the reference's reward broadcast:
whole batch (the default), g = 3 (setup.batch_size, L = A) and the diagonal TD target.

    python tools/reward_group_probe.py timing [--B 510] [--rounds 5] [--calls 200] [--steps 120]
    python tools/reward_group_probe.py sweep [--B 63] [--episodes 60] [--seeds 3] [--noise 0.3]

timing: C2 geometry (N = 256, 64 actuators, 3-layer nets; B = 510 so that Bu = 32 640 is a whole number of 3 x 64 groups).
  (1) the critic pass alone -- pdec_ddpg_critic_grads on one update stream, device events around `calls` calls after a
      warm-up; (2) the training pipeline as bench.py runs it (two streams, captured graphs, critic pass beside the env step),
      host clock around `steps` control steps ending in a stream synchronise.  The modes alternate inside every round;
      each line reports the median over the rounds and the spread (min .. max).
sweep: TrainPipeline at KS22 geometry (N = 192, 8 actuators, 2-layer nets), B trajectories, 51-step episodes from fixed
  initial states, seeds x {whole, g3, diag} x {frozen, moving targets}; mean return (sum over the episode of the mean reward
  over B x A columns) of the first and last 10 episodes, and the zero-action return from the same initial states.
One JSON line per result on stdout."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("distributedconvrl-pde-control_amd")
L = pkg._lib
MODES = {"whole": dict(target_broadcast_group=None), "g3": dict(target_broadcast_group="setup"),
         "diag": dict(quirk_target_broadcast=False)}


def _agent(setup, B, mode, stream, seed, **kw):
    return pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(seed), dtype=torch.float32, stream=stream, start_steps=-1,
                            noise_seed=7 + seed, trajectory_length=1, **MODES[mode], **kw)


def _pipeline(setup, B, mode, seed, graphs, E, noise, **kw):
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    y0 = setup.generate_random_init(np.random.default_rng(seed), B) * 0.15
    env = pkg.PDEenv(setup, B=B, dtype=torch.float32, y0=y0, stream=s_env, autoreset=False)
    agent = _agent(setup, B, mode, s_upd, seed, **kw)
    agent.policy.act_noise = noise
    torch.cuda.synchronize()
    p = pkg.TrainPipeline(env, agent, lag=2, episode_steps=E, stream_env=s_env, stream_upd=s_upd, use_graphs=graphs,
                          noise_seed=99 + seed)
    return p, y0


def timing(a):
    setup = pkg.KSSetup.bench_C2(256)
    B, A_n, ns = a.B, setup.n_actuators, setup.state_shape[0]
    Bu = B * A_n
    s_upd = torch.cuda.Stream()
    g = torch.Generator().manual_seed(3)
    batch = {k: v.cuda() for k, v in dict(state=torch.randn(Bu, ns, generator=g), action=torch.rand(Bu, 1, generator=g) * 2 - 1,
                                          reward=-torch.rand(Bu, generator=g), terminal=(torch.rand(Bu, generator=g) < .05).float(),
                                          next_state=torch.randn(Bu, ns, generator=g)).items()}
    agents = {m: _agent(setup, B, m, s_upd, 1) for m in MODES}
    for ag in agents.values():
        ag.policy.set_reward_interleave(A_n)
    losses = torch.zeros(2, device="cuda:0")
    P_ = L.ptr

    def calls(ag, n):
        pol = ag.policy
        A, Cn, At, Ct = (pol.behavior_actor.model, pol.behavior_critic.model, pol.target_actor.model, pol.target_critic.model)
        s, act, r, t, sn = (batch[k] for k in ("state", "action", "reward", "terminal", "next_state"))
        for _ in range(n):
            L.check(pol.lib.pdec_ddpg_critic_grads(A.handle, Cn.handle, At.handle, Ct.handle, P_(s), P_(act), P_(r), P_(t), P_(sn),
                                                   Bu, 0.99, int(pol.quirk), 1.0, C.c_void_p(losses.data_ptr())))

    pass_us = {m: [] for m in MODES}
    with torch.cuda.stream(s_upd):
        for m, ag in agents.items():
            calls(ag, 20)
        s_upd.synchronize()
        for _ in range(a.rounds):
            for m, ag in agents.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s_upd)
                calls(ag, a.calls)
                e1.record(s_upd)
                e1.synchronize()
                pass_us[m].append(e0.elapsed_time(e1) * 1e3 / a.calls)
    for m, v in pass_us.items():
        print(json.dumps(dict(probe="critic_pass", mode=m, B=B, Bu=Bu, us_median=float(np.median(v)), us_min=float(np.min(v)),
                              us_max=float(np.max(v)), rounds=a.rounds, calls=a.calls)), flush=True)
    pipes = {m: _pipeline(setup, B, m, 0, True, 0, 0.3)[0] for m in MODES}
    for p in pipes.values():
        p.run(5)
        p.capture()
        p.run(2 * a.steps)
        p.sync()
    step_us = {m: [] for m in MODES}
    for _ in range(a.rounds):
        for m, p in pipes.items():
            p.sync()
            t0 = time.perf_counter()
            p.run(a.steps)
            p.sync()
            step_us[m].append((time.perf_counter() - t0) * 1e6 / a.steps)
    for m, v in step_us.items():
        print(json.dumps(dict(probe="pipeline_step", mode=m, B=B, us_median=float(np.median(v)), us_min=float(np.min(v)),
                              us_max=float(np.max(v)), rounds=a.rounds, steps=a.steps,
                              graph_launches=pipes[m].n_graph_launches)), flush=True)


def sweep(a):
    setup = pkg.KSSetup.KS22()
    E = 51
    for frozen in (True, False):
        for seed in range(a.seeds):
            zero = None
            for m in MODES:
                p, y0 = _pipeline(setup, a.B, m, seed, False, E, a.noise, quirk_frozen_targets=frozen)
                if zero is None:      # zero action from the same initial states
                    env = pkg.PDEenv(setup, B=a.B, dtype=torch.float32, y0=y0, stream=p.s_env, autoreset=False)
                    z = torch.zeros(env._ashape, dtype=torch.float32, device="cuda:0")
                    acc = 0.0
                    with torch.cuda.stream(p.s_env):
                        for _ in range(E):
                            env(z)
                            acc += float(env.reward.float().mean())
                    zero = acc
                rets = []
                acc = torch.zeros((), dtype=torch.float64, device="cuda:0")
                for k in range(a.episodes * E):
                    p.step()
                    with torch.cuda.stream(p.s_env):
                        acc += p.rring[k % 3].double().mean()
                    if k % E == E - 1:
                        p.sync()
                        rets.append(float(acc))
                        acc.zero_()
                p.sync()
                r = np.asarray(rets)
                print(json.dumps(dict(probe="sweep", mode=m, frozen=frozen, seed=seed, B=a.B, first10=float(r[:10].mean()),
                                      last10=float(r[-10:].mean()), zero_action=zero, finite=bool(np.isfinite(r).all()),
                                      returns=[round(x, 3) for x in r.tolist()])), flush=True)
                p.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("timing", "sweep"))
    ap.add_argument("--B", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--episodes", type=int, default=60)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--noise", type=float, default=0.3)
    a = ap.parse_args()
    if a.what == "timing":
        a.B = a.B or 510
        timing(a)
    else:
        a.B = a.B or 63
        sweep(a)


if __name__ == "__main__":
    main()
