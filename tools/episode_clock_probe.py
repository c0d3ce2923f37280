#!/usr/bin/env python3
"""Per-trajectory episodes (TrainPipeline(episodes="per_trajectory"), csrc/episode_clock.hip) as measured: what the mode costs
per control step beside the lock-stepped one, and what the two modes learn.

    python tools/episode_clock_probe.py timing [--B 512] [--rounds 7] [--steps 200]
    python tools/episode_clock_probe.py learning [--B 63] [--episodes 60] [--seeds 3] [--noise 0.3]

timing: C2 geometry (N = 256, 64 actuators, 3-layer nets), captured graphs, 51-step episodes, the episode log on in every
  configuration -- lock-stepped, per trajectory, per trajectory with staggered clocks -- alternating inside every round, after
  one untimed round; host clock around `steps` control steps ending in a synchronise of every stream.  Median and spread
  (min .. max) per configuration.  The lock-stepped run issues the first and the last step of every episode eagerly and sums
  the batch-mean reward from the env step's partials; the per-trajectory run replays graphs throughout, adds the clock's two
  launches per step and takes the mean with pdec_reward_mean.
learning: the learning configuration of tools/pipeline_learning_probe.py (KS22 geometry, B trajectories, 51-step episodes from
  a new random field each, whole reward broadcast, frozen targets, graphs on), lock-stepped against per-trajectory with
  staggered clocks, `seeds` seeds.  Per window of 51 control steps: the mean reward per trajectory and step of the episodes
  that ended in it (lock-stepped: the one episode; per trajectory: sum of returns / sum of lengths), and how many ended by a
  blow-up.
One JSON line per result on stdout."""
import argparse
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
E = 51


def _pipeline(setup, B, seed, noise, streams=None, **kw):
    s_env, s_upd = streams if streams is not None else (torch.cuda.Stream(), torch.cuda.Stream())
    y0 = setup.generate_random_init(np.random.default_rng(seed), B) * 0.15
    env = pkg.PDEenv(setup, B=B, dtype=torch.float32, y0=y0, stream=s_env, autoreset=False)
    agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(seed), dtype=torch.float32, stream=s_upd, start_steps=-1,
                             noise_seed=7 + seed, trajectory_length=1)
    agent.policy.act_noise = noise
    torch.cuda.synchronize()
    return pkg.TrainPipeline(env, agent, lag=2, episode_steps=E, stream_env=s_env, stream_upd=s_upd, use_graphs=True,
                             noise_seed=99 + seed, **kw)


def timing(a):
    setup = pkg.KSSetup.bench_C2(256)
    s_env, s_upd = pkg._lib.make_streams((0, 0))       # one set of streams for every configuration
    configs = {"lockstep": dict(log_episodes=64), "per_trajectory": dict(log_episodes=64, episodes="per_trajectory"),
               "per_trajectory_stagger": dict(log_episodes=64, episodes="per_trajectory", stagger=True)}
    pipes = {n: _pipeline(setup, a.B, 0, 0.3, streams=(s_env, s_upd), **kw) for n, kw in configs.items()}
    for p in pipes.values():
        p.run(5)
        p.capture()
        p.run(a.steps)
        p.sync()
    us = {n: [] for n in pipes}
    for r in range(a.rounds + 1):               # (round 0 is not timed)
        for n, p in pipes.items():
            p.sync()
            t0 = time.perf_counter()
            p.run(a.steps)
            p.sync()
            if r > 0:
                us[n].append((time.perf_counter() - t0) * 1e6 / a.steps)
    for n, v in us.items():
        p = pipes[n]
        print(json.dumps(dict(probe="pipeline_step", config=n, B=a.B, us_median=float(np.median(v)), us_min=float(np.min(v)),
                              us_max=float(np.max(v)), rounds=a.rounds, steps=a.steps, graph_launches=p.n_graph_launches,
                              eager_steps=p.n_eager_steps)), flush=True)
    base = np.median(us["lockstep"])
    for n in ("per_trajectory", "per_trajectory_stagger"):
        print(json.dumps(dict(probe="mode_cost", config=n, pct_over_lockstep=float(100 * (np.median(us[n]) - base) / base))),
              flush=True)


def learning(a):
    setup = pkg.KSSetup.KS22()
    n_steps = a.episodes * E
    for seed in range(a.seeds):
        for mode in ("lockstep", "per_trajectory"):
            kw = dict(random_init=True, init_seed=1 + seed)
            if mode == "lockstep":
                kw.update(log_episodes=a.episodes)
            else:
                kw.update(log_episodes=4 * a.episodes, episodes="per_trajectory", stagger=True)
            p = _pipeline(setup, a.B, seed, a.noise, **kw)
            p.run(5)
            p.capture()
            p.run(n_steps - p.tick)
            p.sync()
            if mode == "lockstep":
                ret, blew, dropped = p.episode_returns()
                per_step = [float(r.mean() / E) for r in ret]
                ended = [int(b.sum()) for b in blew]
                n_eps = [a.B] * len(per_step)
            else:
                fin = p.finished_episodes()
                dropped = fin["dropped"]
                per_step, ended, n_eps = [], [], []
                for w in range(a.episodes):
                    m = (fin["end_step"] > w * E) & (fin["end_step"] <= (w + 1) * E)
                    per_step.append(float(fin["ret"][m].sum() / max(1, fin["length"][m].sum())))
                    ended.append(int(fin["blew_up"][m].sum()))
                    n_eps.append(int(m.sum()))
            finite = all(np.isfinite(x).all() for n in ("behavior_actor", "behavior_critic") for x in getattr(p.policy, n).model.params())
            print(json.dumps(dict(probe="learning", mode=mode, seed=seed, B=a.B, steps=n_steps, window=E,
                                  first10=float(np.mean(per_step[:10])), last10=float(np.mean(per_step[-10:])),
                                  reward_per_step=per_step, episodes_ended=n_eps, blew_up=ended, dropped=int(dropped),
                                  graph_launches=p.n_graph_launches, eager_steps=p.n_eager_steps, nets_finite=bool(finite))),
                  flush=True)
            p.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("timing", "learning"))
    ap.add_argument("--B", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--episodes", type=int, default=60)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--noise", type=float, default=0.3)
    a = ap.parse_args()
    if a.B is None:
        a.B = 512 if a.mode == "timing" else 63
    pkg._lib.init(0)
    (timing if a.mode == "timing" else learning)(a)


if __name__ == "__main__":
    main()
