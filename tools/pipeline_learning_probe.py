#!/usr/bin/env python3
"""TrainPipeline's episode ledger (log_episodes) as an instrument: what it costs, and what the pipeline learns.

    python tools/pipeline_learning_probe.py timing [--B 512] [--rounds 7] [--steps 200]
    python tools/pipeline_learning_probe.py sweep [--B 63] [--episodes 60] [--seeds 3] [--noise 0.3] [--eval-B 64]

timing: C2 geometry (N = 256, 64 actuators, 3-layer nets), captured graphs, 51-step episodes, ledger off and on alternating
  inside every round; host clock around `steps` control steps ending in a stream synchronise.  Median and spread (min .. max)
  per configuration.
sweep: KS22 geometry (N = 192, 8 actuators, 2-layer nets), B trajectories, 51-step episodes from a new random initial field
  every episode (random_init), graphs on, returns from the ledger only; {whole, g3, diag} reward broadcast x {frozen, moving}
  targets x seeds.  Every 10 episodes and at the end the best actor (best_actor()) and the final actor are evaluated
  noise-free with env.rollout on a fixed held-out set of random initial fields (seed 10 000, disjoint from training), against
  the zero action on the same set.
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
MODES = {"whole": dict(target_broadcast_group=None), "g3": dict(target_broadcast_group="setup"),
         "diag": dict(quirk_target_broadcast=False)}
E = 51
EVAL_SEED = 10_000


def _pipeline(setup, B, mode, seed, noise, **kw):
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    y0 = setup.generate_random_init(np.random.default_rng(seed), B) * 0.15
    env = pkg.PDEenv(setup, B=B, dtype=torch.float32, y0=y0, stream=s_env, autoreset=False)
    agent_kw = {k: kw.pop(k) for k in ("quirk_frozen_targets",) if k in kw}
    agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(seed), dtype=torch.float32, stream=s_upd, start_steps=-1,
                             noise_seed=7 + seed, trajectory_length=1, **MODES[mode], **agent_kw)
    agent.policy.act_noise = noise
    torch.cuda.synchronize()
    return pkg.TrainPipeline(env, agent, lag=2, episode_steps=E, stream_env=s_env, stream_upd=s_upd, use_graphs=True,
                             noise_seed=99 + seed, **kw)


def timing(a):
    setup = pkg.KSSetup.bench_C2(256)
    pipes = {n: _pipeline(setup, a.B, "whole", 0, 0.3, log_episodes=(64 if n == "ledger_on" else 0))
             for n in ("ledger_off", "ledger_on")}
    for p in pipes.values():
        p.run(5)
        p.capture()
        p.run(2 * a.steps)
        p.sync()
    us = {n: [] for n in pipes}
    for _ in range(a.rounds):
        for n, p in pipes.items():
            p.sync()
            t0 = time.perf_counter()
            p.run(a.steps)
            p.sync()
            us[n].append((time.perf_counter() - t0) * 1e6 / a.steps)
    for n, v in us.items():
        print(json.dumps(dict(probe="pipeline_step", config=n, B=a.B, us_median=float(np.median(v)), us_min=float(np.min(v)),
                              us_max=float(np.max(v)), rounds=a.rounds, steps=a.steps,
                              graph_launches=pipes[n].n_graph_launches)), flush=True)
    off, on = np.median(us["ledger_off"]), np.median(us["ledger_on"])
    print(json.dumps(dict(probe="ledger_cost", pct=float(100 * (on - off) / off))), flush=True)


def _evaluate(setup, B, model, stream):
    """mean return per trajectory (sum over the episode of the mean reward over the actuators), noise-free, on the held-out set"""
    env = pkg.PDEenv(setup, B=B, dtype=torch.float32, stream=stream, autoreset=False)
    with torch.cuda.stream(stream):
        y0 = torch.empty_like(env.y)
        env.random_init(EVAL_SEED, 0, out=y0)
    env.y0 = y0
    env.reset()
    if model is None:
        z = torch.zeros(env._ashape, dtype=torch.float32, device="cuda:0")
        acc = torch.zeros(env.B, dtype=torch.float64, device="cuda:0")
        with torch.cuda.stream(stream):
            for _ in range(E):
                env(z)
                acc += env.reward.double().mean(dim=1)
        stream.synchronize()
        return float(acc.mean())
    out = env.rollout(model.clone(dtype=env.dtype), E)       # (moved to the env's stream for the call)
    stream.synchronize()
    return float(out["reward_sum"].double().mean(dim=1).mean())


def sweep(a):
    setup = pkg.KSSetup.KS22()
    ev_stream = torch.cuda.Stream()
    zero = _evaluate(setup, a.eval_B, None, ev_stream)
    print(json.dumps(dict(probe="zero_action", eval_B=a.eval_B, ret=zero)), flush=True)
    for frozen in (True, False):
        for seed in range(a.seeds):
            for m in MODES:
                p = _pipeline(setup, a.B, m, seed, a.noise, quirk_frozen_targets=frozen, log_episodes=a.episodes,
                              random_init=True, init_seed=1 + seed)
                p.run(5)
                p.capture()
                evals = []
                while p.n_episodes < a.episodes:
                    target = min(a.episodes, (p.n_episodes // 10 + 1) * 10)
                    p.run((target - p.n_episodes) * E - (p.tick - p.ep_start) % E)
                    p.sync()
                    best = _evaluate(setup, a.eval_B, p.best_actor().model, ev_stream) if p.bestepisode > 0 else None
                    final = _evaluate(setup, a.eval_B, p.policy.behavior_actor.model, ev_stream)
                    evals.append(dict(episode=p.n_episodes, best=best, best_episode=p.bestepisode, final=final))
                r = np.asarray(p.rewards)
                last = evals[-1]
                print(json.dumps(dict(probe="sweep", mode=m, frozen=frozen, seed=seed, B=a.B, episodes=p.n_episodes,
                                      first10=float(r[:10].mean()), last10=float(r[-10:].mean()), zero_action=zero,
                                      best_eval=last["best"], final_eval=last["final"],
                                      best_beats_zero=bool(last["best"] is not None and last["best"] > zero),
                                      final_beats_zero=bool(last["final"] > zero), evals=evals,
                                      graph_launches=p.n_graph_launches, finite=bool(np.isfinite(r).all()))), flush=True)
                p.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("timing", "sweep"))
    ap.add_argument("--B", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--episodes", type=int, default=60)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--noise", type=float, default=0.3)
    ap.add_argument("--eval-B", dest="eval_B", type=int, default=64)
    a = ap.parse_args()
    if a.B is None:
        a.B = 512 if a.mode == "timing" else 63      # (63: g = 3 tiles the trajectories)
    pkg._lib.init(0)
    (timing if a.mode == "timing" else sweep)(a)


if __name__ == "__main__":
    main()
