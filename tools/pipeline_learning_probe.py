#!/usr/bin/env python3
"""TrainPipeline's episode ledger (log_episodes) and its greedy held-out evaluation (eval_every) as instruments: what they
cost, and what the pipeline learns.

    python tools/pipeline_learning_probe.py timing [--B 512] [--rounds 7] [--steps 204] [--eval-B 64]
    python tools/pipeline_learning_probe.py sweep [--B 63] [--episodes 60] [--seeds 3] [--noise 0.3] [--eval-B 64] [--eval-every 10]

timing: C2 geometry (N = 256, 64 actuators, 3-layer nets), captured graphs, 51-step episodes; the configurations -- ledger off,
  ledger on, ledger + an evaluation of eval-B fields behind EVERY episode (the worst case) on the env stream, the same on a
  third stream -- alternate inside every round, after one untimed round; host clock around `steps` control steps ending in a
  synchronise of every stream.  Median and spread (min .. max) per configuration.
sweep: KS22 geometry (N = 192, 8 actuators, 2-layer nets), B trajectories, 51-step episodes from a new random initial field
  every episode (random_init), graphs on, returns from the ledger only; {whole, g3, diag} reward broadcast x {frozen, moving}
  targets x seeds.  The noise-free numbers are the pipeline's own device evaluation rows: every eval-every episodes the actor
  is evaluated greedily on a fixed held-out set of random initial fields (seed 10 000, disjoint from training), the best
  actor is the best of those evaluations (best_by="eval"), against the zero action on the same set (eval_zero_score).
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


def _pipeline(setup, B, mode, seed, noise, streams=None, **kw):
    s_env, s_upd = streams if streams is not None else (torch.cuda.Stream(), torch.cuda.Stream())
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
    # ONE set of streams for every configuration (pdec_stream_create: one set per process, at most four)
    s_env, s_upd, s_eval = pkg._lib.make_streams((0, 0, 0))
    ev = dict(log_episodes=64, eval_every=1, eval_inits=a.eval_B, eval_seed=EVAL_SEED)
    configs = {"ledger_off": {}, "ledger_on": dict(log_episodes=64), "eval_env_stream": ev,
               "eval_third_stream": dict(ev, eval_stream=s_eval)}
    pipes = {n: _pipeline(setup, a.B, "whole", 0, 0.3, streams=(s_env, s_upd), **kw) for n, kw in configs.items()}
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
        print(json.dumps(dict(probe="pipeline_step", config=n, B=a.B, us_median=float(np.median(v)), us_min=float(np.min(v)),
                              us_max=float(np.max(v)), rounds=a.rounds, steps=a.steps,
                              graph_launches=pipes[n].n_graph_launches)), flush=True)
    off, on = np.median(us["ledger_off"]), np.median(us["ledger_on"])
    print(json.dumps(dict(probe="ledger_cost", pct=float(100 * (on - off) / off))), flush=True)
    for n in ("eval_env_stream", "eval_third_stream"):
        print(json.dumps(dict(probe="eval_cost", config=n, eval_B=a.eval_B, evaluations=pipes[n].n_evals,
                              pct_over_ledger=float(100 * (np.median(us[n]) - on) / on))), flush=True)


def sweep(a):
    setup = pkg.KSSetup.KS22()
    for frozen in (True, False):
        for seed in range(a.seeds):
            for m in MODES:
                p = _pipeline(setup, a.B, m, seed, a.noise, quirk_frozen_targets=frozen, log_episodes=a.episodes,
                              random_init=True, init_seed=1 + seed, eval_every=a.eval_every, eval_inits=a.eval_B,
                              eval_seed=EVAL_SEED, eval_capacity=max(1, a.episodes // a.eval_every), best_by="eval")
                p.run(5)
                p.capture()
                p.run(a.episodes * E - p.tick)
                p.sync()
                r = np.asarray(p.rewards)
                eps, _, blew, _ = p.eval_returns()
                scores, zero = p.eval_scores, p.eval_zero_score
                evals = [dict(episode=int(e), score=(None if np.isnan(v) else float(v)), stopped=int(bl.sum()))
                         for e, v, bl in zip(eps, scores, blew)]
                best = p.bestreward if p.bestepisode > 0 else None
                final = evals[-1]["score"] if evals and evals[-1]["episode"] == p.n_episodes else None
                print(json.dumps(dict(probe="sweep", mode=m, frozen=frozen, seed=seed, B=a.B, episodes=p.n_episodes,
                                      first10=float(r[:10].mean()), last10=float(r[-10:].mean()), zero_action=zero,
                                      best_eval=best, best_episode=p.bestepisode, final_eval=final,
                                      best_beats_zero=bool(best is not None and best > zero),
                                      final_beats_zero=bool(final is not None and final > zero), evals=evals,
                                      graph_launches=p.n_graph_launches, finite=bool(np.isfinite(r).all()))), flush=True)
                p.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("timing", "sweep"))
    ap.add_argument("--B", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=204)      # (whole 51-step episodes: every round holds the same evaluations)
    ap.add_argument("--episodes", type=int, default=60)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--noise", type=float, default=0.3)
    ap.add_argument("--eval-B", dest="eval_B", type=int, default=64)
    ap.add_argument("--eval-every", dest="eval_every", type=int, default=10)
    a = ap.parse_args()
    if a.B is None:
        a.B = 512 if a.mode == "timing" else 63      # (63: g = 3 tiles the trajectories)
    pkg._lib.init(0)
    (timing if a.mode == "timing" else sweep)(a)


if __name__ == "__main__":
    main()
