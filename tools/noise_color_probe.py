#!/usr/bin/env python3
"""Temporally correlated exploration noise of TrainPipeline (noise_corr=, set_noise_corr) as an instrument: what the state-carrying
acting kernel costs a control step, and what a correlation does to learning.

    python tools/noise_color_probe.py time [--B 512] [--rounds 7] [--steps 204] [--parent TREE] [--alternations 3]
    python tools/noise_color_probe.py learn [--B 63] [--episodes 60] [--seeds 3] [--noise 0.3] [--corrs 0,0.5,0.9] [--equal-integral]

time: C2 geometry (N = 256, 64 actuators, 3-layer nets), captured graphs, 51-step episodes; the pipeline with noise_corr unset and
  the pipeline with noise_corr = 0 (so both compute the same run) alternate inside every round, after one untimed round; host
  clock around `steps` control steps ending in a synchronise of every stream.  Median and spread (min .. max) per configuration.
  On a build without the feature a second unset pipeline stands in for the set one, so that both trees time a process with the
  same buffers and launches.  --parent TREE: a checkout of the parent commit, built; the
  measurement then runs in child processes, one per tree, TREE and this one alternating `alternations` times with the same
  arguments, and the last line says whether the unset step of this tree lies within the parent's run-to-run spread (the min ..
  max over all of the parent's rounds) -- it launches the same code objects.
learn: the learning configuration of tools/pipeline_learning_probe.py -- KS22 geometry, B trajectories, 51-step episodes from a
  new random initial field every episode, graphs on, whole-batch reward broadcast, frozen targets, greedy held-out evaluation
  every 10 episodes -- once per correlation and seed.  --equal-integral: the amplitude at correlation a is
  noise sqrt((1 - a) / (1 + a)), which keeps the variance of the noise SUMMED over many steps, sigma^2 (1 + a) / (1 - a) per step,
  at the white run's instead of the variance of one step.  A record, not a criterion.
One JSON line per result on stdout."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, NOISE, EVAL_SEED = 51, 0.3, 10_000


def _load(tree):
    import torch
    sys.path.insert(0, tree)
    pkg = importlib.import_module("distributedconvrl-pde-control_amd")
    assert os.path.dirname(os.path.dirname(os.path.abspath(pkg.__file__))) == os.path.abspath(tree), pkg.__file__
    return pkg, torch


def _pipeline(pkg, torch, setup, B, streams, seed=0, noise=NOISE, **kw):
    s_env, s_upd = streams
    y0 = setup.generate_random_init(np.random.default_rng(seed), B) * 0.15
    env = pkg.PDEenv(setup, B=B, dtype=torch.float32, y0=y0, stream=s_env, autoreset=False)
    agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(seed), dtype=torch.float32, stream=s_upd, start_steps=-1,
                             noise_seed=7 + seed, trajectory_length=1)
    agent.policy.act_noise = noise
    torch.cuda.synchronize()
    return pkg.TrainPipeline(env, agent, lag=2, episode_steps=E, stream_env=s_env, stream_upd=s_upd, use_graphs=True,
                             noise_seed=99 + seed, **kw)


def time_one(a):
    """one process, one tree: the configurations alternate inside every round"""
    pkg, torch = _load(a.tree)
    has = hasattr(pkg.TrainPipeline, "set_noise_corr")
    setup = pkg.KSSetup.bench_C2(256)
    streams = pkg._lib.make_streams((0, 0))
    # (a tree without the feature runs a second unset pipeline in the place of the set one: the same process, buffers and launches)
    configs = {"unset": {}, "set" if has else "unset_twin": dict(noise_corr=0.0) if has else {}}
    pipes = {n: _pipeline(pkg, torch, setup, a.B, streams, **kw) for n, kw in configs.items()}
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
        print(json.dumps(dict(probe="noise_color_step", tree=a.label, config=n, B=a.B, us_median=float(np.median(v)),
                              us_min=float(np.min(v)), us_max=float(np.max(v)), us=[round(x, 3) for x in v], rounds=a.rounds,
                              steps=a.steps, graph_launches=pipes[n].n_graph_launches)), flush=True)
    if has:
        same = bool(torch.equal(pipes["unset"].y, pipes["set"].y))
        print(json.dumps(dict(probe="noise_color_cost", tree=a.label, same_run=same,
                              pct=float(100 * (np.median(us["set"]) - np.median(us["unset"])) / np.median(us["unset"])))), flush=True)


def timing(a):
    if not a.parent:
        a.tree, a.label = ROOT, "this"
        return time_one(a)
    rows = []
    for i in range(a.alternations):
        for label, tree in (("parent", os.path.abspath(a.parent)), ("this", ROOT)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "time-one", "--tree", tree, "--label", label, "--B", str(a.B),
                                  "--rounds", str(a.rounds), "--steps", str(a.steps)], capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                sys.stderr.write(out.stderr[-4000:])
                raise SystemExit(f"noise_color_probe: the child for the tree '{label}' ended with status {out.returncode}")
            for line in out.stdout.splitlines():
                if line.startswith("{"):
                    print(line, flush=True)
                    rows.append(dict(json.loads(line), alternation=i))
    pick = lambda tree, cfg: [x for r in rows if r["probe"] == "noise_color_step" and r["tree"] == tree and r["config"] == cfg
                              for x in r["us"]]
    par, unset, on = pick("parent", "unset"), pick("this", "unset"), pick("this", "set")
    med = lambda v: float(np.median(v))
    print(json.dumps(dict(probe="noise_color_summary", B=a.B, alternations=a.alternations, rounds=a.rounds, steps=a.steps,
                          parent_unset=dict(median=med(par), min=min(par), max=max(par)),
                          this_unset=dict(median=med(unset), min=min(unset), max=max(unset)),
                          this_set=dict(median=med(on), min=min(on), max=max(on)),
                          unset_median_within_parent_spread=bool(min(par) <= med(unset) <= max(par)),
                          set_cost_pct=float(100 * (med(on) - med(unset)) / med(unset)))), flush=True)


def learn(a):
    pkg, torch = _load(ROOT)
    setup = pkg.KSSetup.KS22()
    for corr in [float(x) for x in a.corrs.split(",")]:
        for seed in range(a.seeds):
            noise = a.noise * (np.sqrt((1 - corr) / (1 + corr)) if a.equal_integral else 1.0)
            p = _pipeline(pkg, torch, setup, a.B, (torch.cuda.Stream(), torch.cuda.Stream()), seed=seed, noise=noise,
                          noise_corr=corr, log_episodes=a.episodes, random_init=True, init_seed=1 + seed, eval_every=a.eval_every,
                          eval_inits=a.eval_B, eval_seed=EVAL_SEED, eval_capacity=max(1, a.episodes // a.eval_every), best_by="eval")
            p.run(5)
            p.capture()
            p.run(a.episodes * E - p.tick)
            p.sync()
            r = np.asarray(p.rewards)
            eps, _, _, _ = p.eval_returns()
            scores, zero = p.eval_scores, p.eval_zero_score
            best = p.bestreward if p.bestepisode > 0 else None
            print(json.dumps(dict(probe="noise_color_learn", corr=corr, seed=seed, B=a.B, noise=float(noise), episodes=p.n_episodes,
                                  first10=float(r[:10].mean()), last10=float(r[-10:].mean()), zero_action=zero, best_eval=best,
                                  best_episode=p.bestepisode,
                                  evals=[None if np.isnan(v) else round(float(v), 4) for v in scores],
                                  eval_episodes=[int(e) for e in eps], graph_launches=p.n_graph_launches,
                                  finite=bool(np.isfinite(r).all()))), flush=True)
            p.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["time", "time-one", "learn"])
    ap.add_argument("--B", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=204)      # (whole 51-step episodes)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--label", default="this")
    ap.add_argument("--episodes", type=int, default=60)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--noise", type=float, default=0.3)
    ap.add_argument("--corrs", default="0,0.5,0.9")
    ap.add_argument("--equal-integral", dest="equal_integral", action="store_true")
    ap.add_argument("--eval-B", dest="eval_B", type=int, default=64)
    ap.add_argument("--eval-every", dest="eval_every", type=int, default=10)
    a = ap.parse_args()
    if a.B is None:
        a.B = 63 if a.what == "learn" else 512
    {"time": timing, "time-one": time_one, "learn": learn}[a.what](a)
