#!/usr/bin/env python3
"""The per-trajectory exploration amplitude of TrainPipeline (noise_scale=, set_noise_scale) as an instrument: what the
array-set acting kernel costs a control step, and what a ladder of noise levels over the batch shows.

    python tools/noise_scale_probe.py timing [--B 512] [--rounds 7] [--steps 200]
    python tools/noise_scale_probe.py ladder [--B 512] [--episodes 30] [--levels 0.0,0.05,0.1,0.3,0.6,1.2]

timing: C2 geometry (N = 256, 64 actuators, 3-layer nets), captured graphs, 51-step episodes; the pipeline with the array unset and
  the pipeline with an array of B equal values (so both compute the same run) alternate inside every round, after one untimed
  round; host clock around `steps` control steps ending in a synchronise of every stream.  Median and spread (min .. max) per
  configuration.  On a build without the feature only the unset configuration runs, so the same command measures the parent.
ladder: the same pipeline, the levels repeated over the batch (trajectory b explores at levels[b % n]); per level the batch-mean
  return of the last `episodes` episodes from the ledger's per-trajectory returns [n, B].  A record, not a criterion.
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
E, NOISE = 51, 0.3
HAS = hasattr(pkg.TrainPipeline, "set_noise_scale")


def _pipeline(setup, B, streams, **kw):
    s_env, s_upd = streams
    y0 = setup.generate_random_init(np.random.default_rng(0), B) * 0.15
    env = pkg.PDEenv(setup, B=B, dtype=torch.float32, y0=y0, stream=s_env, autoreset=False)
    agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(0), dtype=torch.float32, stream=s_upd, start_steps=-1,
                             noise_seed=7, trajectory_length=1)
    agent.policy.act_noise = NOISE
    torch.cuda.synchronize()
    return pkg.TrainPipeline(env, agent, lag=2, episode_steps=E, stream_env=s_env, stream_upd=s_upd, use_graphs=True,
                             noise_seed=99, **kw)


def timing(a):
    setup = pkg.KSSetup.bench_C2(256)
    streams = pkg._lib.make_streams((0, 0))
    configs = {"unset": {}}
    if HAS:
        configs["set"] = dict(noise_scale=np.full(a.B, NOISE))
    pipes = {n: _pipeline(setup, a.B, streams, **kw) for n, kw in configs.items()}
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
        print(json.dumps(dict(probe="noise_scale_step", config=n, B=a.B, us_median=float(np.median(v)), us_min=float(np.min(v)),
                              us_max=float(np.max(v)), rounds=a.rounds, steps=a.steps,
                              graph_launches=pipes[n].n_graph_launches)), flush=True)
    if HAS:
        same = bool(torch.equal(pipes["unset"].y, pipes["set"].y))
        print(json.dumps(dict(probe="noise_scale_cost", pct=float(100 * (np.median(us["set"]) - np.median(us["unset"]))
                                                                 / np.median(us["unset"])), same_run=same)), flush=True)


def ladder(a):
    setup = pkg.KSSetup.bench_C2(256)
    levels = np.array([float(x) for x in a.levels.split(",")])
    scale = levels[np.arange(a.B) % len(levels)]
    p = _pipeline(setup, a.B, pkg._lib.make_streams((0, 0)), noise_scale=scale, log_episodes=a.episodes, random_init=True)
    p.run(5)
    p.capture()
    p.run(a.episodes * E + E - p.tick % E)
    p.sync()
    ret, blew, _ = p.episode_returns()
    for lv in levels:
        sel = scale == lv
        r = ret[:, sel]
        print(json.dumps(dict(probe="noise_ladder", level=float(lv), trajectories=int(sel.sum()), episodes=int(ret.shape[0]),
                              mean_return=float(np.nanmean(r)), first_third=float(np.nanmean(r[: max(1, len(r) // 3)])),
                              last_third=float(np.nanmean(r[-max(1, len(r) // 3):])), blew_up=int(blew[:, sel].sum()))), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["timing", "ladder"])
    ap.add_argument("--B", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--episodes", type=int, default=30)
    ap.add_argument("--levels", default="0.0,0.05,0.1,0.3,0.6,1.2")
    a = ap.parse_args()
    {"timing": timing, "ladder": ladder}[a.what](a)
