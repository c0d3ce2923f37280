"""Throughput of a Population (population.py) against the same members run one after another.

For KS22 and KS200 at each M: env-steps/s of the population (host clock around whole episodes, ending in a synchronise), the
host time per episode split into its phases (Population.timing: issue = initialisers and every enqueue up to the read-back,
readback = the wait for the device, settle = the members' host bookkeeping and the boundary launches), and at M <= 8 the same
members as M solo run() calls back to back.
Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script.

    python tools/population_probe.py [--setups ks22,ks200] [--members 1,8,32,128,256,320] [--episodes 3] [--out probe.json]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("distributedconvrl-pde-control_amd")


def members(setup, seeds, s_upd):
    ags = [pkg.create_agent(setup=setup, B=1, rng=np.random.default_rng(s), noise_seed=s, stream=s_upd) for s in seeds]
    hks = [pkg.PDEhook(min_best_episode=1, use_random_init=True, init_seed=s) for s in seeds]
    for a in ags:
        a.policy.act_noise = setup.act_noise
    return ags, hks


def probe(name, M, episodes):
    setup = getattr(pkg.KSSetup, {"ks22": "KS22", "ks200": "KS200"}[name])()
    s_env, s_upd = pkg.make_streams((-1, 0))
    ags, hks = members(setup, list(range(M)), s_upd)
    pop = pkg.Population(setup, ags, hks, stream_env=s_env, dtype=torch.float64)
    pop.run([pkg.StopAfterEpisode(1) for _ in range(M)])          # warm-up (allocations, first updates)
    torch.cuda.synchronize()
    T = pop._logs.T
    pop.timing = dict(episodes=0, issue_s=0.0, readback_s=0.0, settle_s=0.0)
    t0 = time.perf_counter()
    for _ in range(episodes):
        pop.run([pkg.StopAfterEpisode(1) for _ in range(M)])
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    tm = pop.timing
    row = dict(setup=name, M=M, T=T, episodes=episodes, env_steps_per_s=M * T * episodes / wall, wall_per_episode_ms=1e3 * wall / episodes,
               issue_ms=1e3 * tm["issue_s"] / tm["episodes"], readback_wait_ms=1e3 * tm["readback_s"] / tm["episodes"],
               settle_ms=1e3 * tm["settle_s"] / tm["episodes"])
    if M <= 8:
        envs = [pkg.PDEenv(setup, B=1, dtype=torch.float64, stream=s_env) for _ in range(M)]
        sa, sh = members(setup, list(range(M)), s_upd)
        for a, h, e in zip(sa, sh, envs):
            pkg.run(a, e, pkg.StopAfterEpisode(1), h)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(episodes):
            for a, h, e in zip(sa, sh, envs):
                pkg.run(a, e, pkg.StopAfterEpisode(1), h)
        torch.cuda.synchronize()
        ws = time.perf_counter() - t0
        row["solo_back_to_back_env_steps_per_s"] = M * T * episodes / ws
    pop.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setups", default="ks22,ks200")
    ap.add_argument("--members", default="1,8,32,128,256,320")
    ap.add_argument("--episodes", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for name in a.setups.split(","):
        for M in (int(x) for x in a.members.split(",")):
            r = probe(name, M, a.episodes)
            print(json.dumps(r), flush=True)
            rows.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
