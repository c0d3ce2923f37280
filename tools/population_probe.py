"""Throughput of a Population (population.py) against the same members run one after another.

For KS22, KS200 and the fluid (fluid8: Fluid_8 on the reference's 128 x 128 grid, --te for shorter episodes) at each M: env-steps/s of the population (host clock around whole episodes, ending in a synchronise), the
host time per episode split into its phases (Population.timing: issue = initialisers and every enqueue up to the read-back,
readback = the wait for the device, settle = the members' host bookkeeping and the boundary launches), and at M <= 8 the same
members as M solo run() calls back to back (the fluid: at every M).
With --episodes-per-sync 1,8 every mode gets its own population of the same members; after one untimed round the modes alternate
inside each of --rounds rounds (a region = one pop.run of --episodes episodes), and a row per mode reports the median (min - max)
of env-steps/s over the rounds and the host phases per block (a block = one read-back; at 1 every episode is a block).
Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script.

    python tools/population_probe.py [--setups ks22,ks200] [--members 1,8,32,128,256,320] [--episodes 3] [--out probe.json]
                                     [--episodes-per-sync 1,8] [--rounds 5]
    python tools/population_probe.py --setups fluid8 --members 1,4,16 --episodes-per-sync 1,4 --episodes 3 --rounds 5 [--te 2.0]"""
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


def make_setup(name, te=None):
    if name == "fluid8":
        return pkg.FluidSetup.Fluid_8(**({} if te is None else dict(te=te)))
    return getattr(pkg.KSSetup, {"ks22": "KS22", "ks200": "KS200"}[name])()


def members(setup, seeds, s_upd):
    ags = [pkg.create_agent(setup=setup, B=1, rng=np.random.default_rng(s), noise_seed=s, stream=s_upd) for s in seeds]
    if getattr(setup, "is_fluid", False):       # the fluid script's hook: its error_detection, every member's own generator
        hks = [setup.make_hook(min_best_episode=1, use_random_init=True, init_seed=s, init_rng=np.random.default_rng(s)) for s in seeds]
    else:
        hks = [pkg.PDEhook(min_best_episode=1, use_random_init=True, init_seed=s) for s in seeds]
    for a in ags:
        a.policy.act_noise = setup.act_noise
    return ags, hks


def probe(name, M, episodes, modes=(1,), rounds=1, te=None):
    setup = make_setup(name, te)
    s_env, s_upd = pkg.make_streams((-1, 0))
    pops, walls = {}, {E: [] for E in modes}
    for E in modes:
        ags, hks = members(setup, list(range(M)), s_upd)
        pops[E] = pkg.Population(setup, ags, hks, stream_env=s_env, dtype=torch.float64)

    def region(E):
        kw = dict(episodes_per_sync=E) if E != 1 else {}
        t0 = time.perf_counter()
        pops[E].run([pkg.StopAfterEpisode(episodes) for _ in range(M)], **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for E in modes:                                                # the untimed round (allocations, first updates)
        region(E)
        pops[E].timing = dict(episodes=0, issue_s=0.0, readback_s=0.0, settle_s=0.0, blocks=0)
    for _ in range(rounds):
        for E in modes:
            walls[E].append(region(E))
    rows = []
    for E in modes:
        pop, w = pops[E], np.array(walls[E])
        T, tm = pop._logs.T, pop.timing
        blocks = tm.get("blocks") or tm["episodes"]
        rate = M * T * episodes / w
        row = dict(setup=name, M=M, T=T, episodes=episodes, episodes_per_sync=E, rounds=rounds,
                   env_steps_per_s=float(np.median(rate)), env_steps_per_s_min=float(rate.min()), env_steps_per_s_max=float(rate.max()),
                   wall_per_episode_ms=1e3 * float(np.median(w)) / episodes, blocks=blocks, episodes_per_block=tm["episodes"] / blocks,
                   issue_ms=1e3 * tm["issue_s"] / blocks, readback_wait_ms=1e3 * tm["readback_s"] / blocks,
                   settle_ms=1e3 * tm["settle_s"] / blocks)
        rows.append(row)
    if M <= 8 or name == "fluid8":
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
        rows[0]["solo_back_to_back_env_steps_per_s"] = M * T * episodes / ws
    for pop in pops.values():
        pop.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setups", default="ks22,ks200")
    ap.add_argument("--members", default="1,8,32,128,256,320")
    ap.add_argument("--episodes", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--episodes-per-sync", default="1", help="comma list of modes, alternated inside every round")
    ap.add_argument("--rounds", type=int, default=1, help="timed rounds behind the one untimed round")
    ap.add_argument("--te", type=float, default=None, help="fluid8: episode length in time units (default: the script's 6.0)")
    a = ap.parse_args()
    modes = tuple(int(x) for x in a.episodes_per_sync.split(","))
    rows = []
    for name in a.setups.split(","):
        for M in (int(x) for x in a.members.split(",")):
            for r in probe(name, M, a.episodes, modes, a.rounds, a.te):
                print(json.dumps(r), flush=True)
                rows.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
