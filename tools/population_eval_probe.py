"""Scoring a population's actors on shared held-out states: ONE enqueue (population.evaluate_actors -> pdec_rollout_members)
against one rollout per member.

For KS22 and KellerSegelSetup at each M (K = 8 shared initial fields, T = one episode, fp64 environment, Float32 actors):
  one_launch : evaluate_actors(setup, actors, y0) -- its own B = M K environment, the pointer table, one persistent launch, the
               read-back of rewards and flags;
  loop       : what there was before -- one B = K environment, and per member actor.clone(dtype=float64), env.reset(),
               env.rollout(clone, T), then one read-back of the M x K episode rewards.
For the 2-D setups -- fluid8 = FluidSetup(nx=128) (Fluid_8) and kseg2d = KellerSegel2DSetup() -- the first mode is the batched
step loop (served = 2: the member acting kernel and the env step at B = M K, T times) and is reported under the same keys;
`route` names it.  The issue's shape for them: --setups fluid8,kseg2d --members 4,16 --inits 4.
Host clock around each whole region, which ends in a synchronise; the two modes alternate inside each round; one untimed round
first; median and min - max over the rounds.  Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run.

    python tools/population_eval_probe.py [--setups ks22,keller_segel,fluid8,kseg2d] [--members 1,8,64,256] [--inits 8]
                                          [--rounds 5] [--steps T] [--out x.json]"""
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


def make_actors(setup, M):
    ns, _ = setup.state_shape
    dims, acts = pkg.layer_spec(ns, setup.action_shape[0], setup.nna_scale, True, setup.drop_middle_layer)
    return [pkg.HipMLP(dims, acts, pkg.glorot_uniform(np.random.default_rng(100 + m), dims)) for m in range(M)]


def one_launch(setup, actors, y0, T):
    res = pkg.evaluate_actors(setup, actors, y0=y0, steps=T)        # (ends in the read-back of rewards and flags)
    assert res["one_launch"] or res["batched"]
    return res["episode_reward"]


def loop(setup, actors, y0, T):
    K, cols = y0.shape[0], y0.shape[0] * setup.state_shape[1]
    env = pkg.PDEenv(setup, B=K, dtype=torch.float64, y0=y0, autoreset=False)
    rows = []
    for a in actors:
        clone = a.clone(dtype=torch.float64, max_cols=cols)
        env.reset()
        rows.append(env.rollout(clone, T, learning=False)["reward_sum"].mean(dim=1))
    er = torch.stack(rows)
    er.cpu()                                                         # (the read-back; waits for the device)
    return er


SETUPS = dict(ks22=lambda: pkg.KSSetup.KS22(), keller_segel=lambda: pkg.KellerSegelSetup(),
              fluid8=lambda: pkg.FluidSetup(nx=128), kseg2d=lambda: pkg.KellerSegel2DSetup())


def probe(name, M, K, rounds, steps=None):
    setup = SETUPS[name]()
    T = int(round((setup.te - setup.t0) / setup.dt)) + 1 if steps is None else int(steps)
    actors = make_actors(setup, M)
    if name == "fluid8":            # (no device initialiser from a Philox stream: the setup's own random fields)
        draw = pkg.PDEenv(setup, B=K, dtype=torch.float64, y0=setup.generate_random_init(np.random.default_rng(2024), K), autoreset=False)
        y0 = draw.y0.clone()
    else:
        draw = pkg.PDEenv(setup, B=K, dtype=torch.float64, autoreset=False)
        y0 = torch.empty_like(draw.y)
        draw.random_init(2024, 0, out=y0)
    draw.close()
    torch.cuda.synchronize()
    times = dict(one_launch=[], loop=[])
    same = True
    for r in range(rounds + 1):
        got = {}
        for mode, fn in (("one_launch", one_launch), ("loop", loop)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got[mode] = fn(setup, actors, y0, T)
            torch.cuda.synchronize()
            if r:                                                    # round 0: untimed (allocations, first launches)
                times[mode].append(time.perf_counter() - t0)
        same = same and bool(torch.equal(got["one_launch"].view(torch.int64), got["loop"].view(torch.int64)))
    two_d = name in ("fluid8", "kseg2d")
    row = dict(setup=name, M=M, K=K, T=T, rounds=rounds, route="batched" if two_d else "one_launch",
               workgroups=None if two_d else (M * ((K + 1) // 2) if name == "ks22" else M * K), results_bit_identical=same)
    for mode, ts in times.items():
        ms = 1e3 * np.array(ts)
        row[mode + "_ms_median"], row[mode + "_ms_min"], row[mode + "_ms_max"] = float(np.median(ms)), float(ms.min()), float(ms.max())
    row["ratio_of_medians"] = row["loop_ms_median"] / row["one_launch_ms_median"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setups", default="ks22,keller_segel")
    ap.add_argument("--members", default="1,8,64,256")
    ap.add_argument("--inits", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=None, help="control steps per evaluation (default: one full episode)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for name in a.setups.split(","):
        for M in (int(x) for x in a.members.split(",")):
            r = probe(name, M, a.inits, max(5, a.rounds), a.steps)
            print(json.dumps(r), flush=True)
            rows.append(r)
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
