"""Return against the number of dead actuators and of dead sensors for the saved KS200 actors, and what the fault arrays cost.

Part 1 (the question the weight-shared controller rests on: every actuator runs the same small policy on its own sensor window, so it
should keep working when single actuators or sensors do not).  The saved KS200 actors of tools/ks_robustness_probe.py -- the
behaviour actor of the reference's training run, its never-moved target actor and the zero policy -- are evaluated on K random
fields under scenarios with n dead actuators, then n dead sensors, n from --dead: the same n units for every actor, drawn once
from numpy's default_rng(--seed) so that the scenarios are nested (the 5 dead ones are among the 10).  All scenarios of a kind are
ONE persistent launch (population.evaluate_actors(faults=[...]) -> PDEenv.set_faults -> pdec_env_set_faults,
pdec_rollout_members).  One JSON line per (actor, kind, n): mean / min / max over the K fields of the episode reward, the score (NaN
when a trajectory blew up) and how many did.

Part 2: the fused step at the C2 geometry (bench_C2, 256 cells, fp32, B = --batch) and the persistent KS200 rollout (fp64, B = 64,
--roll-steps steps, the behaviour actor), each with the arrays unset and set (healthy values: the same work for the kernels as any
others): device time per launch from the library's profile (pdec_prof_*: the fp32 256-cell step, healthy or fault-carrying, by the
dispatch's own timestamps with no packets around the kernel; the rollout by an event pair around its launch), --reps rounds in which
the two variants alternate, --iters launches each (the rollout: --iters / 50); median with min and max over the rounds.

    python tools/ks_fault_probe.py [--dead 0,1,2,5,10,20] [--inits 8] [--steps 500] [--seed 2024] [--batch 512] [--out x.json]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
pkg = importlib.import_module("distributedconvrl-pde-control_amd")
from ks_robustness_probe import saved_actors  # noqa: E402


def healthy(setup, B):
    sc = setup.fault_scenario()
    return {k: np.tile(v, (B, 1)) for k, v in sc.items()}


def timed(env, scope, variants, reps, iters):
    """device time of the launches named `scope` (the library's profile, pdec_prof_*; both variants by the same method): for each of `reps` rounds
    every variant in turn -- (name, prepare, call) -- makes `iters` calls between two synchronisations, so that the variants
    alternate within one session; microseconds per launch, (median, min, max) over the rounds"""
    import ctypes as C
    L, lib = pkg._lib, env.lib
    out = {name: [] for name, _, _ in variants}
    for rep in range(reps + 1):                     # (round 0 warms every variant up and is dropped)
        for name, prepare, call in variants:
            prepare()
            call()
            torch.cuda.synchronize()
            L.check(lib.pdec_prof_reset(env.handle))
            L.check(lib.pdec_prof_enable(env.handle, 1))
            for _ in range(iters):
                call()
            torch.cuda.synchronize()
            ms, n = C.c_double(), C.c_int()
            L.check(lib.pdec_prof_get(env.handle, scope, C.byref(ms), C.byref(n)))
            L.check(lib.pdec_prof_enable(env.handle, 0))
            assert n.value == iters, (scope, n.value)
            if rep:
                out[name].append(ms.value * 1e3)         # (pdec_prof_get: the mean per launch, in ms)
    return {k: dict(median_us=float(np.median(v)), min_us=float(min(v)), max_us=float(max(v))) for k, v in out.items()}


def returns(a, setup, names, actors):
    rng = np.random.default_rng(a.seed)
    dead = sorted(int(x) for x in a.dead.split(","))
    order = {"actuators": rng.permutation(setup.n_actuators) + 1, "sensors": rng.permutation(setup.n_sensors) + 1}
    rows = []
    for kind in ("actuators", "sensors"):
        scen = [setup.fault_scenario(**{"dead_" + kind: order[kind][:n]}) for n in dead]
        res = pkg.evaluate_actors(setup, actors, n_inits=a.inits, init_seed=a.seed, steps=a.steps, faults=scen)
        er, ds = res["episode_reward"].cpu().numpy(), res["done_step"].cpu().numpy()
        for m, name in enumerate(names):
            for i, n in enumerate(dead):
                rows.append(dict(actor=name, dead=kind, n=n, K=a.inits, steps=a.steps, mean_return=float(er[m, i].mean()),
                                 min_return=float(er[m, i].min()), max_return=float(er[m, i].max()), score=float(res["score"][m, i]),
                                 blown_up=int((ds[m, i] >= 0).sum()), one_launch=bool(res["one_launch"])))
                print(json.dumps(rows[-1]), flush=True)
    return rows


def costs(a, setup200, actor200):
    rows = []

    def report(what, B, res):
        for name, r in res.items():
            rows.append(dict(what=what, B=B, arrays=name, **r))
            print(json.dumps(rows[-1]), flush=True)

    # the fused step, C2 geometry
    setup = pkg.KSSetup.bench_C2(256)
    B = a.batch
    y0 = setup.generate_random_init(np.random.default_rng(0), B) * 0.15
    env = pkg.PDEenv(setup, B=B, dtype=torch.float32, y0=y0, autoreset=False)
    act = torch.zeros(env._ashape, dtype=torch.float32, device=env.device)
    f = healthy(setup, B)
    for share in (False, True):
        env.set_simd_sharing(share)
        variants = [("unset", lambda: (env.set_faults(), env.reset()), lambda: env(act)),
                    ("set", lambda: (env.set_faults(**f), env.reset()), lambda: env(act))]
        report("ks_env_step C2 fp32" + (", simd-sharing form" if share else ""), B, timed(env, b"ks_env_step", variants, a.reps, a.iters))
    env.close()
    # the persistent rollout, KS200
    B, T = 64, a.roll_steps
    y0 = setup200.generate_random_init(np.random.default_rng(0), B) * 0.15
    env = pkg.PDEenv(setup200, B=B, dtype=torch.float64, y0=y0, autoreset=False)
    actor = actor200.clone(dtype=torch.float64, max_cols=B * setup200.n_actuators)
    f200 = healthy(setup200, B)

    def roll():
        env.reset()
        env.rollout(actor, T, learning=False)
    variants = [("unset", lambda: env.set_faults(), roll), ("set", lambda: env.set_faults(**f200), roll)]
    report(f"ks_rollout KS200 fp64, {T} steps", B, timed(env, b"ks_rollout", variants, a.reps, max(1, a.iters // 50)))
    env.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dead", default="0,1,2,5,10,20")
    ap.add_argument("--inits", type=int, default=8)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--roll-steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    setup = pkg.KSSetup.KS200()
    names, actors = saved_actors(setup)
    torch.cuda.synchronize()
    out = dict(returns=returns(a, setup, names, actors), costs=costs(a, setup, actors[0]))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
