"""What population sweeps cost on the device: the population update launch with per-member hyper-parameters, and the clone launch.

Two workloads (KS22, M members), each meant to run under `rocprofv3 --kernel-trace --stats` in a run of its own:

    python tools/population_sweep_probe.py work-update [--members 256] [--episodes 3] [--sweep]
    python tools/population_sweep_probe.py work-clone  [--members 256] [--pairs 64]

`work-update` trains the population for some episodes (--sweep: members with their own gamma, learning rates and act_limit;
without it equal members, which is all an older library serves).  `work-clone` fills the sources' replay counters to capacity
and clones --pairs learners once with replay="keep" and once with replay="copy" (two launches of pop_clone_members_kernel, in
that order); it prints the bytes each launch moves.

    python tools/population_sweep_probe.py collect [--repeats 3] [--root OTHER_CHECKOUT] [--out DIR] [--hbm-gbs 8000]

runs the workloads under the profiler -- every run a child process under its own `timeout` -- and prints one JSON line: per
repeat the mean duration of the update launch, their mean and spread (max - min) over the repeats, and the clone launches'
times with their bytes as a fraction of --hbm-gbs.  --root runs the update workload of another built checkout (its package and
library, e.g. the parent commit's) with equal members, which is all it serves; the clone is skipped there."""
import argparse
import csv
import glob
import importlib
import json
import os
import subprocess
import sys

# the checkout whose package and library the workloads run (collect --root: another commit's, built)
ROOT = os.environ.get("PDEC_PROBE_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPDATE_KERNELS = ("ddpg_small2f_kernel", "ddpg_small2_kernel", "ddpg_small_kernel")


def _population(M, sweep):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("distributedconvrl-pde-control_amd")
    setup = pkg.KSSetup.KS22()
    s_env, s_upd = pkg.make_streams((-1, 0))
    ags = []
    for m in range(M):
        kw = {}
        if sweep:
            kw = dict(gamma=(0.99, 0.95, 0.9)[m % 3], learning_rate=setup.learning_rate * (1.0, 0.5, 2.0)[m % 3],
                      learning_rate_critic=setup.learning_rate_critic * (1.0, 2.0, 0.5)[m % 3], act_limit=(1.0, 0.8, 1.0)[m % 3])
        ags.append(pkg.create_agent(setup=setup, B=1, rng=np.random.default_rng(m), noise_seed=m, stream=s_upd, **kw))
    hks = [pkg.PDEhook(min_best_episode=1, use_random_init=True, init_seed=m) for m in range(M)]
    for a in ags:
        a.policy.act_noise = setup.act_noise
    return pkg, torch, pkg.Population(setup, ags, hks, stream_env=s_env, dtype=torch.float64)


def work_update(a):
    pkg, torch, pop = _population(a.members, a.sweep)
    for _ in range(a.episodes + 1):           # (the first episode: allocations, the first updates)
        pop.run([pkg.StopAfterEpisode(1) for _ in range(a.members)])
    torch.cuda.synchronize()
    print(json.dumps(dict(work="update", M=a.members, episodes=a.episodes + 1, sweep=bool(a.sweep), T=pop._logs.T)))


def work_clone(a):
    pkg, torch, pop = _population(a.members, True)
    M, n = a.members, a.pairs
    pop.run([pkg.StopAfterEpisode(1) for _ in range(M)])
    torch.cuda.synchronize()
    pairs = {M - 1 - k: k for k in range(n)}
    pol, tr = pop.agents[0].policy, pop.agents[0].trajectory
    learner = 4 * (3 * (pol.behavior_actor.model.num_params + pol.behavior_critic.model.num_params)
                   + pol.behavior_actor.model.num_params + pol.behavior_critic.model.num_params) + 2 * 16 + 8
    pop.clone(pairs, replay="keep")
    torch.cuda.synchronize()
    for k in range(n):                        # full rings: the most a clone can move
        t = pop.agents[k].trajectory
        t.n_sa, t.n_rt = t.capacity + t.stride + 5 * t.stride, t.capacity + 5 * t.stride
    pop.clone(pairs, replay="copy")
    torch.cuda.synchronize()
    rows_sa, rows_rt = tr.capacity + tr.stride, tr.capacity
    replay = 4 * (rows_sa * (tr.state.shape[1] + tr.action.shape[1]) + 2 * rows_rt)
    print(json.dumps(dict(work="clone", M=M, pairs=n, bytes_copied_keep=n * learner, bytes_copied_copy=n * (learner + replay))))


def _short(name):
    return name.split("(")[0].replace("void ", "").replace("pdec::", "").strip()


def _kernel_rows(out_dir):
    """[(kernel name, ns), ...] in launch order from the kernel trace a profiler run left under out_dir"""
    trace = []
    for f in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
        trace += [(_short(r["Kernel_Name"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in rows]
    return trace


def _profiled(tag, args, out, root, limit):
    d = os.path.join(out, tag)
    env = dict(os.environ)
    if root:
        env["PDEC_PROBE_ROOT"] = os.path.abspath(root)
    cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit(f"{tag}: exit status {p.returncode}; nothing more is started")
    info = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    return (info[-1] if info else {}), _kernel_rows(d)


def collect(a):
    os.makedirs(a.out, exist_ok=True)
    res = dict(root=a.root or "this checkout", M=a.members, update=[])
    for variant in (["equal"] if a.root else ["equal", "sweep"]):
        means = []
        for k in range(a.repeats):
            args = ["work-update", "--members", str(a.members), "--episodes", str(a.episodes)] + (["--sweep"] if variant == "sweep" else [])
            _, trace = _profiled(f"update_{variant}_{k}", args, a.out, a.root, a.limit)
            names = sorted({n for n, _ in trace if n.startswith(UPDATE_KERNELS)})
            if len(names) != 1:
                raise SystemExit(f"expected one update kernel in the trace, found {names}")
            ns = [t for n, t in trace if n == names[0]]
            means.append(dict(kernel=names[0], calls=len(ns), mean_us=sum(ns) / len(ns) / 1e3))
        us = [m["mean_us"] for m in means]
        res["update"].append(dict(members=variant, repeats=means, mean_us=sum(us) / len(us), spread_us=max(us) - min(us)))
    if not a.root:
        info, trace = _profiled("clone", ["work-clone", "--members", str(a.members), "--pairs", str(a.pairs)], a.out, None, a.limit)
        ns = [t for n, t in trace if n.startswith("pop_clone_members_kernel")]
        if len(ns) != 2:
            raise SystemExit(f"expected two clone launches in the trace, found {len(ns)}")
        for mode, t in zip(("keep", "copy"), ns):
            moved = 2 * info[f"bytes_copied_{mode}"]                 # read + written
            res[f"clone_{mode}"] = dict(pairs=a.pairs, us=t / 1e3, bytes_moved=moved, gb_per_s=moved / t,
                                        fraction_of_hbm=moved / t / a.hbm_gbs)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["work-update", "work-clone", "collect"])
    ap.add_argument("--members", type=int, default=256)
    ap.add_argument("--episodes", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--root", default=None)
    ap.add_argument("--out", default="build/sweep_probe")
    ap.add_argument("--limit", type=int, default=240, help="seconds allowed to each profiled child")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="peak HBM bandwidth the clone is set against (GB/s)")
    a = ap.parse_args()
    {"work-update": work_update, "work-clone": work_clone, "collect": collect}[a.what](a)


if __name__ == "__main__":
    main()
