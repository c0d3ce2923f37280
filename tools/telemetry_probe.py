#!/usr/bin/env python3
"""Telemetry of TrainPipeline (telemetry, telemetry_every; csrc/telemetry.hip) as measured: what the two launches cost a control
step, and what a healthy and a failing run look like in their columns.

    python tools/telemetry_probe.py time --parent-tree DIR [--B 512] [--rounds 4] [--windows 3] [--steps 2000] [--every 1 6]
    python tools/telemetry_probe.py watch [--episodes 30] [--B 64] [--print-every 3]

time: the protocol of tools/nstep_probe.py time -- the C2 shape (bench_C2(256): N = 256, 64 actuators, 3-layer nets), B = 512,
  51-step lock-stepped episodes, captured graphs; every configuration in worker PROCESSES of its own, one process at a time, the
  configurations alternating inside every round; a worker warms up, captures, runs `steps` untimed steps and then `windows` timed
  windows of `steps` control steps that end in a synchronise of every stream.  Configurations: the parent commit twice
  ("parent_a", "parent_b": a checkout of it with its library built, --parent-tree DIR; their difference is the noise of the
  method -- without DIR this tree constructed without the argument, "absent_a" / "absent_b"), telemetry = 0, and telemetry = 1024
  with every --every.  Median and spread over all windows per configuration, and the median's difference to the first reference in
  per cent.
watch: three short runs, B = 64, fp32, 51-step episodes from a new random field each, noise 0.3, graphs, frozen target networks --
  KS22 with the diagonal target (the configuration of tests/test_gpu_pipeline_learns.py, which learns), KS22 with the whole-batch
  reward broadcast (beats the zero action in one of three seeds), and the 1-D Keller-Segel setup, where frozen targets
  end in a saturated actor (README, the regime table) -- and per printed episode the episode means of the step columns and the
  last row of the update columns.
One JSON line per result on stdout."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "distributedconvrl-pde-control_amd"
E = 51


def _load(tree):
    sys.path.insert(0, tree)
    return importlib.import_module(PKG)


def _pipeline(pkg, setup, B, seed, y0=None, agent_kw=None, streams=None, **kw):
    import torch
    s_env, s_upd = streams if streams is not None else (torch.cuda.Stream(), torch.cuda.Stream())
    env = pkg.PDEenv(setup, B=B, dtype=torch.float32, y0=y0, stream=s_env, autoreset=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")            # (the other target regime: the setup's TargetNetworkWarning)
        agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(seed), dtype=torch.float32, stream=s_upd, start_steps=-1,
                                 noise_seed=7 + seed, trajectory_length=1, **(agent_kw or {}))
    agent.policy.act_noise = 0.3
    torch.cuda.synchronize()
    return pkg.TrainPipeline(env, agent, lag=2, episode_steps=E, stream_env=s_env, stream_upd=s_upd, use_graphs=True,
                             noise_seed=99 + seed, **kw)


def worker(a):
    """one configuration in a process of its own: warm-up, capture, then `windows` timed windows; one JSON line"""
    pkg = _load(a.tree)
    pkg._lib.init(0)
    s_env, s_upd = pkg._lib.make_streams((0, 0))
    setup = pkg.KSSetup.bench_C2(256)
    kw = {}
    if a.telemetry is not None:
        kw = dict(telemetry=a.telemetry, telemetry_every=a.telemetry_every)
    p = _pipeline(pkg, setup, a.B, 0, y0=setup.generate_random_init(np.random.default_rng(0), a.B) * 0.15, streams=(s_env, s_upd), **kw)
    p.run(5)
    p.capture()
    p.run(a.steps)
    p.sync()
    us = []
    for _ in range(a.windows):
        p.sync()
        t0 = time.perf_counter()
        p.run(a.steps)
        p.sync()
        us.append((time.perf_counter() - t0) * 1e6 / a.steps)
    rows = None
    if a.telemetry:
        tel = p.telemetry()
        rows = [len(tel["step"]["step"]) + tel["dropped_steps"], len(tel["update"]["update"]) + tel["dropped_updates"]]
    print(json.dumps(dict(us=us, graphs=len(p.graphs), rpart=p.rpart is not None, graph_launches=p.n_graph_launches,
                          eager_steps=p.n_eager_steps, rows=rows, cols=p.cols,
                          params=[p.policy.behavior_actor.model.num_params, p.policy.behavior_critic.model.num_params])), flush=True)
    p.close()


def timing(a):
    ref = ("parent", a.parent_tree) if a.parent_tree else ("absent", ROOT)
    configs = [(f"{ref[0]}_a", ref[1], None, 1), (f"{ref[0]}_b", ref[1], None, 1), ("telemetry_0", ROOT, 0, 1)]
    configs += [(f"telemetry_every_{m}", ROOT, 1024, m) for m in a.every]
    us = {c[0]: [] for c in configs}
    last = {}
    for _r in range(a.rounds):
        for name, tree, tel, m in configs:          # one process at a time: no two of them hold the device together
            cmd = [sys.executable, os.path.abspath(__file__), "worker", "--tree", tree, "--B", str(a.B), "--steps", str(a.steps),
                   "--windows", str(a.windows)]
            if tel is not None:
                cmd += ["--telemetry", str(tel), "--telemetry-every", str(m)]
            out = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, check=True, timeout=300).stdout
            last[name] = json.loads(out.strip().splitlines()[-1])
            us[name] += last[name]["us"]
    base = float(np.median(us[configs[0][0]]))
    for name, v in us.items():
        print(json.dumps(dict(probe="telemetry_time", config=name, B=a.B, us_median=float(np.median(v)), us_min=float(np.min(v)),
                              us_max=float(np.max(v)), pct_vs_first_reference=float(100 * (np.median(v) - base) / base),
                              processes=a.rounds, windows=a.windows, steps=a.steps, graphs=last[name]["graphs"],
                              reward_partials=last[name]["rpart"], graph_launches=last[name]["graph_launches"],
                              eager_steps=last[name]["eager_steps"], rows=last[name]["rows"], cols=last[name]["cols"],
                              params=last[name]["params"])), flush=True)


def watch(a):
    pkg = _load(ROOT)
    pkg._lib.init(0)
    runs = (("ks22_frozen_diagonal", pkg.KSSetup.KS22(), dict(quirk_target_broadcast=False), "learns"),
            ("ks22_frozen_broadcast", pkg.KSSetup.KS22(), {}, "beats the zero action in one of three seeds"),
            ("kseg_frozen", pkg.KellerSegelSetup(), {}, "saturated actor"))
    for name, setup, agent_kw, known in runs:
        n = a.episodes * E
        y0 = setup.generate_random_init(np.random.default_rng(0), a.B) * 0.15 if name.startswith("ks22") else None
        p = _pipeline(pkg, setup, a.B, 0, y0=y0, agent_kw=dict(agent_kw, quirk_frozen_targets=True), log_episodes=a.episodes,
                      random_init=True, init_seed=1, telemetry=n)
        p.run(5)
        p.capture()
        p.run(n - p.tick)
        p.sync()
        tel = p.telemetry()
        st, up = tel["step"], tel["update"]
        returns = p.rewards
        # update u was issued at control step u + 2 (lag 2): the last update row of episode e is that of its last step
        for e in range(a.episodes):
            if e % a.print_every and e != a.episodes - 1:
                continue
            sl = slice(e * E, (e + 1) * E)
            u = (e + 1) * E - 1 - 2
            print(json.dumps(dict(
                probe="telemetry_watch", run=name, readme_says=known, episode=e + 1, episode_return=float(returns[e]),
                reward_mean=float(np.nanmean(st["reward_mean"][sl])), reward_min=float(np.nanmin(st["reward_min"][sl])),
                action_abs_mean=float(st["action_abs_mean"][sl].mean()),
                action_saturated_fraction=float(st["action_saturated_fraction"][sl].mean()),
                state_abs_max=float(st["state_abs_max"][sl].max()), blown_up=float(st["blown_up"][sl].sum()),
                critic_loss=float(up["critic_loss"][u]), actor_loss=float(up["actor_loss"][u]),
                actor_norm2=float(up["actor_norm2"][u]), critic_norm2=float(up["critic_norm2"][u]),
                actor_target_dist2=float(up["actor_target_dist2"][u]), critic_target_dist2=float(up["critic_target_dist2"][u]),
                actor_step2=float(up["actor_step2"][u]), critic_step2=float(up["critic_step2"][u]),
                actor_abs_max=float(up["actor_abs_max"][u]), critic_abs_max=float(up["critic_abs_max"][u]))), flush=True)
        print(json.dumps(dict(probe="telemetry_watch", run=name, summary=True, first_nonfinite_step=tel["first_nonfinite_step"],
                              first_nonfinite_update=tel["first_nonfinite_update"], dropped_steps=tel["dropped_steps"],
                              graph_launches=p.n_graph_launches)), flush=True)
        p.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("time", "watch", "worker"))
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--telemetry", type=int, default=None)
    ap.add_argument("--telemetry-every", type=int, default=1)
    ap.add_argument("--every", type=int, nargs="+", default=[1, 6])
    ap.add_argument("--B", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--episodes", type=int, default=30)
    ap.add_argument("--print-every", type=int, default=3)
    a = ap.parse_args()
    if a.B is None:
        a.B = 64 if a.mode == "watch" else 512
    {"time": timing, "watch": watch, "worker": worker}[a.mode](a)


if __name__ == "__main__":
    main()
