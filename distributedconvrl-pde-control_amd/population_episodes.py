"""The episode machinery of a Population: what the host-settled path (`run_episode`: one read-back per episode) and the block path
(population_blocks.py: the episode boundary on the device) share.

The control steps of an episode are issued as in run._run_device_episodes, but each of the three per-step launches -- the glue
(POST_ACT push, acting, PRE_ACT push), the small update, the env step -- is ONE launch of M workgroups: workgroup m reads member
m's pointers from a device table and its counters from row m of the counter table (population_slots.py).  The glue and the update
run on the networks' stream, the member-layout env step on the environment's; two events hand a step over (`issue_steps`, the one
statement of that protocol).  On the host-settled path the table is written once per episode and read back once, and every member's
host state is settled exactly as the solo loop settles it at its number of executed steps."""
import time

import numpy as np
import torch

from . import _lib
from .agent import PRE_EPISODE_STAGE
from .env import _on_stream
from .pipeline import _Event
from .population_slots import SAMPLE, counter_rows
from .run import (_EpisodeLogs, _add_episode_reward, _episode_schedule, _episode_steps, _episode_time, _executed_steps, _join,
                  _stop_fired)


class _MemberEnv:
    """what a member's hook sees of the population's environment at the end of its episode of n steps"""

    def __init__(self, env, m, n):
        self.setup, self.te, self.dt, self.is_fluid = env.setup, env.te, env.dt, env.is_fluid
        self.stream, self.B = env.stream, 1
        self.y = env.y[m:m + 1]
        self.time = _episode_time(env.dt, n)


def episode_buffers(pop, T):
    """(logs, flags): the per-step slots of one episode of T steps (run._EpisodeLogs at B = M) and the members' done flags per
    step [T, M], made once and kept from episode to episode"""
    if pop._logs is None or pop._logs.T != T:
        with _on_stream(pop.stream_env):
            pop._logs = _EpisodeLogs(pop.env, T)
            pop._flags = torch.zeros((T, pop.M), dtype=torch.int32, device=pop.env.device)
    return pop._logs, pop._flags


def upload_rows(pop, active):
    """the counter table of an episode's start, from the agents as they stand: written, completed by the library (BPA / BPC)
    and uploaded; returns the host table"""
    rows = counter_rows(pop.agents, active, pop._hyper_rows())
    _lib.check(pop.lib.pdec_population_bp_sel(pop._h, _lib.ptr(rows), 0))
    with _on_stream(pop.stream_upd):
        pop.rows.copy_(torch.from_numpy(rows))
    return rows


def issue_steps(pop, logs, flags, ev_act, ev_env):
    """the T control steps of one episode from the environment as it stands, and the time-out push.  Per step: the
    member-indexed glue and update on the networks' stream, the member-layout env step on the environment's; ev_act hands the
    step's actions to the environment, ev_env its outcome back to the networks."""
    env, lib, h, T = pop.env, pop.lib, pop._h, logs.T
    s_env, s_upd = pop.stream_env, pop.stream_upd
    P = _lib.ptr
    with _on_stream(s_env):
        logs.y[0].copy_(env.y)
        logs.state[0].copy_(env.state)
        flags.zero_()
    _join(s_upd, s_env)
    for t in range(T):
        _lib.check(lib.pdec_population_glue(h, 0, P(logs.reward[t - 1]) if t else None, P(flags[t - 1]) if t else None,
                                            P(logs.state[t]), P(logs.action[t + 1])))
        ev_act.record(s_upd)
        ev_act.wait(s_env)
        _lib.check(lib.pdec_population_update(h))
        _lib.check(lib.pdec_env_step(env.handle, P(logs.y[t]), P(logs.action[t + 1]), P(logs.action[t]), P(logs.state[t]),
                                     P(logs.y[t + 1]), P(logs.p[t]), P(logs.state[t + 1]), P(logs.reward[t]), P(flags[t])))
        ev_env.record(s_env)
        ev_env.wait(s_upd)
    _lib.check(lib.pdec_population_glue(h, 1, P(logs.reward[T - 1]), P(flags[T - 1]), None, None))   # the time-out push


def step_means(pop, logs):
    """[M * T] on the networks' stream: the per-step episode reward of PDEhook (mean over the actuators), member-major rows as a
    B = 1 run reduces them"""
    with _on_stream(pop.stream_upd):
        return logs.reward.transpose(0, 1).contiguous().reshape(pop.M * logs.T, -1).mean(dim=1)


# ---- the opening of an episode

def ic_case(setup):
    """generate_random_init's case (FluidSetup.jl:386-394): ic(4) in evaluation, ic(3) in training"""
    return 4 if setup.evaluation else 3


def _per_member(mask, like):
    """a mask [M] shaped to select whole members of `like` [M, ...]"""
    return mask.view((mask.shape[0],) + (1,) * (like.dim() - 1))


def open_episode(pop, act, rnd, source):
    """env.reset(); the members of `rnd` then start from a random field of their own -- all fields drawn in one launch from
    `source`, the fluid's vortex tables [M, nv, 4] or the others' Philox (seeds [M], offsets [M]) -- with their states sensed anew,
    the others keeping their reset state as their solo hooks leave it; the members outside `act` keep the y and state they had.
    act, rnd: device bool masks [M] -- on the host-settled path from the host's lists, on the block path from the device columns
    -- or None: every member is active / none draws.  (`source`'s tensors were made with the environment's stream current: the
    caching allocator's stream order keeps them alive.)"""
    env, lib = pop.env, pop.lib
    with _on_stream(pop.stream_env):
        keep = None if act is None else (env.y.clone(), env.state.clone())
    env.reset()
    with _on_stream(pop.stream_env):
        if rnd is not None:
            drawn = torch.empty_like(env.y)
            if pop.is_fluid:
                _lib.check(lib.pdec_fluid_ic_dev(env.handle, _lib.ptr(source), int(source.shape[-2]), _lib.ptr(drawn)))
            else:
                _lib.check(lib.pdec_env_random_init_members(env.handle, _lib.ptr(source[0]), _lib.ptr(source[1]), _lib.ptr(drawn)))
            y0 = torch.where(_per_member(rnd, env.y), drawn, env.y0)
            env.y0 = y0
            env.y.copy_(y0)
            st = env.featurize(env.y, env.state if env.setup.temporal_steps > 1 else None)
            env.state.copy_(torch.where(_per_member(rnd, env.state), st, env.state))
            env._state0.copy_(env.state)
        if keep is not None:
            env.y.copy_(torch.where(_per_member(act, env.y), env.y, keep[0]))
            env.state.copy_(torch.where(_per_member(act, env.state), env.state, keep[1]))


def _open_from_host(pop, active):
    """open_episode with the masks and the draws' source from the host: the active members whose hooks use random inits draw,
    the fluid's from their own generators as their solo hooks do (one upload), the others from their hooks' Philox offsets,
    which move on"""
    from .population_blocks import draw_block_tables
    env, hooks = pop.env, pop.hooks
    draws = active & np.array([bool(hk.use_random_init) for hk in hooks])
    act = rnd = source = None
    with _on_stream(pop.stream_env):
        if not active.all():
            act = torch.from_numpy(active.copy()).to(env.device)
        if draws.any():
            rnd = torch.from_numpy(draws).to(env.device)
            if pop.is_fluid:
                tables, _ = draw_block_tables(pop.setup, [hk.init_rng if d else None for hk, d in zip(hooks, draws)], 1,
                                              ic_case(pop.setup))
                source = torch.from_numpy(tables[0]).to(env.device)
            else:
                seed_off = [[hk.init_seed if d else 0 for hk, d in zip(hooks, draws)],
                            [hk._init_off if d else 0 for hk, d in zip(hooks, draws)]]
                source = torch.tensor(seed_off, dtype=torch.int64).to(env.device)
                nblk = (env.random_init_coefficients() + 3) // 4
                for m in np.flatnonzero(draws):
                    hooks[m]._init_off += nblk
    open_episode(pop, act, rnd, source)


# ---- the host-settled episode

def run_episode(pop, active, stops):
    """one episode of every active member: opened, issued, read back once, and every member settled on the host"""
    env, M, lib, cols = pop.env, pop.M, pop.lib, pop.cols
    s_env, s_upd = pop.stream_env, pop.stream_upd
    P = _lib.ptr
    t0 = time.perf_counter()
    _open_from_host(pop, active)
    for m in np.flatnonzero(active):
        pop.agents[m](PRE_EPISODE_STAGE, env)           # host counters only (pop_sa)
    T = _episode_steps(env)
    logs, flags = episode_buffers(pop, T)
    start = upload_rows(pop, active)
    ev_act, ev_env = _Event(lib), _Event(lib)        # (held to the episode's end)
    issue_steps(pop, logs, flags, ev_act, ev_env)
    means = step_means(pop, logs)
    with _on_stream(s_upd):
        pack = torch.cat([pop.rows.view(-1).view(torch.uint8), flags.view(-1).view(torch.uint8), means.view(-1).view(torch.uint8)])
        t1 = time.perf_counter()
        host = pack.cpu().numpy()                                          # the one read-back (bytes)
    t2 = time.perf_counter()
    nr, nf = pop.rows.numel() * 8, flags.numel() * 4
    rows_out = host[:nr].copy().view(np.int64).reshape(pop.rows.shape)
    fl = host[nr:nr + nf].copy().view(np.int32).reshape(T, M)
    mean_h = host[nr + nf:].copy().view(np.float64).reshape(M, T)
    # ---- settle every member at its number of executed steps
    n_of = np.array([_executed_steps(fl[:, m], T) if active[m] else 0 for m in range(M)], dtype=np.int64)
    pop.episode_steps.append(n_of.copy())
    pol0, tr0 = pop.agents[0].policy, pop.agents[0].trajectory
    sched = _episode_schedule(start[:, :SAMPLE + 1], T, cols, pol0.behavior_actor.model.dims[-1], tr0.capacity, tr0.stride,
                              pol0.update_after, pol0.update_freq, pol0.update_loops, pol0.batch_size, pol0.start_steps)
    _lib.check(lib.pdec_population_bp_sel(pop._h, P(rows_out), 1))
    with _on_stream(s_env):
        ii = torch.as_tensor(n_of, device=env.device)
        ar = torch.arange(M, device=env.device)
        env.y = logs.y[ii, ar].contiguous()
        env.state = logs.state[ii, ar].contiguous()
    # POST_EPISODE push of the final states with the zero action (active members; one launch)
    s_upd.wait_stream(s_env)
    _lib.check(lib.pdec_population_glue(pop._h, 2, None, None, P(env.state), None))
    was = np.flatnonzero(active)
    if any(pop.hooks[m].collect_bestDF for m in was):
        with _on_stream(s_env):
            la, lp, ly, lr = (x.cpu() for x in (logs.action, logs.p, logs.y, logs.reward))
    which = np.zeros(M, dtype=np.int32)
    for m in was:
        ag, hk, n = pop.agents[m], pop.hooks[m], int(n_of[m])
        pol, tr = ag.policy, ag.trajectory
        counters = rows_out[m, :SAMPLE + 1].tolist()
        if counters != sched.after[m, n - 1].tolist():
            raise RuntimeError(f"Population: member {m}'s device counters disagree with its {n} executed steps")
        pol.update_step, tr.n_sa, tr.n_rt, pol._noise_off, pol._sample_off = counters
        _add_episode_reward(hk, mean_h[m, :n], np.float64)
        if hk.collect_bestDF:
            hk._rows_bulk = (list(range(1, n + 1)), la[1:n + 1, m], lp[:n, m], ly[1:n + 1, m], lr[:n, m])
        fired = _stop_fired(stops[m], ag, n)
        ag.end_episode(env.state[m], pushed=True)          # POST_EPISODE: its push went out above, one launch for all
        with _on_stream(s_env):
            new_best = hk.end_episode(_MemberEnv(env, m, n))
        which[m] = (1 if new_best else 0) | (2 if hk.collect_NNA else 0)
        if fired:
            active[m] = False
    if which.any():                                        # the hooks' best / current actor copies: one launch
        with _on_stream(s_upd):
            pop._which.copy_(torch.from_numpy(which))
        _lib.check(lib.pdec_population_copy_actors(pop._h, P(pop._which)))
    s_env.wait_stream(s_upd)
    add_timing(pop, 1, t0, t1, t2, time.perf_counter())


def add_timing(pop, episodes, t0, t1, t2, t3):
    """host seconds per phase of one read-back: issue = initialisers + every enqueue up to it, readback = waiting for the device,
    settle = the members' host bookkeeping and the boundary launches"""
    tm = pop.timing
    tm["episodes"] += episodes
    tm["blocks"] = tm.get("blocks", 0) + 1
    tm["issue_s"] += t1 - t0
    tm["readback_s"] += t2 - t1
    tm["settle_s"] += t3 - t2
