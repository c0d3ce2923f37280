"""Blocks of episodes (Population.run(stops, episodes_per_sync = E > 1)): up to E whole episodes enqueued per read-back.

The episode boundary -- hook, stop condition, counters, the next initial field -- is decided on the device
(pdec_population_episode_close) from each member's book (population_slots.py), and the members' host state is settled once per
block from the device's episode log; every member ends bit for bit where E = 1 leaves it.  A block is as long as its neediest
active member can still need (block_length), so that no episode of a block is idle for every member.  Fluid members draw their
vortex tables for the whole block on the host, each from its own generator, which is set back afterwards to what the member
consumed; where their hooks hold the setup's own error_detection, its device form runs behind every episode's close launch."""
import time

import numpy as np
import torch

from . import _lib
from .agent import PRE_EPISODE_STAGE, POST_EPISODE_STAGE
from .env import _on_stream
from .pipeline import _Event
from .population_episodes import add_timing, episode_buffers, ic_case, issue_steps, open_episode, step_means, upload_rows
from .population_slots import (ROW, BOOK, ELOG, USTEP, NSA, NRT, SAMPLE, ACTIVE, BK_EP, BK_BESTREWARD, BK_BESTEPISODE, BK_STOP_CUR,
                               BK_RANDOM_INIT, BK_INIT_SEED, BK_INIT_OFF, EL_REWARD, EL_STEPS, EL_NEW_BEST, EL_RAN, book_rows,
                               python_max_state)  # noqa: F401  (python_max_state: the carried max() of the book, reached from here)
from .run import StopAfterEpisode, StopAfterEpisodeWithMinSteps, _episode_schedule, _episode_steps, _join


# ---- how many episodes a member can still need (pure host logic)

def episodes_still_needed(stop, T):
    """the least number of episodes of at most T control steps after which `stop` (a StopAfterEpisode or
    StopAfterEpisodeWithMinSteps as run.py writes them, in its current state) can have fired; at least 1"""
    if type(stop) is StopAfterEpisode:          # cur += 1 per episode end, fires at cur >= episode
        return max(1, int(stop.episode) - int(stop.cur))
    if type(stop) is StopAfterEpisodeWithMinSteps:      # cur += 1 per step, fires at an episode end that begins with cur >= step
        need = int(stop.step) - int(stop.cur) + 1       # steps until the call that can fire, that call included
        return max(1, -(-need // int(T)))
    raise TypeError(f"episodes_still_needed: {type(stop).__name__}")


def block_length(stops, active, T, E):
    """episodes of the next block: min(E, max over the active members of episodes_still_needed), so that no episode of a block
    is idle for every member"""
    return min(int(E), max(episodes_still_needed(s, T) for s, a in zip(stops, active) if a))


# ---- fluid members: the vortex tables of a block of episodes, and what the episode logs cost (pure host logic)

def draw_block_tables(setup, rngs, L, caseno):
    """The initial vortex tables of up to L episodes for each member: rngs[m] is member m's own init_rng, or None for a member
    that draws none (idle, or without random inits).  Member m's e-th table is the e-th successive
    setup.ic_vortices(caseno, rngs[m], 1) of its generator, as its solo hook draws one per episode.  Returns (tables
    [L, M, nv, 4] -- ones where nothing was drawn --, states): states[m] = [the generator's state before the first draw, the state
    behind draw 1, ..., behind draw L], or None."""
    tables, states = None, []
    for m, rng in enumerate(rngs):
        if rng is None:
            states.append(None)
            continue
        st = [rng.bit_generator.state]
        for e in range(int(L)):
            v = setup.ic_vortices(caseno, rng, 1)[0]
            if tables is None:              # (the table's length is ic_vortices' own)
                tables = np.ones((int(L), len(rngs)) + v.shape, dtype=np.float64)
            tables[e, m] = v
            st.append(rng.bit_generator.state)
        states.append(st)
    if tables is None:
        tables = np.ones((int(L), len(rngs), 1, 4), dtype=np.float64)
    return tables, states


def restore_block_rngs(rngs, states, consumed):
    """after a block: member m's generator goes back to the state behind the last table it consumed (consumed[m] of the L drawn),
    so a member that stopped inside the block has advanced its generator exactly as far as its solo run has"""
    for rng, st, k in zip(rngs, states, consumed):
        if rng is not None and st is not None:
            rng.bit_generator.state = st[int(k)]


def episode_log_bytes(setup, T, itemsize=8):
    """(logs, best_rows) bytes PER MEMBER of a population's per-step slots of one episode of T control steps (run._EpisodeLogs:
    y, state and action T + 1 slots, p and reward T) and of the best episode's rows the block path keeps on the device
    (action, p, y, reward: T slots each).  A fluid field is a complex spectrum (two reals per cell); p has the field's shape."""
    fluid = bool(getattr(setup, "is_fluid", False))
    y = int(np.prod(setup.y_shape)) * (2 if fluid else 1)
    p = y if fluid else int(np.prod(getattr(setup, "p_shape", (setup.nx,))))
    ns, A = setup.state_shape
    a = int(np.prod(setup.action_shape))
    r = int(setup.reward_len)
    logs = (int(T) + 1) * (y + ns * A + a) + int(T) * (p + r)
    best = int(T) * (a + p + y + r)
    return logs * int(itemsize), best * int(itemsize)


# ---- a block: allocate, write the tables, enqueue, read back, settle

def own_error_detection(pop, hk):
    """is the hook's error_detection FluidSetup.error_detection of this population's own setup (what make_hook() sets)?  The
    block path then runs its device form (pdec_fluid_error_detection) behind every episode's close launch"""
    f = hk.error_detection
    return (pop.is_fluid and getattr(f, "__self__", None) is pop.setup
            and getattr(f, "__func__", None) is getattr(type(pop.setup), "error_detection", None))


def _allocate(pop, logs, L, want_rows):
    """the block's device buffers, kept from block to block: the book, the episode log of L episodes, the best episodes' rows
    (where a hook collects them) and the fluid's error flags err[e, m] (zeroed)"""
    M, T, dev = pop.M, logs.T, pop.env.device
    with _on_stream(pop.stream_upd):
        if pop._elog is None or pop._elog.shape[0] < L:
            pop._book = torch.zeros((M, BOOK), dtype=torch.int64, device=dev)
            pop._elog = torch.zeros((L, M, ELOG), dtype=torch.int64, device=dev)
        if want_rows and (pop._best_rows is None or pop._best_rows[0].shape[1] != T):
            pop._best_rows = tuple(torch.zeros((M, T) + tuple(x.shape[2:]), dtype=x.dtype, device=dev)
                                   for x in (logs.action, logs.p, logs.y, logs.reward))
    if pop.is_fluid:
        with _on_stream(pop.stream_env):
            if pop._err is None or pop._err.shape[0] < L:
                pop._err = torch.zeros((L, M), dtype=torch.int32, device=dev)
            pop._err.zero_()


def _write_tables(pop, active, stops):
    """the counter table and the book of the block's start (one upload each); returns the host tables"""
    start = upload_rows(pop, active)
    book = book_rows(pop.hooks, stops, None if pop.is_fluid else (pop.env.random_init_coefficients() + 3) // 4)
    with _on_stream(pop.stream_upd):
        pop._book.copy_(torch.from_numpy(book))
    return start, book


def _draw_tables(pop, active, L):
    """the vortex tables of the whole block from the members' own generators (one upload); the generators are set back to what
    each member consumed when the block is settled.  Returns (device tables [L, M, nv, 4], generators, their states)"""
    rngs = [hk.init_rng if (a and hk.use_random_init) else None for a, hk in zip(active, pop.hooks)]
    tab, states = draw_block_tables(pop.setup, rngs, L, ic_case(pop.setup))
    with _on_stream(pop.stream_env):
        return torch.from_numpy(tab).to(pop.env.device), rngs, states


def _enqueue(pop, L, logs, flags, any_random, tables, want_rows, detect, reset_post):
    """L episodes, each opened from the device columns, issued, and closed on the device"""
    env, lib, h, T = pop.env, pop.lib, pop._h, logs.T
    s_env, s_upd = pop.stream_env, pop.stream_upd
    P = _lib.ptr
    book, which = pop._book, pop._which
    ysz, ssz = env.y[0].numel(), env.state[0].numel()
    ev_act, ev_env = _Event(lib), _Event(lib)
    for e in range(L):
        _join(s_upd, s_env)
        with _on_stream(s_env):
            act = pop.rows[:, ACTIVE] != 0
            rnd = source = None
            if any_random:
                rnd = act & (book[:, BK_RANDOM_INIT] != 0)
                source = tables[e] if pop.is_fluid else (book[:, BK_INIT_SEED].contiguous(), book[:, BK_INIT_OFF].contiguous())
        open_episode(pop, act, rnd, source)
        issue_steps(pop, logs, flags, ev_act, ev_env)
        # ---- the boundary, all on the networks' stream: close (hook, stop rule, final y / state), the POST_EPISODE push of
        # the final states, the best episode's rows, the hooks' actor copies, then the counters of the next episode
        means = step_means(pop, logs)
        close = (P(pop._elog[e]), P(flags), P(means), T, P(logs.y), P(logs.state), P(env.y), P(env.state), ysz, ssz, P(which),
                 reset_post, int(e == L - 1))
        _lib.check(lib.pdec_population_episode_close(h, 0, P(book), *close))
        _lib.check(lib.pdec_population_glue(h, 2, None, None, P(env.state), None))
        if want_rows:
            la, lp, ly, lr = logs.action, logs.p, logs.y, logs.reward
            _lib.check(lib.pdec_population_copy_best_rows(
                h, P(which), P(pop._elog[e]), T, P(la), P(lp), P(ly), P(lr), *[P(b) for b in pop._best_rows],
                la[0, 0].numel(), lp[0, 0].numel(), ly[0, 0].numel(), lr[0, 0].numel()))
        _lib.check(lib.pdec_population_copy_actors(h, P(which)))
        _lib.check(lib.pdec_population_episode_close(h, 1, P(book), *close))
        if detect:
            # on the environment's stream, behind the close launch (which wrote env.y) and before the next initialiser
            s_env.wait_stream(s_upd)
            _lib.check(lib.pdec_fluid_error_detection(env.handle, P(env.y), P(pop._err[e])))


def _read_back(pop, L):
    """the one read-back of a block, and the one place that knows its packed layout: rows [M, ROW], book [M, BOOK], the episode
    log [L, M, ELOG] and, for the fluid, err [L, M] as int64s.  Returns (rows, book, elog, err or None, the host clock before
    and behind the wait)"""
    M = pop.M
    if pop.is_fluid:
        pop.stream_upd.wait_stream(pop.stream_env)
    with _on_stream(pop.stream_upd):
        parts = [pop.rows.view(-1), pop._book.view(-1), pop._elog[:L].reshape(-1)]
        if pop.is_fluid:
            parts.append(pop._err[:L].reshape(-1).to(torch.int64))
        pack = torch.cat(parts)
        t1 = time.perf_counter()
        host = pack.cpu().numpy()
    t2 = time.perf_counter()
    pop.stream_env.wait_stream(pop.stream_upd)
    rows, book, elog, err = np.split(host, np.cumsum([M * ROW, M * BOOK, L * M * ELOG]))
    return (rows.reshape(M, ROW).copy(), book.reshape(M, BOOK), elog.reshape(L, M, ELOG),
            err.reshape(L, M) if pop.is_fluid else None, t1, t2)


def _replay_counters(pop, start, elog, ran, reset_post):
    """[M, 5]: the counters every member must end the block with -- the schedule of each episode at its logged number of steps,
    with the boundary movements between them; every episode's steps are noted in pop.episode_steps"""
    pol0, tr0 = pop.agents[0].policy, pop.agents[0].trajectory
    L, T = elog.shape[0], pop._logs.T
    cur = start[:, :SAMPLE + 1].copy()
    for e in range(L):
        n_of = elog[e, :, EL_STEPS].copy()
        pop.episode_steps.append(n_of)
        idx = np.flatnonzero(ran[e])
        sched = _episode_schedule(cur, T, pop.cols, pol0.behavior_actor.model.dims[-1], tr0.capacity, tr0.stride, pol0.update_after,
                                  pol0.update_freq, pol0.update_loops, pol0.batch_size, pol0.start_steps)
        cur[idx] = sched.after[idx, n_of[idx] - 1]
        cur[idx, NSA] += pop.cols                           # POST_EPISODE: the final state with the zero action
        if reset_post:
            cur[idx, USTEP] = 0
        if e + 1 < L:                                       # PRE_EPISODE pop of the members that go on
            go = idx[ran[e + 1, idx] & (cur[idx, NSA] > cur[idx, NRT])]
            cur[go, NSA] -= tr0.stride
    return cur


def _settle_member(pop, m, stop, counters, bk, elog_m, err_m):
    """member m's agent, hook and stop condition behind the block, from its counters, its book row bk, its column of the
    episode log and of the error flags (None: no device error detection).  Returns the steps of its last new best episode whose
    rows its hook collects, or None"""
    ag, hk, T = pop.agents[m], pop.hooks[m], pop._logs.T
    pol, tr = ag.policy, ag.trajectory
    pol.update_step, tr.n_sa, tr.n_rt, pol._noise_off, pol._sample_off = counters
    rewards = elog_m[:, EL_REWARD].copy().view(np.float64)
    for e in np.flatnonzero(elog_m[:, EL_RAN]):
        r = float(rewards[e])
        if elog_m[e, EL_STEPS] == T and hk.ep >= hk.min_best_episode:
            hk.rewards_compare.append(r)
        # PDEhook.end_episode: an episode that ended early and is errored, noted before ep advances
        if err_m is not None and elog_m[e, EL_STEPS] < T and err_m[e] and own_error_detection(pop, hk):
            hk.errored_episodes.append(hk.ep)
        hk.rewards.append(r)
        hk.ep += 1
    if hk.ep != int(bk[BK_EP]):
        raise RuntimeError(f"Population: member {m}'s device episode index disagrees with its episode log")
    hk.bestreward = float(bk[BK_BESTREWARD:BK_BESTREWARD + 1].view(np.float64)[0])
    hk.bestepisode = int(bk[BK_BESTEPISODE])
    stop.cur = int(bk[BK_STOP_CUR])
    if not pop.is_fluid:
        hk._init_off = int(bk[BK_INIT_OFF])
    best_e = np.flatnonzero(elog_m[:, EL_NEW_BEST])
    return int(elog_m[best_e[-1], EL_STEPS]) if best_e.size and hk.collect_bestDF else None


def _flush_best_rows(pop, changed):
    """the best episodes' rows of the members in `changed` [(m, steps)], through the hook's own row path"""
    with _on_stream(pop.stream_upd):
        ii = torch.as_tensor([m for m, _ in changed], device=pop.env.device)
        ba, bp, by, br = (b.index_select(0, ii).cpu() for b in pop._best_rows)
    for j, (m, n) in enumerate(changed):
        hk = pop.hooks[m]
        hk._rows_bulk = (list(range(1, n + 1)), ba[j, :n], bp[j, :n], by[j, :n], br[j, :n])
        hk._flush(pop.env)
        hk.bestDF, hk.currentDF = list(hk.currentDF), []


def run_block(pop, active, stops, L):
    """L whole episodes enqueued, one read-back, every member settled for the block"""
    t0 = time.perf_counter()
    logs, flags = episode_buffers(pop, _episode_steps(pop.env))
    was = np.flatnonzero(active)
    want_rows = any(pop.hooks[m].collect_bestDF and pop.hooks[m].collect_NNA for m in was)
    _allocate(pop, logs, L, want_rows)
    for m in was:                                           # PRE_EPISODE of the block's first episode is the host's
        pop.agents[m](PRE_EPISODE_STAGE, pop.env)           # host counters only (pop_sa)
    start, book = _write_tables(pop, active, stops)
    any_random = bool(book[:, BK_RANDOM_INIT].any())
    tables, rngs, rng_states = _draw_tables(pop, active, L) if pop.is_fluid and any_random else (None, None, None)
    detect = pop.is_fluid and any(own_error_detection(pop, pop.hooks[m]) for m in was)
    reset_post = int(pop.agents[0].policy.reset_stage == POST_EPISODE_STAGE)
    _enqueue(pop, L, logs, flags, any_random, tables, want_rows, detect, reset_post)
    rows_out, book_out, elog, err, t1, t2 = _read_back(pop, L)
    # ---- settle every member for the whole block: the replayed counters must end at the device's
    ran = elog[:, :, EL_RAN] != 0
    if not (ran[0] == active).all() or (ran[1:] & ~ran[:-1]).any():
        raise RuntimeError("Population: the device's episode log disagrees with the members that were active")
    cur = _replay_counters(pop, start, elog, ran, reset_post)
    for m in was:
        if cur[m].tolist() != rows_out[m, :SAMPLE + 1].tolist():
            raise RuntimeError(f"Population: member {m}'s device counters disagree with its executed steps of the block")
    _lib.check(pop.lib.pdec_population_bp_sel(pop._h, _lib.ptr(rows_out), 1))
    changed = []
    for m in was:
        n_best = _settle_member(pop, m, stops[m], rows_out[m, :SAMPLE + 1].tolist(), book_out[m], elog[:, m],
                                None if err is None else err[:, m])
        if n_best is not None:
            changed.append((m, n_best))
        if not rows_out[m, ACTIVE]:
            active[m] = False
    if rngs is not None:
        restore_block_rngs(rngs, rng_states, ran.sum(axis=0))
    if changed:
        _flush_best_rows(pop, changed)
    add_timing(pop, L, t0, t1, t2, time.perf_counter())
