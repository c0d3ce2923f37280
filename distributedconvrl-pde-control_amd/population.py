"""Populations: M independently seeded reference-shaped learners trained side by side on one GPU.

Every member is an ordinary `Agent` (create_agent(setup=..., B=1, stream=s_upd)) with its own `PDEhook`; `Population.run`
leaves each of them bit for bit where `run(agent_m, PDEenv(setup, B=1, ...), stops[m], hook_m)` leaves it.  The control steps
of an episode are issued as in run._run_device_episodes, but each of the three per-step launches -- the glue (POST_ACT push,
acting, PRE_ACT push), the small update, the env step -- is ONE launch of M workgroups: workgroup m reads member m's pointers
from a device table and its counters (ring positions, Philox offsets, update_step, halt flag) from row m of a device int64
table (include/pdeconv.h, pdec_population_create).  The host writes that table once per episode, reads it back once, and
settles each member's host state exactly as the solo loop does at its number of executed steps.

Members may differ in their hyper-parameters (gamma, Polyak rho, the two learning rates, act_noise, act_limit): the agents' own
attributes are read into the row table of every episode, so a sweep is M agents created with different values, and a change
between two `run` calls takes effect as it does in a solo run.  `Population.clone` copies a member's learner into others in one
launch, and `Population.exploit` applies it to an evaluation's ranking (population-based selection: the worst members take
over the best members' learners and go on with perturbed hyper-parameters)."""
import ctypes as C
import time

import numpy as np
import torch

from . import _lib
from .agent import Agent, PRE_EXPERIMENT_STAGE, PRE_EPISODE_STAGE, POST_EPISODE_STAGE, POST_EXPERIMENT_STAGE
from .env import PDEenv, _on_stream
from .hook import PDEhook
from .pipeline import _Event
from .pipeline_eval import held_out_fields
from .run import (StopAfterEpisode, StopAfterEpisodeWithMinSteps, _EpisodeLogs, _add_episode_reward, _episode_schedule,
                  _episode_steps, _episode_time, _executed_steps, _join, _stop_fired, device_episodes_ok)

# a member's row of the device counter table: POP_ROW and enum PopSlot of csrc/population.hpp (tests/test_host_logic.py compares them)
ROW = 16
USTEP, NSA, NRT, NOISE, SAMPLE, HALT, ACTIVE, BPA, BPC, NOISE_AMP, LIMIT = range(11)
# a member's own gamma, rho and ADAM step sizes (bit patterns of doubles): enum PopHyperSlot of csrc/population.hpp; slot 15 is free
GAMMA, RHO, ETA_A, ETA_C = range(11, 15)
# a member's book -- what its hook and its stop condition hold between two episodes -- and the episode log of a block:
# POP_BOOK / enum PopBookSlot and POP_ELOG / enum PopElogSlot of csrc/population.hpp (tests/test_population_blocks_host.py compares them)
BOOK = 16
(BK_EP, BK_MIN_BEST, BK_COLLECT_NNA, BK_CMP_HAS, BK_CMP, BK_BESTREWARD, BK_BESTEPISODE, BK_STOP_KIND, BK_STOP_CUR, BK_STOP_LIMIT,
 BK_RANDOM_INIT, BK_INIT_SEED, BK_INIT_OFF, BK_INIT_INC, BK_FIRED, BK_SPARE) = range(BOOK)
ELOG = 4
EL_REWARD, EL_STEPS, EL_NEW_BEST, EL_RAN = range(ELOG)
HYPER_KEYS = ("gamma", "rho", "actor_lr", "critic_lr", "act_noise", "act_limit")
PERTURBED = ("actor_lr", "critic_lr", "act_noise")      # what exploit's perturbation multiplies


class _MemberEnv:
    """what a member's hook sees of the population's environment at the end of its episode of n steps"""

    def __init__(self, env, m, n):
        self.setup, self.te, self.dt, self.is_fluid = env.setup, env.te, env.dt, env.is_fluid
        self.stream, self.B = env.stream, 1
        self.y = env.y[m:m + 1]
        self.time = _episode_time(env.dt, n)


def _refuse(msg):
    raise _lib.PdecError("Population: " + msg)


# ---- blocks of episodes: how many a member can still need, and Python's max() as a carried state (pure host logic)

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


def python_max_state(values):
    """(has, cmp) of Python's max(values) carried element by element: the first element unless a later one compares greater
    (a NaN that comes first stays; a later NaN never replaces)"""
    has, cmp = 0, 0.0
    for v in values:
        if not has:
            has, cmp = 1, v
        elif v > cmp:
            cmp = v
    return has, float(cmp)


# ---- evaluation: every member's actor scored on the SAME held-out initial fields, in one launch where the library serves it

def member_workgroups(M, K):
    """The workgroups of the KS member rollout (csrc/ks_rollout.hip: ks_rollout_kernel, member form) for M members of K trajectories:
    a list of (member, pair, b0, has1).  Workgroup w serves member w // ceil(K / 2), pair w % ceil(K / 2): the trajectories
    b0 = member * K + 2 * pair and, where has1, b0 + 1 -- the pairing of a solo launch on K trajectories, so the two
    trajectories that share a complex FFT always belong to one member."""
    hp = (K + 1) // 2
    out = []
    for w in range(M * hp):
        m, pair = divmod(w, hp)
        out.append((m, pair, m * K + 2 * pair, 2 * pair + 1 < K))
    return out


def score_members(episode_reward, done_step):
    """score [M] and order of a population from episode_reward [M, K] and done_step [M, K] (host arrays): a member's score is
    the mean of its K episode rewards, NaN when any of its trajectories blew up (done_step >= 0) or is not finite; order =
    member indices best first, NaN scores last, ties by index."""
    er = np.asarray(episode_reward, dtype=np.float64)
    ds = np.asarray(done_step)
    bad = (ds >= 0).any(axis=1) | ~np.isfinite(er).all(axis=1)
    score = np.where(bad, np.nan, np.where(bad[:, None], 0.0, er).mean(axis=1))
    order = sorted(range(er.shape[0]), key=lambda m: (bool(np.isnan(score[m])), -score[m] if not np.isnan(score[m]) else 0.0, m))
    return score, order


# ---- selection: who takes over whom (pure host logic)

def plan_exploit(score, order, frac=0.25):
    """[(dst, src), ...] of one exploit step on M members from an evaluation's `score` [M] (NaN: not rankable) and `order` (best
    first, NaN last, ties by index: score_members).  n = max(1, floor(frac M)), frac <= 0.5; the sources are the best n members
    of `order` with a finite score, the destinations the worst n of `order` followed by every NaN-scored member not among them
    (each group in `order`'s sequence); destination k takes source k mod n_sources.  Empty when no score is finite.  No member is
    both a source and a destination."""
    score = np.asarray(score, dtype=np.float64)
    order = [int(m) for m in order]
    M = len(order)
    if not 0.0 < frac <= 0.5:
        raise ValueError(f"plan_exploit: frac must lie in (0, 0.5] (got {frac!r})")
    if score.shape != (M,) or sorted(order) != list(range(M)):
        raise ValueError("plan_exploit: score [M] and order (a permutation of the M members) are needed")
    n = max(1, int(np.floor(frac * M)))
    sources = [m for m in order[:n] if np.isfinite(score[m])]
    if not sources:
        return []
    worst = order[M - n:]
    dests = [m for m in worst + [m for m in order[:M - n] if not np.isfinite(score[m])] if m not in sources]
    return [(d, sources[k % len(sources)]) for k, d in enumerate(dests)]


def perturb_factors(rng, n, lo, hi):
    """[n, len(PERTURBED)] factors of exploit's perturbation, each `lo` or `hi` with equal probability, from ONE draw of the
    numpy Generator `rng` (row k: destination k of the plan; columns: PERTURBED)"""
    pick = rng.integers(0, 2, size=(int(n), len(PERTURBED)))
    return np.where(pick == 0, float(lo), float(hi))


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


def _model(actor):
    return getattr(actor, "model", actor)


def _handle_int(model):
    return int(getattr(model.handle, "value", model.handle))


def _has_persistent_rollout(setup):
    """the 2-D environments and the global agent have no persistent rollout at all"""
    return not (getattr(setup, "is_fluid", False) or getattr(setup, "is_kseg2d", False) or getattr(setup, "mono", False))


def _has_batched_rollout(setup):
    """the two 2-D environments with per-actuator agents: no persistent rollout, but pdec_rollout_members enqueues ONE step loop on
    the B = M K environment for them (served = 2), the member acting kernel in the place of the acting call"""
    return ((getattr(setup, "is_fluid", False) or getattr(setup, "is_kseg2d", False)) and not getattr(setup, "mono", False)
            and not getattr(setup, "memory_size", 0))


ACT_MEMBERS_LDS = 48 * 1024      # SMALL_ACT_LDS of csrc/mlp.hpp


def act_members_tiles(C, maxw, itemsize):
    """The tile plan of the member acting kernel (csrc/act_members.hip: act_members_plan) for C columns per member, an actor whose
    widest layer (input included) has maxw rows and states of `itemsize` bytes: (TC, tiles per member).  A workgroup holds two
    activation buffers [maxw][TC] in LDS; TC is the largest multiple of 64 that fits ACT_MEMBERS_LDS, capped at C rounded up to
    64.  (0, 0): not even 64 columns fit -- the call is not served."""
    tc = ACT_MEMBERS_LDS // (2 * int(maxw) * int(itemsize)) // 64 * 64
    if tc < 64 or C < 1:
        return 0, 0
    tc = min(tc, -(-int(C) // 64) * 64)
    return tc, -(-int(C) // tc)


FAULT_KEYS = ("actuator_gain", "sensor_gain", "sensor_bias")


def fault_arrays(setup, scenario, index=0):
    """one scenario of evaluate_actors(faults=...) as float64 arrays [A], [S], [S], missing keys healthy; shapes refused by name"""
    if not hasattr(setup, "fault_scenario"):
        raise _lib.PdecError(f"evaluate_actors(faults=...): {type(setup).__name__} has no actuator / sensor faults (KS setups only)")
    extra = set(scenario) - set(FAULT_KEYS)
    if extra:
        raise _lib.PdecError(f"evaluate_actors: faults[{index}] has unknown keys {sorted(extra)}; a scenario holds {FAULT_KEYS}")
    return setup.fault_scenario(**{k: scenario[k] for k in FAULT_KEYS if scenario.get(k) is not None})


def evaluate_actors(setup, actors, y0=None, n_inits=8, init_seed=0, steps=None, dtype=torch.float64, stream=None, act_limit=1.0,
                    log=False, device="cuda:0", mu=None, control_from=0, faults=None):
    """One greedy evaluation episode of each of M actors (HipMLPs or approximators of ONE shape) from the same K initial fields:
    `y0` [K, ...] in the environment's memory layout, or -- None -- n_inits fields drawn once with env.random_init from the
    Philox stream (init_seed, 0).  `steps` defaults to one episode (te / dt + 1, as testrun).  The environment of
    B = M * K trajectories is this call's own (member m: trajectories m K .. m K + K - 1) on `stream`, which waits for every
    actor's stream.  Where the library serves it (pdec_rollout_members: KS and 1-D Keller-Segel, per-actuator actors of <= 3
    layers no wider than 32) all M episodes are ONE launch, Float32 actors read as they are.  For the fluid and the 2-D
    Keller-Segel setups (per-actuator agents, memory_size = 0; actors pdec_policy_act_members serves) the control steps are
    enqueued ONCE on that B = M K environment -- the member acting kernel, then the batched env step -- instead of M times at
    B = K.  Otherwise M env.rollout calls on one B = K environment with actor clones as testrun makes them.  The same numbers,
    member by member and bit for bit, on all three routes.
    Returns episode_reward [M, K] (mean over actuators of the summed reward, PDEhook's figure), reward_sum [M, K, A],
    done_step [M, K] (device tensors), score [M] (numpy; NaN: a trajectory blew up or is not finite), order (best first, NaN
    last, ties by index), one_launch, workgroups (of the one launch; None otherwise), batched (True: the one step loop of the
    2-D setups; False on the other two routes) and with log=True the rows y, p, action, reward [T, M, K, ...].
    Robustness (scripts/KS/KS200_disturbed/KS200_disturbed.jl at batch scale; KS setups): `mu`, a sequence of n_mu disturbance
    amplitudes, evaluates every actor at every amplitude on the same K fields -- the environment has B = M * n_mu * K
    trajectories, member m's block laid out [n_mu][K], each (member, amplitude) block of K trajectories its own entry of the
    launch's actor table (so KS is still ONE launch, and a block's numbers are bit for bit those of the call with that single
    amplitude) -- and `control_from` = n0 leaves the first n0 steps uncontrolled and unrewarded (PDEenv.rollout).  The result
    then carries episode_reward [M, n_mu, K], reward_sum [M, n_mu, K, A], done_step [M, n_mu, K], score [M, n_mu] (the NaN rule
    per (member, amplitude)), mu (numpy) and order by the mean of score over the amplitudes (NaN if any of them is NaN); the
    log rows are [T, M, n_mu, K, ...].  mu=None: the shapes above, setup.mu everywhere.
    Fault tolerance (KS setups): `faults`, a sequence of n_f scenarios as KSSetup.fault_scenario makes them (dicts of
    actuator_gain [A], sensor_gain [S], sensor_bias [S]), evaluates every actor under every scenario on the same K fields, laid
    out exactly as `mu` is: B = M * n_f * K, each (member, scenario) block its own entry of the actor table (PDEenv.set_faults on
    the one environment, whose initial state is sensed through the faults).  The result carries episode_reward [M, n_f, K],
    reward_sum [M, n_f, K, A], done_step [M, n_f, K], score [M, n_f], faults (the scenarios) and order by the mean score over the
    scenarios with the NaN rule of the mu form; a block is bit for bit the call with that single scenario.  `faults` together
    with `mu` is refused."""
    members = [_model(a) for a in actors]
    M = len(members)
    if M < 1:
        raise _lib.PdecError("evaluate_actors: needs at least one actor")
    mus = None if mu is None else [float(x) for x in np.asarray(mu, dtype=np.float64).reshape(-1)]
    if mus is not None and not mus:
        raise _lib.PdecError("evaluate_actors: mu is empty")
    if faults is not None and mus is not None:
        raise _lib.PdecError("evaluate_actors: faults together with mu is not served (one sweep per call)")
    scen = None
    if faults is not None:
        scen = [fault_arrays(setup, f, i) for i, f in enumerate(faults)]
        if not scen:
            raise _lib.PdecError("evaluate_actors: faults is empty")
    n_mu = len(scen) if scen is not None else (1 if mus is None else len(mus))      # blocks per member: amplitudes or scenarios
    control_from = int(control_from)
    models = [md for md in members for _ in range(n_mu)]       # one entry per (member, amplitude) block of K trajectories
    M_members, M = M, M * n_mu
    for m, md in enumerate(members):
        if list(md.dims) != list(models[0].dims) or list(md.acts) != list(models[0].acts):
            raise _lib.PdecError(f"evaluate_actors: member {m}'s actor shape {list(md.dims)} / activations differ from member 0's "
                                 f"{list(models[0].dims)}: all members must have the same shape")
    dev = torch.device(device)
    small = None                # the B = K environment: draws the shared fields, and serves the member-by-member form
    T = int(round((setup.te - setup.t0) / setup.dt)) + 1 if steps is None else int(steps)
    with _on_stream(stream):    # (the environments' own tensors are made on their stream as well)
        if y0 is None:
            small, y0 = held_out_fields(setup, n_inits, init_seed, dtype, device, stream)   # (the draw of TrainPipeline(eval_every=...))
        y0 = (y0 if isinstance(y0, torch.Tensor) else torch.as_tensor(np.array(y0, copy=True))).to(device=dev, dtype=dtype).contiguous()
        K = int(y0.shape[0])
        env = None              # without a persistent rollout or a batched step loop no B = M K environment is built to hear it
        if _has_persistent_rollout(setup) or _has_batched_rollout(setup):
            env = PDEenv(setup, B=M * K, dtype=dtype, device=device, y0=y0.repeat((M,) + (1,) * (y0.dim() - 1)), stream=stream,
                         autoreset=False)
            if mus is not None:
                env.set_disturbance(torch.tensor(mus, dtype=torch.float64).repeat_interleave(K).repeat(M_members))
            if scen is not None:    # trajectory (m, f, k) carries scenario f; the initial state is sensed through it
                env.set_faults(**{k: torch.as_tensor(np.stack([sc[k] for sc in scen])).repeat_interleave(K, dim=0).repeat(M_members, 1)
                                  for k in FAULT_KEYS})
                env.reset()
            if control_from:
                _lib.check(env.lib.pdec_env_set_control_from(env.handle, control_from))
    B = M * K
    s_env = stream if stream is not None else torch.cuda.current_stream(dev)
    others = {}
    for md in models:
        s = getattr(md, "stream", None)
        if s is not None and s.cuda_stream != s_env.cuda_stream:
            others[s.cuda_stream] = s
    for s in others.values():
        s_env.wait_stream(s)
    kw = dict(dtype=dtype, device=dev)
    served = C.c_int(0)
    if env is not None:
        with _on_stream(stream):
            out = dict(reward_sum=torch.zeros((B, setup.reward_len), **kw), done_step=torch.zeros(B, dtype=torch.int32, device=dev))
            done_any = torch.zeros(B, dtype=torch.int32, device=dev)
            if log:
                out.update(y=torch.empty((T,) + env._yshape, **kw), p=torch.empty((T,) + env._pshape, **kw),
                           action=torch.empty((T,) + env._ashape, **kw), reward=torch.empty((T, B, setup.reward_len), **kw))
        handles = (_lib.Handle * M)(*[_handle_int(md) for md in models])
        P = _lib.ptr
        try:
            _lib.check(env.lib.pdec_rollout_members(
                env.handle, handles, M, K, T, P(env.y), P(env.state), P(env.action), float(act_limit), 0, P(out["reward_sum"]),
                P(out.get("y")), P(out.get("p")), P(out.get("action")), P(out.get("reward")), P(done_any), P(out["done_step"]),
                C.byref(served)))
        finally:
            for s in others.values():       # whatever next writes the actors' parameters waits for the launch that reads them
                s.wait_stream(s_env)
    one, batched = served.value == 1, served.value == 2
    if not (one or batched):
        if env is not None:
            env.close()
        if small is None:
            with _on_stream(stream):
                small = PDEenv(setup, B=K, dtype=dtype, device=device, y0=y0, stream=stream, autoreset=False)
        else:
            small.set_y0(y0)
        cols = K * setup.state_shape[1]
        parts = []
        for v, md in enumerate(models):
            if v % n_mu == 0:
                actor = md if (md.dtype == small.dtype and md.max_cols >= cols) else md.clone(dtype=small.dtype, max_cols=cols)
            if mus is not None:
                small.set_disturbance(torch.full((K,), mus[v % n_mu], dtype=torch.float64))
            if scen is not None:
                small.set_faults(**{k: torch.as_tensor(scen[v % n_mu][k]).unsqueeze(0).repeat(K, 1) for k in FAULT_KEYS})
            small.reset()
            parts.append(small.rollout(actor, T, act_limit=act_limit, learning=False, log=log, control_from=control_from))
        with _on_stream(stream):
            out = {k: torch.cat([p_[k] for p_ in parts], dim=0 if k in ("reward_sum", "done_step") else 1)
                   for k in (("reward_sum", "done_step") + (("y", "p", "action", "reward") if log else ()))}
    with _on_stream(stream):
        res = dict(reward_sum=out["reward_sum"].view(M, K, -1), done_step=out["done_step"].view(M, K))
        res["episode_reward"] = res["reward_sum"].mean(dim=2)
        for k in ("y", "p", "action", "reward"):
            if k in out:
                res[k] = out[k].view((T, M, K) + tuple(out[k].shape[2:]))
        host = (res["episode_reward"].double().cpu().numpy(), res["done_step"].cpu().numpy())     # (waits for the stream)
    res["score"], res["order"] = score_members(*host)
    if mus is not None or scen is not None:
        with _on_stream(stream):
            for k in ("reward_sum", "done_step", "episode_reward"):
                res[k] = res[k].view((M_members, n_mu) + tuple(res[k].shape[1:]))
            for k in ("y", "p", "action", "reward"):
                if k in res:
                    res[k] = res[k].view((T, M_members, n_mu) + tuple(res[k].shape[2:]))
        res["score"] = res["score"].reshape(M_members, n_mu)
        if mus is not None:
            res["mu"] = np.asarray(mus, dtype=np.float64)
        else:
            res["faults"] = scen
        mean = res["score"].mean(axis=1)                  # NaN if any amplitude's score is
        res["order"] = sorted(range(M_members), key=lambda m: (bool(np.isnan(mean[m])), -mean[m] if not np.isnan(mean[m]) else 0.0, m))
    res["one_launch"], res["batched"] = one, batched
    is_ks = one and tuple(setup.y_shape) == (setup.nx,)      # (served: a setup with a persistent rollout, so no 2-D one)
    res["workgroups"] = (len(member_workgroups(M, K)) if is_ks else B) if one else None
    if one or batched:
        env.close()
    if small is not None:
        small.close()
    return res


class Population:
    def __init__(self, setup, agents, hooks, stream_env, dtype=torch.float64, device="cuda:0", part_streams=None,
                 max_log_bytes=8 << 30):
        """part_streams: handed to the population's PDEenv (the fluid steps its batch in parts on them where it splits it).
        max_log_bytes: the most the per-step slots of one episode (and the best-row copies of the block path) may take on the
        device; a fluid member's are (T + 1) + T full spectra and more (episode_log_bytes)."""
        M = len(agents)
        if M < 1 or len(hooks) != M:
            _refuse("needs one hook per agent and at least one member")
        name = type(setup).__name__
        if getattr(setup, "is_kseg2d", False):
            _refuse(f"{name} is not served (its batched step, part streams and initialisers need their own check); "
                    "KSSetup, KellerSegelSetup and FluidSetup are")
        if dtype != torch.float64:
            _refuse("fp64 environments only (the shape of every reference-shaped run)")
        if getattr(setup, "memory_size", 0):
            _refuse("memory_size > 0 is not on the device-episode path")
        if stream_env is None:
            _refuse("needs an explicit environment stream (make_streams)")
        # before anything is allocated: the members must be learners of THIS setup
        ns, A = setup.state_shape
        for m, ag in enumerate(agents):
            if not isinstance(ag, Agent):
                _refuse(f"member {m}: an Agent with a PDEhook is needed")
            pol = ag.policy
            if getattr(pol.behavior_actor.model, "noise_scale", None) is not None:
                _refuse(f"member {m}: a noise scale array is set on its actor (set_noise_scale); a member explores at its own "
                        "act_noise, which may differ from member to member")
            if getattr(pol, "mono", None) or getattr(pol, "reward_group", None) is not None:
                continue                # (refused by name below)
            rows, stride = pol.behavior_actor.model.dims[0], ag.trajectory.stride
            if rows != ns or stride != A:
                _refuse(f"member {m}: its actor reads {rows} state rows and its replay takes {stride} columns per step, but {name} "
                        f"has {ns} state rows and {A} actuators: the member was not made for this setup")
            if getattr(setup, "is_fluid", False) and stride > 256:
                _refuse(f"member {m}: {stride} actuators per step, and the device-episode path serves at most 256 "
                        f"(run.device_episodes_ok); of {name}'s experiments Fluid_8 and Fluid_16 are served, Fluid_32 is not")
        self.setup, self.agents, self.hooks, self.M = setup, list(agents), list(hooks), M
        probe = PDEenv(setup, B=1, dtype=dtype, device=device, stream=stream_env, autoreset=False)
        a0 = agents[0]
        for m, (ag, hk) in enumerate(zip(agents, hooks)):
            if not isinstance(ag, Agent) or type(hk) is not PDEhook:
                _refuse(f"member {m}: an Agent with a PDEhook is needed")
            pol = ag.policy
            if getattr(pol, "mono", None) or getattr(pol, "reward_group", None) is not None:
                _refuse(f"member {m}: the global/mono agent and reward groups are not served")
            if pol.reducer is not None:
                _refuse(f"member {m}: a reducer is not on the device-episode path")
            if pol.memory_size:
                _refuse(f"member {m}: memory_size > 0 is not on the device-episode path")
            if pol.sampling != "device":
                _refuse(f"member {m}: host sampling is not on the device-episode path")
            if hk.log_trajectory != 0:
                _refuse(f"member {m}: log_trajectory != 0 is not on the device-episode path")
            if not device_episodes_ok(ag, probe, StopAfterEpisode(1), hk):
                _refuse(f"member {m}: a solo run would not take the device-episode path (run.device_episodes_ok: "
                        "start policy, sampling, small update, streams)")
            # (gamma, rho, the learning rates, act_noise and act_limit are each member's own: _hyper_rows)
            for k in ("update_after", "update_freq", "update_loops", "batch_size", "start_steps", "quirk"):
                if getattr(pol, k) != getattr(a0.policy, k):
                    _refuse(f"member {m}: hyper-parameter {k} differs from member 0's")
            for attr in ("behavior_actor", "behavior_critic"):
                if getattr(pol, attr).model.dims != getattr(a0.policy, attr).model.dims:
                    _refuse(f"member {m}: network shapes differ from member 0's")
            if type(pol.start_policy) is not type(a0.policy.start_policy):
                _refuse(f"member {m}: start policy differs from member 0's")
            tr = ag.trajectory
            if tr.capacity != a0.trajectory.capacity or tr.stride != a0.trajectory.stride:
                _refuse(f"member {m}: replay capacity differs from member 0's")
            if tr.stream.cuda_stream != a0.trajectory.stream.cuda_stream:
                _refuse(f"member {m}: update stream differs from member 0's")
        probe.close()
        # the update kernel is chosen once for the whole launch, from member 0's rho at this point (small_plan: the frozen-target
        # kernel at rho == 1, compared as the Float32 the kernels compute with)
        self._launch_wide = None
        self._frozen_launch = bool(np.float32(a0.policy.rho_effective) == np.float32(1.0))
        self._hyper_rows()
        self.stream_env, self.stream_upd = stream_env, a0.trajectory.stream
        if self.stream_env.cuda_stream == self.stream_upd.cuda_stream:
            _refuse("the environment and the networks need two different streams")
        T = _episode_steps(setup)
        per_logs, per_best = episode_log_bytes(setup, T, 8)
        need = M * (per_logs + per_best)
        if need > int(max_log_bytes):
            _refuse(f"the per-step slots of one episode of {T} steps take {M * per_logs} bytes for {M} members and the best "
                    f"episode's rows of the block path {M * per_best} more: {need} bytes in all, above max_log_bytes = "
                    f"{int(max_log_bytes)}; at most {int(max_log_bytes) // (per_logs + per_best)} members fit")
        self.is_fluid = bool(getattr(setup, "is_fluid", False))
        self.env = PDEenv(setup, B=M, dtype=dtype, device=device, stream=stream_env, autoreset=False, part_streams=part_streams)
        self.lib = lib = self.env.lib
        if not self.is_fluid:       # (the fluid step is per trajectory as it stands: no pairing of trajectories to re-arrange)
            _lib.check(lib.pdec_env_set_member_layout(self.env.handle, 1))
        self.cols = A
        pol0, tr0 = a0.policy, a0.trajectory
        with _on_stream(self.stream_upd):
            self.rows = torch.zeros((M, ROW), dtype=torch.int64, device=self.env.device)
        H = (_lib.Handle * M)
        hs = [H(*[_handle_int(getattr(ag.policy, k).model) for ag in agents])
              for k in ("behavior_actor", "behavior_critic", "target_actor", "target_critic")]
        traces = (C.c_void_p * (4 * M))(*[t.data_ptr() for ag in agents for t in (ag.trajectory.state, ag.trajectory.action,
                                                                                    ag.trajectory.reward, ag.trajectory.terminal)])
        seeds = (C.c_uint64 * (2 * M))(*[s for ag in agents for s in (ag.policy._noise_seed, ag.policy._sample_seed)])
        losses = (C.c_void_p * M)(*[ag.policy._losses.data_ptr() for ag in agents])
        self._h = _lib.Handle()
        _lib.check(lib.pdec_population_create(
            C.byref(self._h), M, hs[0], hs[1], hs[2], hs[3], traces, seeds, losses, _lib.dtype_code(dtype), A, tr0.capacity,
            tr0.stride, int(pol0.update_loops), int(pol0.batch_size), float(pol0.y), pol0.rho_effective, int(pol0.quirk),
            float(pol0.behavior_actor.optimizer.eta), float(pol0.behavior_critic.optimizer.eta), int(pol0.update_after * tr0.stride),
            int(pol0.update_freq), int(pol0.start_steps), _lib.ptr(self.rows)))
        # (refused for network shapes whose update kernel takes one set for the whole launch: members then must not differ)
        if lib.pdec_population_set_member_hyper(self._h, 1) != 0:
            self._launch_wide = (lib.pdec_last_error().decode(errors="replace"), self._hyper_rows()[0, :4].copy())
            self._hyper_rows()
        for ag in agents:
            ag.policy.set_reward_interleave(1)
        with _on_stream(self.stream_upd):
            self._which = torch.zeros(M, dtype=torch.int32, device=self.env.device)
        self.episode_steps = []       # per episode: the control steps each member executed (0: idle)
        # host seconds per phase, summed over episodes: issue = initialisers + every enqueue up to the read-back,
        # readback = waiting for the device, settle = the members' host bookkeeping and the boundary launches
        # (blocks: read-backs; with episodes_per_sync = 1 every episode is one)
        self.timing = dict(episodes=0, issue_s=0.0, readback_s=0.0, settle_s=0.0, blocks=0)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.pdec_destroy(self._h)
            self._h = _lib.Handle()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- per-member hyper-parameters: the agents' own attributes are the truth, read when an episode's row table is written
    def _hyper_rows(self):
        """[M, 6] doubles in HYPER_KEYS' order with rho = rho_effective (what the kernels receive), after the rule for rho: the
        update kernel is one for the whole launch, so either every member's targets are frozen (rho_effective == 1) or none's are"""
        q0 = self.agents[0].policy.quirk_frozen_targets
        out = np.empty((self.M, len(HYPER_KEYS)), dtype=np.float64)
        for m, ag in enumerate(self.agents):
            pol = ag.policy
            if pol.quirk_frozen_targets != q0:
                _refuse(f"member {m}: quirk_frozen_targets differs from member 0's (frozen and moving target networks take "
                        "different update kernels, and the kernel is one for the whole launch)")
            rho = float(pol.rho_effective)
            if bool(np.float32(rho) == np.float32(1.0)) != self._frozen_launch:
                _refuse(f"member {m}: rho_effective = {rho:g} beside "
                        f"{'frozen targets (rho_effective = 1)' if self._frozen_launch else 'moving targets (rho_effective < 1)'} "
                        "of the population: rho may differ between members only while every member's rho_effective is < 1 "
                        "(rho == 1 selects the frozen-target kernel for the whole launch)")
            out[m] = (float(pol.y), rho, float(pol.behavior_actor.optimizer.eta), float(pol.behavior_critic.optimizer.eta),
                      float(pol.act_noise), float(pol.act_limit))
            if self._launch_wide is not None and not np.array_equal(out[m, :4], self._launch_wide[1]):
                _refuse(f"member {m}: gamma, rho or a learning rate differs from the population's at its creation, and "
                        f"{self._launch_wide[0]}")
        return out

    def hyper(self):
        """the members' hyper-parameters as a dict of numpy arrays [M]: gamma (policy.y), rho (policy.p), rho_effective (what
        the update receives: 1 under quirk_frozen_targets), actor_lr, critic_lr, act_noise, act_limit"""
        t = self._hyper_rows()
        out = {k: t[:, i].copy() for i, k in enumerate(HYPER_KEYS)}
        out["rho_effective"] = out["rho"]
        out["rho"] = np.array([float(ag.policy.p) for ag in self.agents])
        return out

    def set_hyper(self, m, gamma=None, rho=None, actor_lr=None, critic_lr=None, act_noise=None, act_limit=None):
        """write member m's agent attributes (None: keep); legal between `run` calls, in force from the next episode on"""
        pol = self.agents[m].policy
        if gamma is not None:
            pol.y = gamma
        if rho is not None:
            pol.p = rho
        if actor_lr is not None:
            pol.behavior_actor.optimizer.eta = actor_lr
        if critic_lr is not None:
            pol.behavior_critic.optimizer.eta = critic_lr
        if act_noise is not None:
            pol.act_noise = act_noise
        if act_limit is not None:
            pol.act_limit = act_limit
        self._hyper_rows()              # (the rule for rho)

    # ---- selection
    def clone(self, pairs, replay="copy"):
        """pairs {dst: src}: member dst takes over member src's learner -- the four networks, the ADAM moments and beta powers,
        the loss pair and, with replay="copy", the filled prefix of src's replay traces with its counters (replay="keep": dst
        keeps its own replay) -- in ONE launch for all pairs (pdec_population_clone).  Exactly what load_agent(dst) of
        save_agent(src, with_trajectory=(replay == "copy")) does to the learner; dst keeps its own update_step, noise and sample
        seeds and offsets, host rng, hook (a log: rewards history and best actor stay dst's), environment row and
        hyper-parameters.  Legal between `run` calls.  No member may be both a source and a destination."""
        if replay not in ("copy", "keep"):
            _refuse(f'clone: replay must be "copy" or "keep", not {replay!r}')
        M = self.M
        src = np.arange(M, dtype=np.int32)
        rows_sa, rows_rt = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64)
        for d, s in pairs.items():
            if not 0 <= int(d) < M:
                _refuse(f"clone: destination {d} is not one of the {M} members")
            src[int(d)] = int(s) if -2 ** 31 <= int(s) < 2 ** 31 else -1
        moved = [(d, int(src[d])) for d in range(M) if src[d] != d]
        if replay == "copy":
            for d, s in moved:
                if 0 <= s < M:
                    tr = self.agents[s].trajectory
                    rows_sa[d], rows_rt[d] = min(tr.n_sa, tr.capacity + tr.stride), min(tr.n_rt, tr.capacity)
        s_env, s_upd = self.stream_env, self.stream_upd
        _join(s_upd, s_env)
        try:
            _lib.check(self.lib.pdec_population_clone(self._h, src.ctypes.data_as(C.c_void_p), rows_sa.ctypes.data_as(C.c_void_p),
                                                      rows_rt.ctypes.data_as(C.c_void_p)))
        finally:
            _join(s_upd, s_env)
        if replay == "copy":
            for d, s in moved:
                td, ts = self.agents[d].trajectory, self.agents[s].trajectory
                td.n_sa, td.n_rt = ts.n_sa, ts.n_rt
        return moved

    def exploit(self, result=None, frac=0.25, perturb=None, rng=None, replay="copy"):
        """One step of population-based selection: plan_exploit on `result` (an evaluation's dict with score and order; None:
        self.evaluate()), `clone` of the plan, then every destination inherits its source's gamma, rho, learning rates,
        act_noise and act_limit -- with perturb=(lo, hi) its actor_lr, critic_lr and act_noise each times lo or hi, drawn from the
        numpy Generator `rng` (perturb_factors).  Returns [{dst, src, hyper}, ...] in the plan's order."""
        if perturb is not None and rng is None:
            _refuse("exploit: perturb=(lo, hi) needs rng (a numpy.random.Generator)")
        if result is None:
            result = self.evaluate()
        plan = plan_exploit(result["score"], result["order"], frac)
        if not plan:
            return []
        self.clone(dict(plan), replay=replay)
        fac = perturb_factors(rng, len(plan), *perturb) if perturb is not None else np.ones((len(plan), len(PERTURBED)))
        table = self.hyper()
        applied = []
        for k, (d, s) in enumerate(plan):
            h = {key: float(table[key][s]) for key in HYPER_KEYS}
            for j, key in enumerate(PERTURBED):
                h[key] = h[key] * float(fac[k, j])
            self.set_hyper(d, **h)
            applied.append(dict(dst=d, src=s, hyper=h))
        return applied

    def evaluate(self, which="current", **kw):
        """evaluate_actors on the members' behaviour actors ("current") or on their hooks' best actors ("best"): every member
        scored on the same held-out initial fields.  The evaluation has its own environment; the population's environment,
        counter table, Philox offsets and replay traces are not touched, so training that goes on afterwards is bit for bit what
        it would have been without the call."""
        if which == "current":
            actors = [ag.policy.behavior_actor for ag in self.agents]
        elif which == "best":
            for m, hk in enumerate(self.hooks):
                if not hk.collect_NNA or hk.bestNNA is None:
                    _refuse(f'evaluate(which="best"): member {m}\'s hook keeps no best actor (collect_NNA, and at least one run)')
            actors = [hk.bestNNA for hk in self.hooks]
        else:
            _refuse(f'evaluate: which must be "current" or "best", not {which!r}')
        kw.setdefault("stream", self.stream_env)
        kw.setdefault("dtype", self.env.dtype)
        kw.setdefault("device", self.env.device)
        return evaluate_actors(self.setup, actors, **kw)

    # ---- the episode loop
    def run(self, stops, episodes_per_sync=1):
        """run every member until its stop condition fires.  episodes_per_sync = E > 1: blocks of up to E whole episodes are
        enqueued per read-back -- the episode boundary (hook, stop condition, counters, next initial field) is decided on the
        device (pdec_population_episode_close) and the members' host state is settled once per block; every member ends bit for
        bit where E = 1 leaves it.  Refused with E > 1: collect_history (needs every episode's rows on the host) and a hook
        that was given an error_detection callable."""
        if len(stops) != self.M or any(type(s) not in (StopAfterEpisode, StopAfterEpisodeWithMinSteps) for s in stops):
            _refuse("one StopAfterEpisode / StopAfterEpisodeWithMinSteps per member")
        E = int(episodes_per_sync)
        if E < 1 or E != episodes_per_sync:
            _refuse(f"episodes_per_sync must be a whole number >= 1 (got {episodes_per_sync!r}) for members 0..{self.M - 1}")
        if E > 1:
            for m, (ag, hk) in enumerate(zip(self.agents, self.hooks)):
                if hk.collect_history:
                    _refuse(f"member {m}: collect_history needs every episode's rows on the host; run it with episodes_per_sync=1")
                if hk.error_detection_given and not self._own_error_detection(hk):
                    _refuse(f"member {m}: a hook with an error_detection callable is settled on the host every episode; run it "
                            "with episodes_per_sync=1")
                if (ag.policy.reset_stage == POST_EPISODE_STAGE) != (self.agents[0].policy.reset_stage == POST_EPISODE_STAGE):
                    _refuse(f"member {m}: reset_stage differs from member 0's (one boundary launch serves all members)")
        env, M = self.env, self.M
        s_env, s_upd = self.stream_env, self.stream_upd
        for ag, hk in zip(self.agents, self.hooks):
            hk(PRE_EXPERIMENT_STAGE, ag, env)
            ag(PRE_EXPERIMENT_STAGE, env)
        # the hooks' best / current actors (made at PRE_EXPERIMENT): the targets of the one copy launch per episode
        best = (_lib.Handle * M)(*[_handle_int(hk.bestNNA.model) if hk.collect_NNA else 0 for hk in self.hooks])
        cur = (_lib.Handle * M)(*[_handle_int(hk.currentNNA.model) if hk.collect_NNA else 0 for hk in self.hooks])
        _lib.check(self.lib.pdec_population_set_actor_copies(self._h, best, cur))
        active = np.ones(M, dtype=bool)
        while active.any():
            _join(s_upd, s_env)
            if E == 1:
                self._episode(active, stops)
                self.timing["blocks"] = self.timing.get("blocks", 0) + 1
            else:
                self._block(active, stops, block_length(stops, active, _episode_steps(env), E))
        _join(s_upd, s_env)
        for ag, hk in zip(self.agents, self.hooks):
            hk(POST_EXPERIMENT_STAGE, ag, env)
        return self.hooks

    def _ic_case(self):
        """generate_random_init's case (FluidSetup.jl:386-394): ic(4) in evaluation, ic(3) in training"""
        return 4 if self.setup.evaluation else 3

    def _fluid_ic(self, table, out):
        """pdec_fluid_ic_dev on the environment's stream: `out` [M, ...] from the device table [M, nv, 4] (kept alive by the
        caching allocator's stream order: it was made with the environment's stream current)"""
        _lib.check(self.lib.pdec_fluid_ic_dev(self.env.handle, _lib.ptr(table), int(table.shape[-2]), _lib.ptr(out)))

    def _pre_episode(self, active):
        """env.reset(), agent PRE_EPISODE (the dummy pop), hook PRE_EPISODE (random inits: one launch for all members); the
        rows of idle members are restored afterwards"""
        env, M, lib = self.env, self.M, self.lib
        idle = np.flatnonzero(~active)
        with _on_stream(self.stream_env):
            keep_y, keep_s = (env.y[idle].clone(), env.state[idle].clone()) if idle.size else (None, None)
        env.reset()
        for m in np.flatnonzero(active):
            self.agents[m](PRE_EPISODE_STAGE, env)          # host counters only (pop_sa)
        rnd = [m for m in np.flatnonzero(active) if self.hooks[m].use_random_init]
        with _on_stream(self.stream_env):
            if rnd:
                drawn = torch.empty_like(env.y)
                if self.is_fluid:
                    # every member's own vortex table from its own generator, as its solo hook draws it
                    # (FluidSetup.random_init_device); one upload, one initialiser launch at B = M
                    tables, _ = draw_block_tables(self.setup, [self.hooks[m].init_rng if m in rnd else None for m in range(M)], 1,
                                                  self._ic_case())
                    self._fluid_ic(torch.from_numpy(tables[0]).to(env.device), drawn)
                else:
                    nblk = (env.random_init_coefficients() + 3) // 4
                    seeds = torch.tensor([self.hooks[m].init_seed if m in rnd else 0 for m in range(M)], dtype=torch.int64)
                    offs = torch.tensor([self.hooks[m]._init_off if m in rnd else 0 for m in range(M)], dtype=torch.int64)
                    so = torch.stack([seeds, offs]).to(env.device, non_blocking=False)
                    _lib.check(lib.pdec_env_random_init_members(env.handle, _lib.ptr(so[0]), _lib.ptr(so[1]), _lib.ptr(drawn)))
                    for m in rnd:
                        self.hooks[m]._init_off += nblk
                mask = torch.zeros(M, dtype=torch.bool)
                mask[rnd] = True
                mask = mask.to(env.device)
                y0 = torch.where(mask.view((M,) + (1,) * (env.y.dim() - 1)), drawn, env.y0)
                env.y0 = y0
                env.y.copy_(y0)
                # the re-initialised members' states only: the others keep their reset state, as their solo hooks leave it
                st = env.featurize(env.y, env.state if env.setup.temporal_steps > 1 else None)
                env.state.copy_(torch.where(mask.view((M,) + (1,) * (env.state.dim() - 1)), st, env.state))
                env._state0.copy_(env.state)
            if idle.size:
                ii = torch.as_tensor(idle, device=env.device)
                env.y.index_copy_(0, ii, keep_y)
                env.state.index_copy_(0, ii, keep_s)

    def _episode(self, active, stops):
        env, M, lib, cols = self.env, self.M, self.lib, self.cols
        s_env, s_upd = self.stream_env, self.stream_upd
        P = _lib.ptr
        t0 = time.perf_counter()
        self._pre_episode(active)
        T = _episode_steps(env)
        logs = getattr(self, "_logs", None)
        if logs is None or logs.T != T:
            with _on_stream(s_env):
                logs = self._logs = _EpisodeLogs(env, T)
                self._flags = torch.zeros((T, M), dtype=torch.int32, device=env.device)     # per step: the members' done flags
        flags = self._flags
        # ---- the counter table of this episode (one upload)
        rows = np.zeros((M, ROW), dtype=np.int64)
        rows[:, GAMMA:ETA_C + 1] = self._hyper_rows()[:, :4].copy().view(np.int64)
        for m, ag in enumerate(self.agents):
            pol, tr = ag.policy, ag.trajectory
            rows[m, [USTEP, NSA, NRT, NOISE, SAMPLE]] = (pol.update_step, tr.n_sa, tr.n_rt, pol._noise_off, pol._sample_off)
            rows[m, HALT], rows[m, ACTIVE] = (0, 1) if active[m] else (1, 0)
            rows[m, NOISE_AMP:LIMIT + 1] = np.array([float(pol.act_noise), float(pol.act_limit)], dtype=np.float64).view(np.int64)
        _lib.check(lib.pdec_population_bp_sel(self._h, rows.ctypes.data_as(C.c_void_p), 0))
        start = rows.copy()
        with _on_stream(s_env):
            logs.y[0].copy_(env.y)
            logs.state[0].copy_(env.state)
            flags.zero_()
        with _on_stream(s_upd):
            self.rows.copy_(torch.from_numpy(rows))
        ev_act, ev_env = _Event(lib), _Event(lib)
        _join(s_upd, s_env)
        # (per step: the member-indexed glue and update on the networks' stream, the member-layout env step on the env's)
        for t in range(T):
            _lib.check(lib.pdec_population_glue(self._h, 0, P(logs.reward[t - 1]) if t else None, P(flags[t - 1]) if t else None,
                                                P(logs.state[t]), P(logs.action[t + 1])))
            ev_act.record(s_upd)
            ev_act.wait(s_env)
            _lib.check(lib.pdec_population_update(self._h))
            _lib.check(lib.pdec_env_step(env.handle, P(logs.y[t]), P(logs.action[t + 1]), P(logs.action[t]), P(logs.state[t]),
                                         P(logs.y[t + 1]), P(logs.p[t]), P(logs.state[t + 1]), P(logs.reward[t]), P(flags[t])))
            ev_env.record(s_env)
            ev_env.wait(s_upd)
        _lib.check(lib.pdec_population_glue(self._h, 1, P(logs.reward[T - 1]), P(flags[T - 1]), None, None))   # the time-out push
        with _on_stream(s_upd):
            # the per-step episode reward of PDEhook (mean over the actuators), member-major rows as a B = 1 run reduces them
            means = logs.reward.transpose(0, 1).contiguous().reshape(M * T, -1).mean(dim=1)
            pack = torch.cat([self.rows.view(-1).view(torch.uint8), flags.view(-1).view(torch.uint8), means.view(-1).view(torch.uint8)])
            t1 = time.perf_counter()
            host = pack.cpu().numpy()                                          # the one read-back (bytes)
        t2 = time.perf_counter()
        nr, nf = M * ROW * 8, T * M * 4
        rows_out = host[:nr].copy().view(np.int64).reshape(M, ROW)
        fl = host[nr:nr + nf].copy().view(np.int32).reshape(T, M)
        mean_h = host[nr + nf:].copy().view(np.float64).reshape(M, T)
        # ---- settle every member at its number of executed steps
        n_of = np.array([_executed_steps(fl[:, m], T) if active[m] else 0 for m in range(M)], dtype=np.int64)
        self.episode_steps.append(n_of.copy())
        pol0, tr0 = self.agents[0].policy, self.agents[0].trajectory
        sched = _episode_schedule(start[:, :SAMPLE + 1], T, cols, pol0.behavior_actor.model.dims[-1], tr0.capacity, tr0.stride,
                                  pol0.update_after, pol0.update_freq, pol0.update_loops, pol0.batch_size, pol0.start_steps)
        _lib.check(lib.pdec_population_bp_sel(self._h, rows_out.ctypes.data_as(C.c_void_p), 1))
        with _on_stream(s_env):
            ii = torch.as_tensor(n_of, device=env.device)
            ar = torch.arange(M, device=env.device)
            env.y = logs.y[ii, ar].contiguous()
            env.state = logs.state[ii, ar].contiguous()
            # POST_EPISODE push of the final states with the zero action (active members; one launch)
        s_upd.wait_stream(s_env)
        _lib.check(lib.pdec_population_glue(self._h, 2, None, None, P(env.state), None))
        want_rows = any(self.hooks[m].collect_bestDF for m in np.flatnonzero(active))
        if want_rows:
            with _on_stream(s_env):
                la, lp, ly, lr = (x.cpu() for x in (logs.action, logs.p, logs.y, logs.reward))
        np_dt = np.float64
        which = np.zeros(M, dtype=np.int32)
        for m in np.flatnonzero(active):
            ag, hk, n = self.agents[m], self.hooks[m], int(n_of[m])
            pol, tr = ag.policy, ag.trajectory
            counters = rows_out[m, :SAMPLE + 1].tolist()
            if counters != sched.after[m, n - 1].tolist():
                raise RuntimeError(f"Population: member {m}'s device counters disagree with its {n} executed steps")
            pol.update_step, tr.n_sa, tr.n_rt, pol._noise_off, pol._sample_off = counters
            _add_episode_reward(hk, mean_h[m, :n], np_dt)
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
                self._which.copy_(torch.from_numpy(which))
            _lib.check(lib.pdec_population_copy_actors(self._h, P(self._which)))
        s_env.wait_stream(s_upd)
        t3 = time.perf_counter()
        tm = self.timing
        tm["episodes"] += 1
        tm["issue_s"] += t1 - t0
        tm["readback_s"] += t2 - t1
        tm["settle_s"] += t3 - t2

    # ---- blocks of episodes (run(stops, episodes_per_sync > 1)): the episode boundary on the device
    def _own_error_detection(self, hk):
        """is the hook's error_detection FluidSetup.error_detection of this population's own setup (what make_hook() sets)?  The
        block path then runs its device form (pdec_fluid_error_detection) behind every episode's close launch"""
        f = hk.error_detection
        return (self.is_fluid and getattr(f, "__self__", None) is self.setup
                and getattr(f, "__func__", None) is getattr(type(self.setup), "error_detection", None))

    def _open_episode(self, any_random, table=None):
        """_pre_episode with the members masked by the device columns ACTIVE (rows) and use_random_init / init seed / init offset
        (book) instead of host lists: env.reset(), the random fields of all members in one launch, idle members keep y and state"""
        env, lib = self.env, self.lib
        M = self.M
        with _on_stream(self.stream_env):
            act = self.rows[:, ACTIVE] != 0
            keep_y, keep_s = env.y.clone(), env.state.clone()
        env.reset()
        with _on_stream(self.stream_env):
            if any_random:
                drawn = torch.empty_like(env.y)
                if self.is_fluid:       # this episode's slice of the block's vortex tables
                    self._fluid_ic(table, drawn)
                else:
                    seeds, offs = self._book[:, BK_INIT_SEED].contiguous(), self._book[:, BK_INIT_OFF].contiguous()
                    _lib.check(lib.pdec_env_random_init_members(env.handle, _lib.ptr(seeds), _lib.ptr(offs), _lib.ptr(drawn)))
                mask = act & (self._book[:, BK_RANDOM_INIT] != 0)
                y0 = torch.where(mask.view((M,) + (1,) * (env.y.dim() - 1)), drawn, env.y0)
                env.y0 = y0
                env.y.copy_(y0)
                st = env.featurize(env.y, env.state if env.setup.temporal_steps > 1 else None)
                env.state.copy_(torch.where(mask.view((M,) + (1,) * (env.state.dim() - 1)), st, env.state))
                env._state0.copy_(env.state)
            env.y.copy_(torch.where(act.view((M,) + (1,) * (env.y.dim() - 1)), env.y, keep_y))
            env.state.copy_(torch.where(act.view((M,) + (1,) * (env.state.dim() - 1)), env.state, keep_s))

    def _block(self, active, stops, L):
        """L whole episodes enqueued, one read-back, every member settled for the block"""
        env, M, lib, cols = self.env, self.M, self.lib, self.cols
        s_env, s_upd = self.stream_env, self.stream_upd
        P = _lib.ptr
        t0 = time.perf_counter()
        T = _episode_steps(env)
        logs = getattr(self, "_logs", None)
        if logs is None or logs.T != T:
            with _on_stream(s_env):
                logs = self._logs = _EpisodeLogs(env, T)
                self._flags = torch.zeros((T, M), dtype=torch.int32, device=env.device)     # per step: the members' done flags
        flags = self._flags
        want_rows = any(self.hooks[m].collect_bestDF and self.hooks[m].collect_NNA for m in np.flatnonzero(active))
        with _on_stream(s_upd):
            if getattr(self, "_elog", None) is None or self._elog.shape[0] < L:
                self._book = torch.zeros((M, BOOK), dtype=torch.int64, device=env.device)
                self._elog = torch.zeros((L, M, ELOG), dtype=torch.int64, device=env.device)
            if want_rows and (getattr(self, "_best_rows", None) is None or self._best_rows[0].shape[1] != T):
                self._best_rows = tuple(torch.zeros((M, T) + tuple(x.shape[2:]), dtype=x.dtype, device=env.device)
                                        for x in (logs.action, logs.p, logs.y, logs.reward))
        # ---- the counter table and the book of this block (one upload); PRE_EPISODE of its first episode is the host's
        for m in np.flatnonzero(active):
            self.agents[m](PRE_EPISODE_STAGE, env)          # host counters only (pop_sa)
        rows = np.zeros((M, ROW), dtype=np.int64)
        book = np.zeros((M, BOOK), dtype=np.int64)
        rows[:, GAMMA:ETA_C + 1] = self._hyper_rows()[:, :4].copy().view(np.int64)
        nblk = 0 if self.is_fluid else (env.random_init_coefficients() + 3) // 4     # (fluid: INIT_OFF / INIT_INC carry 0)
        as_bits = lambda v: int(np.array([v], dtype=np.float64).view(np.int64)[0])      # noqa: E731
        for m, (ag, hk) in enumerate(zip(self.agents, self.hooks)):
            pol, tr = ag.policy, ag.trajectory
            rows[m, [USTEP, NSA, NRT, NOISE, SAMPLE]] = (pol.update_step, tr.n_sa, tr.n_rt, pol._noise_off, pol._sample_off)
            rows[m, HALT], rows[m, ACTIVE] = (0, 1) if active[m] else (1, 0)
            rows[m, NOISE_AMP:LIMIT + 1] = np.array([float(pol.act_noise), float(pol.act_limit)], dtype=np.float64).view(np.int64)
            has, cmp = python_max_state(hk.rewards_compare)
            st = stops[m]
            kind, lim = (0, st.episode) if type(st) is StopAfterEpisode else (1, st.step)
            book[m, :BK_FIRED] = (hk.ep, hk.min_best_episode, int(bool(hk.collect_NNA)), has, as_bits(cmp), as_bits(hk.bestreward),
                                  hk.bestepisode, kind, st.cur, lim, int(bool(hk.use_random_init)), hk.init_seed, 0 if self.is_fluid else hk._init_off, nblk)
        _lib.check(lib.pdec_population_bp_sel(self._h, rows.ctypes.data_as(C.c_void_p), 0))
        start = rows.copy()
        with _on_stream(s_upd):
            self.rows.copy_(torch.from_numpy(rows))
            self._book.copy_(torch.from_numpy(book))
        any_random = bool(book[:, BK_RANDOM_INIT].any())
        tables = rngs = rng_states = None
        if self.is_fluid:
            # the vortex tables of the whole block from the members' own generators (one upload); the generators are set back
            # to what each member consumed when the block is settled.  err[e, m]: error_detection behind episode e's close
            if any_random:
                rngs = [hk.init_rng if (active[m] and hk.use_random_init) else None for m, hk in enumerate(self.hooks)]
                tab, rng_states = draw_block_tables(self.setup, rngs, L, self._ic_case())
                with _on_stream(s_env):
                    tables = torch.from_numpy(tab).to(env.device)
            detect = any(self._own_error_detection(self.hooks[m]) for m in np.flatnonzero(active))
            with _on_stream(s_env):
                if getattr(self, "_err", None) is None or self._err.shape[0] < L:
                    self._err = torch.zeros((L, M), dtype=torch.int32, device=env.device)
                self._err.zero_()
        reset_post = int(self.agents[0].policy.reset_stage == POST_EPISODE_STAGE)
        ysz, ssz = env.y[0].numel(), env.state[0].numel()
        ev_act, ev_env = _Event(lib), _Event(lib)
        for e in range(L):
            _join(s_upd, s_env)
            self._open_episode(any_random, tables[e] if tables is not None else None)
            with _on_stream(s_env):
                logs.y[0].copy_(env.y)
                logs.state[0].copy_(env.state)
                flags.zero_()
            _join(s_upd, s_env)
            # (per step: the member-indexed glue and update on the networks' stream, the member-layout env step on the env's)
            for t in range(T):
                _lib.check(lib.pdec_population_glue(self._h, 0, P(logs.reward[t - 1]) if t else None, P(flags[t - 1]) if t else None,
                                                    P(logs.state[t]), P(logs.action[t + 1])))
                ev_act.record(s_upd)
                ev_act.wait(s_env)
                _lib.check(lib.pdec_population_update(self._h))
                _lib.check(lib.pdec_env_step(env.handle, P(logs.y[t]), P(logs.action[t + 1]), P(logs.action[t]), P(logs.state[t]),
                                             P(logs.y[t + 1]), P(logs.p[t]), P(logs.state[t + 1]), P(logs.reward[t]), P(flags[t])))
                ev_env.record(s_env)
                ev_env.wait(s_upd)
            _lib.check(lib.pdec_population_glue(self._h, 1, P(logs.reward[T - 1]), P(flags[T - 1]), None, None))   # the time-out push
            # ---- the boundary, all on the networks' stream: close (hook, stop rule, final y / state), the POST_EPISODE push of
            # the final states, the best episode's rows, the hooks' actor copies, then the counters of the next episode
            with _on_stream(s_upd):
                # the per-step episode reward of PDEhook (mean over the actuators), member-major rows as a B = 1 run reduces them
                means = logs.reward.transpose(0, 1).contiguous().reshape(M * T, -1).mean(dim=1)
            close = (P(self._elog[e]), P(flags), P(means), T, P(logs.y), P(logs.state), P(env.y), P(env.state), ysz, ssz,
                     P(self._which), reset_post, int(e == L - 1))
            _lib.check(lib.pdec_population_episode_close(self._h, 0, P(self._book), *close))
            _lib.check(lib.pdec_population_glue(self._h, 2, None, None, P(env.state), None))
            if want_rows:
                la, lp, ly, lr = logs.action, logs.p, logs.y, logs.reward
                _lib.check(lib.pdec_population_copy_best_rows(
                    self._h, P(self._which), P(self._elog[e]), T, P(la), P(lp), P(ly), P(lr), *[P(b) for b in self._best_rows],
                    la[0, 0].numel(), lp[0, 0].numel(), ly[0, 0].numel(), lr[0, 0].numel()))
            _lib.check(lib.pdec_population_copy_actors(self._h, P(self._which)))
            _lib.check(lib.pdec_population_episode_close(self._h, 1, P(self._book), *close))
            if self.is_fluid and detect:
                # on the environment's stream, behind the close launch (which wrote env.y) and before the next initialiser
                s_env.wait_stream(s_upd)
                _lib.check(lib.pdec_fluid_error_detection(env.handle, P(env.y), P(self._err[e])))
        if self.is_fluid:
            s_upd.wait_stream(s_env)
        with _on_stream(s_upd):
            parts = [self.rows.view(-1), self._book.view(-1), self._elog[:L].reshape(-1)]
            if self.is_fluid:
                parts.append(self._err[:L].reshape(-1).to(torch.int64))
            pack = torch.cat(parts)
            t1 = time.perf_counter()
            host = pack.cpu().numpy()                                          # the one read-back of the block
        t2 = time.perf_counter()
        s_env.wait_stream(s_upd)
        rows_out = host[:M * ROW].reshape(M, ROW).copy()
        book_out = host[M * ROW:M * (ROW + BOOK)].reshape(M, BOOK)
        elog = host[M * (ROW + BOOK):M * (ROW + BOOK) + L * M * ELOG].reshape(L, M, ELOG)
        err = host[M * (ROW + BOOK) + L * M * ELOG:].reshape(L, M) if self.is_fluid else None
        # ---- settle every member for the whole block: the schedule of each episode at its logged number of steps, with the
        # boundary movements between them, must end at the device's counters
        pol0, tr0 = self.agents[0].policy, self.agents[0].trajectory
        was = np.flatnonzero(active)
        ran = elog[:, :, EL_RAN] != 0
        if not (ran[0] == active).all() or (ran[1:] & ~ran[:-1]).any():
            raise RuntimeError("Population: the device's episode log disagrees with the members that were active")
        cur = start[:, :SAMPLE + 1].copy()
        for e in range(L):
            n_of = elog[e, :, EL_STEPS].copy()
            self.episode_steps.append(n_of)
            idx = np.flatnonzero(ran[e])
            sched = _episode_schedule(cur, T, cols, pol0.behavior_actor.model.dims[-1], tr0.capacity, tr0.stride, pol0.update_after,
                                      pol0.update_freq, pol0.update_loops, pol0.batch_size, pol0.start_steps)
            cur[idx] = sched.after[idx, n_of[idx] - 1]
            cur[idx, NSA] += cols                               # POST_EPISODE: the final state with the zero action
            if reset_post:
                cur[idx, USTEP] = 0
            if e + 1 < L:                                       # PRE_EPISODE pop of the members that go on
                go = idx[ran[e + 1, idx] & (cur[idx, NSA] > cur[idx, NRT])]
                cur[go, NSA] -= tr0.stride
        for m in was:
            if cur[m].tolist() != rows_out[m, :SAMPLE + 1].tolist():
                raise RuntimeError(f"Population: member {m}'s device counters disagree with its executed steps of the block")
        _lib.check(lib.pdec_population_bp_sel(self._h, rows_out.ctypes.data_as(C.c_void_p), 1))
        rewards = elog[:, :, EL_REWARD].copy().view(np.float64)
        changed = []
        for m in was:
            ag, hk, bk = self.agents[m], self.hooks[m], book_out[m]
            pol, tr = ag.policy, ag.trajectory
            pol.update_step, tr.n_sa, tr.n_rt, pol._noise_off, pol._sample_off = rows_out[m, :SAMPLE + 1].tolist()
            for e in np.flatnonzero(ran[:, m]):
                r = float(rewards[e, m])
                if elog[e, m, EL_STEPS] == T and hk.ep >= hk.min_best_episode:
                    hk.rewards_compare.append(r)
                # PDEhook.end_episode: an episode that ended early and is errored, noted before ep advances
                if err is not None and elog[e, m, EL_STEPS] < T and err[e, m] and self._own_error_detection(hk):
                    hk.errored_episodes.append(hk.ep)
                hk.rewards.append(r)
                hk.ep += 1
            if hk.ep != int(bk[BK_EP]):
                raise RuntimeError(f"Population: member {m}'s device episode index disagrees with its episode log")
            hk.bestreward = float(bk[BK_BESTREWARD:BK_BESTREWARD + 1].view(np.float64)[0])
            hk.bestepisode = int(bk[BK_BESTEPISODE])
            stops[m].cur = int(bk[BK_STOP_CUR])
            if not self.is_fluid:
                hk._init_off = int(bk[BK_INIT_OFF])
            best_e = np.flatnonzero(elog[:, m, EL_NEW_BEST])
            if best_e.size and hk.collect_bestDF:
                changed.append((m, int(elog[best_e[-1], m, EL_STEPS])))
            if not rows_out[m, ACTIVE]:
                active[m] = False
        if rngs is not None:
            restore_block_rngs(rngs, rng_states, ran.sum(axis=0))
        if changed:                                             # the best episodes' rows, through the hook's own row path
            with _on_stream(s_upd):
                ii = torch.as_tensor([m for m, _ in changed], device=env.device)
                ba, bp, by, br = (b.index_select(0, ii).cpu() for b in self._best_rows)
            for j, (m, n) in enumerate(changed):
                hk = self.hooks[m]
                hk._rows_bulk = (list(range(1, n + 1)), ba[j, :n], bp[j, :n], by[j, :n], br[j, :n])
                hk._flush(env)
                hk.bestDF, hk.currentDF = list(hk.currentDF), []
        t3 = time.perf_counter()
        tm = self.timing
        tm["episodes"] += L
        tm["blocks"] = tm.get("blocks", 0) + 1
        tm["issue_s"] += t1 - t0
        tm["readback_s"] += t2 - t1
        tm["settle_s"] += t3 - t2
