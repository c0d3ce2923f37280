"""Evaluation of a population: every member's actor scored on the SAME held-out initial fields.

evaluate_actors drives one of three routes, which give the same numbers member by member and bit for bit:
  one launch        pdec_rollout_members serves all M episodes in ONE persistent launch (KS and 1-D Keller-Segel, per-actuator
                    actors of <= 3 layers no wider than 32; workgroups as member_workgroups lays them out);
  batched           the fluid and the 2-D Keller-Segel: the same call enqueues ONE step loop on the B = M K environment, the member
                    acting kernel (act_members_tiles: its tile plan) in the place of the acting call;
  member by member  everything else: M env.rollout calls on one B = K environment, with actor clones as testrun makes them.
A sweep over disturbance amplitudes (`mu`) or fault scenarios (`faults`) gives every member n blocks of K trajectories; each
(member, block) pair is an entry of its own in the launch's actor table."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .env import PDEenv, _on_stream
from .pipeline_eval import held_out_fields

NOT_SERVED, ONE_LAUNCH, BATCHED = 0, 1, 2       # what pdec_rollout_members reports in `served`
_LOG_KEYS = ("y", "p", "action", "reward")


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


def _best_first(score):
    """the indices of `score` best first, NaN last, ties by index"""
    keys = [(True, 0.0, m) if np.isnan(s) else (False, -s, m) for m, s in enumerate(score)]
    return sorted(range(len(keys)), key=keys.__getitem__)


def score_members(episode_reward, done_step):
    """score [M] and order of a population from episode_reward [M, K] and done_step [M, K] (host arrays): a member's score is
    the mean of its K episode rewards, NaN when any of its trajectories blew up (done_step >= 0) or is not finite; order =
    member indices best first, NaN scores last, ties by index."""
    er = np.asarray(episode_reward, dtype=np.float64)
    ds = np.asarray(done_step)
    bad = (ds >= 0).any(axis=1) | ~np.isfinite(er).all(axis=1)
    score = np.where(bad, np.nan, np.where(bad[:, None], 0.0, er).mean(axis=1))
    return score, _best_first(score)


def _model(actor):
    return getattr(actor, "model", actor)


def _handle_int(model):
    return int(getattr(model.handle, "value", model.handle))


def _has_persistent_rollout(setup):
    """the 2-D environments and the global agent have no persistent rollout at all"""
    return not (getattr(setup, "is_fluid", False) or getattr(setup, "is_kseg2d", False) or getattr(setup, "mono", False))


def _has_batched_rollout(setup):
    """the two 2-D environments with per-actuator agents: no persistent rollout, but pdec_rollout_members enqueues ONE step loop on
    the B = M K environment for them (served = BATCHED), the member acting kernel in the place of the acting call"""
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


def _sweep_blocks(setup, mu, faults):
    """(mus, scen): the amplitudes of a `mu` sweep as floats, the scenarios of a `faults` sweep as arrays; None where not asked for"""
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
    return mus, scen


def _entries_env(setup, y0, M, n_blk, mus, scen, control_from, dtype, device, stream):
    """the call's own environment of B = M n_blk K trajectories, member m's block laid out [n_blk][K]: trajectory (m, j, k) starts
    from field k and carries amplitude / scenario j (the initial state is sensed through the faults)"""
    K = int(y0.shape[0])
    env = PDEenv(setup, B=M * n_blk * K, dtype=dtype, device=device, y0=y0.repeat((M * n_blk,) + (1,) * (y0.dim() - 1)), stream=stream,
                 autoreset=False)
    if mus is not None:
        env.set_disturbance(torch.tensor(mus, dtype=torch.float64).repeat_interleave(K).repeat(M))
    if scen is not None:
        env.set_faults(**{k: torch.as_tensor(np.stack([sc[k] for sc in scen])).repeat_interleave(K, dim=0).repeat(M, 1)
                          for k in FAULT_KEYS})
        env.reset()
    if control_from:
        _lib.check(env.lib.pdec_env_set_control_from(env.handle, control_from))
    return env


def _other_streams(models, s_env):
    """the actors' streams that are not the environment's"""
    streams = [getattr(md, "stream", None) for md in models]
    return list({s.cuda_stream: s for s in streams if s is not None and s.cuda_stream != s_env.cuda_stream}.values())


def _rollout_members(env, models, K, T, act_limit, log, stream, s_env, others):
    """the one-launch and the batched route: pdec_rollout_members on the B = len(models) K environment.  Returns (rows, served);
    NOT_SERVED: nothing was enqueued"""
    setup, B, dev = env.setup, len(models) * K, env.device
    kw = dict(dtype=env.dtype, device=dev)
    with _on_stream(stream):
        out = dict(reward_sum=torch.zeros((B, setup.reward_len), **kw), done_step=torch.zeros(B, dtype=torch.int32, device=dev))
        done_any = torch.zeros(B, dtype=torch.int32, device=dev)
        if log:
            out.update(y=torch.empty((T,) + env._yshape, **kw), p=torch.empty((T,) + env._pshape, **kw),
                       action=torch.empty((T,) + env._ashape, **kw), reward=torch.empty((T, B, setup.reward_len), **kw))
    handles = (_lib.Handle * len(models))(*[_handle_int(md) for md in models])
    served = C.c_int(NOT_SERVED)
    P = _lib.ptr
    try:
        _lib.check(env.lib.pdec_rollout_members(
            env.handle, handles, len(models), K, T, P(env.y), P(env.state), P(env.action), float(act_limit), 0, P(out["reward_sum"]),
            P(out.get("y")), P(out.get("p")), P(out.get("action")), P(out.get("reward")), P(done_any), P(out["done_step"]),
            C.byref(served)))
    finally:
        for s in others:        # whatever next writes the actors' parameters waits for the launch that reads them
            s.wait_stream(s_env)
    return out, served.value


def _member_by_member(small, models, n_blk, K, T, mus, scen, act_limit, log, control_from, stream):
    """the third route: one rollout per (member, block) entry on the B = K environment `small`, a member's actor cloned once where
    its dtype or column capacity does not fit"""
    cols = K * small.setup.state_shape[1]
    parts = []
    for v, md in enumerate(models):
        if v % n_blk == 0:
            actor = md if (md.dtype == small.dtype and md.max_cols >= cols) else md.clone(dtype=small.dtype, max_cols=cols)
        if mus is not None:
            small.set_disturbance(torch.full((K,), mus[v % n_blk], dtype=torch.float64))
        if scen is not None:
            small.set_faults(**{k: torch.as_tensor(scen[v % n_blk][k]).unsqueeze(0).repeat(K, 1) for k in FAULT_KEYS})
        small.reset()
        parts.append(small.rollout(actor, T, act_limit=act_limit, learning=False, log=log, control_from=control_from))
    with _on_stream(stream):
        return {k: torch.cat([p_[k] for p_ in parts], dim=0 if k in ("reward_sum", "done_step") else 1)
                for k in (("reward_sum", "done_step") + (_LOG_KEYS if log else ()))}


def _per_block(res, M, n_blk, T, stream):
    """a sweep's result: every [entries, ...] array as [M, n_blk, ...], the order by the mean score over the blocks"""
    with _on_stream(stream):
        for k in ("reward_sum", "done_step", "episode_reward"):
            res[k] = res[k].view((M, n_blk) + tuple(res[k].shape[1:]))
        for k in _LOG_KEYS:
            if k in res:
                res[k] = res[k].view((T, M, n_blk) + tuple(res[k].shape[2:]))
    res["score"] = res["score"].reshape(M, n_blk)
    res["order"] = _best_first(res["score"].mean(axis=1))       # NaN if any block's score is


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
    mus, scen = _sweep_blocks(setup, mu, faults)
    n_blk = len(scen) if scen is not None else (1 if mus is None else len(mus))     # blocks per member: amplitudes or scenarios
    models = [md for md in members for _ in range(n_blk)]       # one entry per (member, block) of K trajectories
    entries = len(models)
    for m, md in enumerate(members):
        if list(md.dims) != list(members[0].dims) or list(md.acts) != list(members[0].acts):
            raise _lib.PdecError(f"evaluate_actors: member {m}'s actor shape {list(md.dims)} / activations differ from member 0's "
                                 f"{list(members[0].dims)}: all members must have the same shape")
    control_from = int(control_from)
    dev = torch.device(device)
    small = None                # the B = K environment: draws the shared fields, and serves the member-by-member route
    T = int(round((setup.te - setup.t0) / setup.dt)) + 1 if steps is None else int(steps)
    with _on_stream(stream):    # (the environments' own tensors are made on their stream as well)
        if y0 is None:
            small, y0 = held_out_fields(setup, n_inits, init_seed, dtype, device, stream)   # (the draw of TrainPipeline(eval_every=...))
        y0 = (y0 if isinstance(y0, torch.Tensor) else torch.as_tensor(np.array(y0, copy=True))).to(device=dev, dtype=dtype).contiguous()
        K = int(y0.shape[0])
        env = None              # without a persistent rollout or a batched step loop no B = entries K environment is built to hear it
        if _has_persistent_rollout(setup) or _has_batched_rollout(setup):
            env = _entries_env(setup, y0, M, n_blk, mus, scen, control_from, dtype, device, stream)
    s_env = stream if stream is not None else torch.cuda.current_stream(dev)
    others = _other_streams(models, s_env)
    for s in others:
        s_env.wait_stream(s)
    out, route = (None, NOT_SERVED) if env is None else _rollout_members(env, models, K, T, act_limit, log, stream, s_env, others)
    if route == NOT_SERVED:
        if env is not None:
            env.close()
        if small is None:
            with _on_stream(stream):
                small = PDEenv(setup, B=K, dtype=dtype, device=device, y0=y0, stream=stream, autoreset=False)
        else:
            small.set_y0(y0)
        out = _member_by_member(small, models, n_blk, K, T, mus, scen, act_limit, log, control_from, stream)
    with _on_stream(stream):
        res = dict(reward_sum=out["reward_sum"].view(entries, K, -1), done_step=out["done_step"].view(entries, K))
        res["episode_reward"] = res["reward_sum"].mean(dim=2)
        for k in _LOG_KEYS:
            if k in out:
                res[k] = out[k].view((T, entries, K) + tuple(out[k].shape[2:]))
        host = (res["episode_reward"].double().cpu().numpy(), res["done_step"].cpu().numpy())     # (waits for the stream)
    res["score"], res["order"] = score_members(*host)
    if mus is not None or scen is not None:
        _per_block(res, M, n_blk, T, stream)
        res.update(dict(faults=scen) if mus is None else dict(mu=np.asarray(mus, dtype=np.float64)))
    res["one_launch"], res["batched"] = route == ONE_LAUNCH, route == BATCHED
    # (one launch: a setup with a persistent rollout, so no 2-D one; its KS form pairs trajectories, the Keller-Segel takes one each)
    in_pairs = route == ONE_LAUNCH and tuple(setup.y_shape) == (setup.nx,)
    res["workgroups"] = (len(member_workgroups(entries, K)) if in_pairs else entries * K) if route == ONE_LAUNCH else None
    if route != NOT_SERVED:
        env.close()
    if small is not None:
        small.close()
    return res
