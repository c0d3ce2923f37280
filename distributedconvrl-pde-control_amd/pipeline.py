"""The batched training step as a two-stream pipeline, eager or replayed from captured HIP graphs.

One control step keeps the reference's stage order -- act -> update -> env step (RL.jl's run loop through
src/PDEagent.jl:175-209, :342-418 and src/PDEenv.jl:195-241):

    env stream:     wait update_{k-1}  ->  act_k (actor forward + exploration noise + clamp)  ->  env_k (fused env step)
    update stream:  wait act_{k-1}     ->  update_k (critic half, actor half: 4 launches) on the transition of step k - LAG

The update needs nothing of step k (DDPG is off-policy; the reference samples its minibatches from a 150k-deep replay,
src/PDEagent.jl:317-340) and act_k reads a published copy of the actor that update_k does not write, so update_k runs
back to back behind update_{k-1} beside act_k / env_k; act_{k+1} follows update_k, exactly as `agent(env)` follows
`update!` in the run loop.  (update_k must follow act_{k-1}, the last reader of the image its actor half republishes;
env_{k-LAG}, its batch, precedes act_{k-1} on the env stream.)

Data-parallel runs (N > 1, policy-gradient-only exchange, frozen target networks): the all-reduce of the actor's gradient and
the ADAM launch that consumes it leave the update stream (`stream_ar`):

    update stream:  critic half_k -> [wait apply_{k-1}] actor pass_k -> slab reduction_k ---------> critic half_{k+1} -> ...
    side stream:                                                        wait reduction_k -> all-reduce_k -> ADAM(actor)_k

The critic half reads the TARGET actor only (a' = At(s'), src/PDEagent.jl:385), which never moves (quirk_frozen_targets), so
critic half_{k+1} does not depend on ADAM(actor)_k and hides the collective; the next readers of the updated actor -- act_{k+1} on
the env stream and actor pass_{k+1} -- wait for the event on the ADAM launch.  Same kernels, same arguments, same order of
arithmetic as the in-chain order: bit-identical (tests/test_gpu_pipeline.py, tests/test_aa_multirank_gpu.py).

Every buffer a step touches is a pure function of the step counter k (rings indexed by k mod 2 / 3 / 6) and every
per-step scalar lives on the device (noise counter: pdec_policy_act_rng_dev; ADAM beta powers), so the launch arguments
of step k + 6 are those of step k: chunks of 24 / 6 / 1 consecutive steps starting at each of the six ring phases are
captured ONCE into HIP graphs (pdec_capture_begin / _end) and replayed with one host call per chunk instead of ~12 ctypes
calls per step.  Inside a chunk the cross-stream events above become graph edges; a chunk forks the update branch off
the env stream at its first step and joins it at its last.  The first and the last step of an episode
(initial-condition pointers, time-out terminal flags; te / dt + 1 = 51 steps in scripts/KS/KS22) are issued eagerly.  Eager and replayed runs enqueue the same kernels with the same arguments and are
bit-identical (tests/test_gpu_agent.py).

Episode bookkeeping (opt-in; PDEhook's, src/PDEhook.jl:42-97): `log_episodes` keeps an episode ledger on the device -- one
small launch behind every env step adds the step's per-trajectory mean reward to an fp64 running return (a library call like
the others, so recorded steps and graphs carry it), and the episode's last step, which is eager, snapshots the parameters
its acting kernel read, writes the episode's row and makes the hook's best-episode decision without a read-back.
`random_init` draws a new initial field for every episode at its (eager) first step, on the env stream, before the acting
kernel reads it.

Greedy held-out evaluation (opt-in, `eval_every`; needs the ledger): behind the last step of every eval_every-th episode the
snapshot of that step is rolled out without noise on an environment of its own from K fixed held-out fields, and the ledger
scores it on the device -- per trajectory b, from the rollout's reward_sum [K][R] and done_step [K]: ret_b = (sum_a (double)
reward_sum[b][a]) / R in a order, blew_b = done_step[b] >= 0; score = (sum_b ret_b) / K in b order, NaN when any blew_b is set or
any ret_b is not finite (population.score_members' rule; `eval_score` restates it on the host).  Enqueued at the (eager) last
step, never inside a capture or a recorded step:

    env stream:   [wait eval_{n-1} done] -> pdec_ledger_eval_load (staging -> evaluation actor) -> event
    eval stream:  wait event -> reset the evaluation env to eval_y0 -> pdec_rollout -> pdec_ledger_eval_close -> done event

With eval_stream=None the eval stream is the env stream (behind the episode's last env step, no events).

Per-trajectory episodes (opt-in, episodes="per_trajectory"; csrc/episode_clock.hip): the episode boundary is decided on the device.
pdec_epclock_step right behind pdec_env_step -- on the ring slots of step k: rring, fring, tring, aring[k % 3], ybuf[(k+1) % 2],
sring[(k+1) % 6] -- ends the episode of every trajectory whose blow-up flag is raised or whose own clock has reached
episode_steps, in that step: terminal row, log entry, restart field and its features, zero action_prev (a ring of two buffers the
clock writes and the next env step reads).  The host schedules as for episode_steps = 0: only step 0 is a first step, there is no
last step, every other step is interior -- the same launch sequence, recorded and captured.  The batch-mean reward of the reward
broadcast is taken by pdec_reward_mean behind the clock, on the rows it has sanitised; the env step's reward partials are not armed.

n-step transitions (opt-in, n_step = n > 1; csrc/nstep.hip): one more launch on the env stream, pdec_nstep_step, behind everything
that writes the rows of step k -- pdec_env_step, the clock call, the ledger call, the last step's time-out fill -- and in front of
pdec_reward_mean.  It stores (s_k, a_k, r_k, t_k) in a device ring of depth n and writes nbatch[k % 3]: per column the transition that
starts at step u = k - n + 1 -- s_u, a_u, R = sum_{i <= m} gamma^i r_{u+i} up to the first terminal step u + m (m <= n - 1), T = 1 where
there was one.  update_k trains on nbatch[(k - LAG) % 3] with next_state = sring[(k - LAG + 1) % 6] and the scalar gamma_n; a cut
window has T = 1 and does not bootstrap, so one discount serves every column.  Every step emits cols transitions, each start once;
transitions that start before the last restart are not consumed: the first update is at k - LAG >= _first_tick + n - 1.  pdec_reward_mean
runs on the assembled reward and the env step's reward partials are not armed.  The ring position is a device counter, so recorded steps
and graphs carry the call.

Telemetry (opt-in, telemetry = N > 0; csrc/telemetry.hip): two more launches, each reducing what its stream has just written to one row
of doubles in a device ring of N rows.  pdec_telemetry_step sits on the env stream behind the n-step call -- behind everything step k
puts there -- and reads sring[(k+1) % 6], aring / rring / tring / fring[k % 3] as those calls leave them: reward mean / min / max,
action mean and saturation, the largest state entry, blown-up and terminal counts, non-finite counts.  pdec_telemetry_update sits on
the update stream behind the last launch of update_k (in front of the event act_{k+1} waits for where that event is a record; where it
rides on the update's own launch, an event of its own behind the telemetry launch orders it before the next chunk graph)
and reads the four networks' flat parameters and the loss pair: both losses, sum theta^2, the squared distance to the targets and to
the parameters at the previous call, the largest entry, non-finite counts.  It is issued at the updating steps with k % telemetry_every
== 0; telemetry_every divides the ring period, so a ring phase always holds the same calls.  The row counters live on the device and
are advanced by the one thread that writes the row, so no argument depends on the step and recorded steps and graphs carry both calls.
Nothing is read back until pipe.telemetry()."""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib

PERIOD = 6            # lcm of the ring lengths (2: y / published actor / beta-power and noise-counter slots; 3; 6)


class _Event:
    """device-scope event of the library (pdec_event_create: no system-scope fence), torch.cuda.Event-like surface"""

    def __init__(self, lib):
        self.lib, self.h = lib, _lib.Handle()
        _lib.check(lib.pdec_event_create(C.byref(self.h)))

    def record(self, stream):
        _lib.check(self.lib.pdec_event_record(self.h, C.c_void_p(stream.cuda_stream)))

    def wait(self, stream):
        _lib.check(self.lib.pdec_stream_wait_event(C.c_void_p(stream.cuda_stream), self.h))

    def __del__(self):
        try:
            self.lib.pdec_destroy(self.h)
        except Exception:
            pass


class _TorchEvent:
    """the same surface on a default torch event (diagnostic: PDEC_TORCH_EVENTS=1)"""

    def __init__(self, lib=None):
        self.ev = torch.cuda.Event()

    def record(self, stream):
        self.ev.record(stream)

    def wait(self, stream):
        stream.wait_event(self.ev)


class _Clock:
    """the episode clock of a pipeline (pdec_epclock_create), released with it"""

    def __init__(self, lib, env_handle, episode_steps, capacity, random_init, seed, rank, world):
        self.lib, self.h = lib, _lib.Handle()
        _lib.check(lib.pdec_epclock_create(C.byref(self.h), env_handle, int(episode_steps), int(capacity), int(bool(random_init)),
                                           int(seed), int(rank), int(world)))

    def __del__(self):
        try:
            self.lib.pdec_destroy(self.h)
        except Exception:
            pass


class _NStep:
    """the n-step object of a pipeline (pdec_nstep_create) on the env stream, released with it"""

    def __init__(self, lib, n, cols, ns, na, dtype, stream):
        self.lib, self.h = lib, _lib.Handle()
        _lib.check(lib.pdec_nstep_create(C.byref(self.h), int(n), int(cols), int(ns), int(na), _lib.dtype_code(dtype)))
        _lib.check(lib.pdec_set_stream(self.h, C.c_void_p(stream.cuda_stream)))

    def __del__(self):
        try:
            self.lib.pdec_destroy(self.h)
        except Exception:
            pass


class _Telemetry:
    """the telemetry object of a pipeline (pdec_telemetry_create), its step launch on the env stream, released with it"""

    def __init__(self, lib, capacity, B, cols, ns, na, dtype, actor_handle, critic_handle, stream):
        self.lib, self.h = lib, _lib.Handle()
        _lib.check(lib.pdec_telemetry_create(C.byref(self.h), int(capacity), int(B), int(cols), int(ns), int(na),
                                             _lib.dtype_code(dtype), actor_handle, critic_handle))
        _lib.check(lib.pdec_set_stream(self.h, C.c_void_p(stream.cuda_stream)))

    def __del__(self):
        try:
            self.lib.pdec_destroy(self.h)
        except Exception:
            pass


# the columns of a telemetry row, in the device's order (csrc/telemetry.hip)
TELEMETRY_STEP_COLUMNS = ("step", "reward_mean", "reward_min", "reward_max", "reward_nonfinite", "action_mean", "action_abs_mean",
                          "action_saturated", "state_abs_max", "state_nonfinite", "blown_up", "terminal")
TELEMETRY_UPDATE_COLUMNS = ("update", "critic_loss", "actor_loss", "actor_norm2", "critic_norm2", "actor_target_dist2",
                            "critic_target_dist2", "actor_step2", "critic_step2", "actor_abs_max", "critic_abs_max",
                            "actor_nonfinite", "critic_nonfinite")


class _Ledger:
    """the episode ledger of a pipeline (pdec_ledger_create), released with it"""

    def __init__(self, lib, env_handle, actor_handle, capacity):
        self.lib, self.h = lib, _lib.Handle()
        _lib.check(lib.pdec_ledger_create(C.byref(self.h), env_handle, actor_handle, int(capacity)))

    def __del__(self):
        try:
            self.lib.pdec_destroy(self.h)
        except Exception:
            pass


def eval_score(reward_sum, done_step):
    """(ret [K] float64, blew [K] bool, score) of one greedy evaluation from a rollout's host arrays reward_sum [K, R] and
    done_step [K], in the order of arithmetic of the device (module docstring; csrc/ledger.hip: ledger_eval_close_kernel)"""
    rs = np.asarray(reward_sum)
    K, R = rs.shape
    ret = np.zeros(K)
    for a in range(R):
        ret = ret + rs[:, a].astype(np.float64)
    ret = ret / float(R)
    blew = np.asarray(done_step).reshape(K) >= 0
    s = 0.0
    for v in ret:
        s += float(v)
    bad = bool(blew.any()) or not bool(np.isfinite(ret).all())
    return ret, blew, (float("nan") if bad else s / float(K))


class TrainPipeline:
    def __init__(self, env, agent, lag=2, episode_steps=51, stream_env=None, stream_upd=None, use_graphs=True,
                 chunks=(24, 6, 1), use_replay=False, noise_seed=1234, kick_env_after_critic=None, stream_ar=None,
                 ar_off_chain=None, log_episodes=0, min_best_episode=0, random_init=False, init_seed=0, init_rng=None,
                 init_rank=(0, 1), eval_every=0, eval_inits=8, eval_seed=0, eval_y0=None, eval_capacity=64, eval_stream=None,
                 best_by="train", noise_scale=None, episodes="lockstep", stagger=False, n_step=1,
                 telemetry=0, telemetry_every=1):
        """env: PDEenv on `stream_env`; agent: create_agent(..., stream=stream_upd).  lag: the update of step k trains on
        the transition of step k - lag (>= 1).  episode_steps: lock-stepped episodes of that many control steps (0: one
        endless episode): the last transition is terminal (done = time >= te, src/PDEenv.jl:227) and the next step starts
        from env.y0 (reset!, :183-193).  use_replay: route the update through the device-resident replay (row F1): every
        transition is pushed (src/PDEagent.jl:254-289) and the update trains on B * A transitions drawn from it
        (:317-340) instead of the B * A fresh ones (eager only).  stream_ar: a third stream for the gradient all-reduce + the
        actor's ADAM launch of a data-parallel run (module docstring); ar_off_chain: None = whenever that order is legal
        (split update, policy-gradient-only exchange, frozen targets, stream_ar given), False = keep the collective on the update
        stream, True = insist (raises when illegal).

        log_episodes = N > 0: the episode ledger (module docstring) keeps the last N episodes' per-trajectory returns and
        blow-up bits (episode_returns(), rewards) and the best actor (best_actor(), bestreward, bestepisode: an episode whose
        1-based number is >= min_best_episode and whose batch-mean return is >= every earlier such one, PDEhook.jl:65-76; a
        NaN mean is never chosen and does not block later episodes).  Needs episode_steps > 0.  With an active reducer the
        returns are this rank's trajectories and the best actor is not tracked.  An episode cut by reset_from() is not logged.
        random_init: every episode starts from a new field -- KS / Keller-Segel / 2-D Keller-Segel: env.random_init(init_seed,
        off), episode e of rank r of W (init_rank = (r, W)) drawing from off = (e W + r) * n with n = B ceil(nc / 4) the
        counters of one call, so W ranks of B trajectories draw together what one rank of W B draws ((0, 1): PDEhook's
        advance); the fluid draws the same way (n = B nv, pdec_fluid_ic_rng) unless an init_rng is given: then
        setup.random_init_device(env, init_rng), the host's table.  A field given to reset_from() is used as it is.
        A fluid environment must have the networks' dtype; its steps are never captured (use_graphs resolves to False).

        eval_every = N > 0: greedy held-out evaluation (module docstring) behind the last step of every episode whose 1-based
        number is a multiple of N -- one episode of episode_steps control steps, learning = 0, the policy's act_limit, on an
        environment of its own (B = K, the training env's setup and dtype) from the fields eval_y0 [K, ...], or, None,
        eval_inits fields drawn once as population.evaluate_actors draws its own (Philox stream (eval_seed, 0) of
        env.random_init; the fluid: setup.random_init_device(env, np.random.default_rng(eval_seed))).  pipe.eval_y0: the
        fields; pipe.eval_zero_score: the score of the zero action on them (an actor with all parameters 0, run once here).
        The last eval_capacity evaluations are kept: eval_returns(), eval_scores.  eval_stream: None = the env stream, or a
        stream that is neither the env nor the update stream (made by the same make_streams call) on which the evaluation
        runs beside training.  best_by: "train" -- best_actor() / bestreward / bestepisode follow the training return, as
        without evaluations -- or "eval": the hook's rule on the evaluation scores (episode >= min_best_episode, score not
        NaN and >= every earlier such score), keeping the evaluated parameters.  Needs log_episodes > 0 (the snapshot lives
        in the ledger), episode_steps > 0 and no active reducer.

        noise_scale = [B] (host array or device tensor): trajectory b explores at noise_scale[b] in the place of the policy's
        act_noise -- see set_noise_scale.  None: the policy's scalar.

        An environment that holds fault arrays (PDEenv.set_faults, called before the pipeline is made) needs no argument here:
        the arrays are read by the kernels, so eager steps, recorded calls and captured graphs all step through them, writing
        new values into them between two run() calls keeps the recorded steps and the graphs, the reset image of the episode
        start is featurized through them and the per-trajectory episode clock re-featurizes a restarted trajectory through its
        own sensor faults.  The evaluation environment (eval_every) is this pipeline's own and stays healthy.  (The flag-synchronised
        single-trajectory step of run(..., device_episodes) has no fault-carrying form; run() orders such an environment's streams
        with events.)

        episodes = "per_trajectory": every trajectory keeps its own episode clock on the device (csrc/episode_clock.hip;
        DESIGN.md 3.5).  One boundary call behind every env step ends the episode of trajectory b IN that step when its blow-up
        flag is raised or its clock reaches episode_steps: the row's transition is terminal, its return is logged, and the
        trajectory restarts from row b of env.y0 -- or, with random_init, from row b of env.random_init(init_seed, off) at
        off = (n W + r) B ceil(nc / 4), n the number of episodes b has finished: the field the lock-stepped pipeline draws for
        its episode n (the host-issued step 0 draws episode 0 through _draw_init).  The other trajectories go on.  The host
        schedules as for episode_steps = 0 -- step 0 is the only first step, every later one is interior -- so capture() and
        the recorded calls cover every step and chunks need not fit an episode.  stagger=True starts the clock of trajectory
        b at floor(b E / B): the time-outs spread evenly over the E phases of an episode (the first episode of b is shorter by
        that much and is logged with the steps it really took).  log_episodes = C > 0 is then the log capacity PER TRAJECTORY
        (finished_episodes(), episodes_finished); episode_returns() / rewards belong to the lock-stepped mode.  reset_from()
        sets every clock back to its initial value and drops the running returns.  The 1-D environments with per-actuator
        agents and memory_size = 0 only; not with use_replay, an active reducer, evaluations or best-actor tracking (score
        actors with population.evaluate_actors between run() calls).

        n_step = n > 1 (1 .. 32): the update trains on n-step transitions assembled on the device (module docstring;
        csrc/nstep.hip).  Step k emits, per column, the transition that starts at step k - n + 1: its state and action, the
        discounted sum of the rewards up to its first terminal step (at most n of them), terminal = 1 where the window was cut by
        one; the next state is the one-step batch's, sring[(k + 1) % 6].  update_k trains on the batch assembled at step k - lag
        with gamma_n (policy.y multiplied n times) in the place of policy.y, so the first update after a restart is n - 1 steps
        later than with n = 1.  pipe.n_step, pipe.gamma_n; pipe.nstep_batch(j): the batch assembled at step j.  Both episode
        modes, every environment, the ledger, evaluations, noise_scale and a reducer are served; use_replay=True is refused
        (the replay route pushes one-step rows).  n_step is run state of the pipeline: checkpoints do not store it.  n_step = 1
        builds nothing and issues the launches it always did.

        telemetry = N > 0: per-step training telemetry kept on the device (module docstring; csrc/telemetry.hip), the last N rows
        of each of two rings.  One row per control step -- step, reward_mean / _min / _max over the finite rewards and
        reward_nonfinite, action_mean / action_abs_mean over the driving row of every action column and action_saturated (columns
        with |a| >= policy.act_limit), state_abs_max, state_nonfinite, blown_up (trajectories), terminal (columns) -- and one row
        per recorded update -- update, critic_loss, actor_loss (- mean Q), and per network norm2 = sum theta^2, target_dist2 =
        sum (theta - theta_target)^2, step2 = sum (theta - theta_prev)^2, abs_max, nonfinite.  telemetry_every = m in {1, 2, 3, 6}:
        the update row is written at the updating steps k with k % m == 0 only (the update stream is the critical chain of the
        two-stream step); theta_prev is the parameters at the previous RECORDED update, so *_step2 then spans m updates (0 in the
        first row).  The step row is written at every step.  pipe.telemetry() synchronises and returns the rows;
        pipe.telemetry_reset() clears them; reset_from() leaves them alone and `step` keeps counting control steps.  Both episode
        modes, every environment, n_step, noise_scale, the ledger, evaluations and use_replay are served.  An active reducer is
        refused: the actor's apply runs on a side stream beside the next critic half there, and no point of one stream sees a
        consistent parameter set.  It is run state of the pipeline: checkpoints do not store it.  telemetry = 0 builds nothing and
        issues the launches it always did."""
        self._check_n_step(n_step, use_replay)
        self.n_step = int(n_step)
        self._check_telemetry(telemetry, telemetry_every, agent.policy.reducer)
        self.telemetry_capacity, self.telemetry_every = int(telemetry), int(telemetry_every)
        # pdec_policy_act_rng_dev reads the state ring in the actor's type: a fluid environment of another dtype cannot step.
        # Refused by name at the first run() / capture(), not here: an object of that combination may be constructed and asked
        # for its episode-start draw (tests/test_gpu_pipeline_episodes.py::test_random_inits_fluid does).
        self._dtype_refusal = None
        if getattr(env, "is_fluid", False) and env.dtype != agent.policy.behavior_actor.model.dtype:
            self._dtype_refusal = (f"TrainPipeline: the fluid environment ({env.dtype}) and the networks "
                                   f"({agent.policy.behavior_actor.model.dtype}) must have one dtype: the acting kernel reads "
                                   "the environment's state ring in the actor's type")
        self._check_episode_mode(env, agent, episodes, stagger, episode_steps, use_replay, eval_every, min_best_episode, best_by)
        self.per_traj, self.stagger = episodes == "per_trajectory", bool(stagger)
        self._check_eval_args(env, agent, episode_steps, stream_env, stream_upd, log_episodes, eval_every, eval_inits, eval_y0,
                              eval_capacity, eval_stream, best_by)
        self.env, self.agent, self.policy = env, agent, agent.policy
        self.lib = env.lib
        self.LAG = max(1, int(lag))
        assert self.LAG in (1, 2), "rings hold the last 3 transitions: lag 1 or 2"
        self.E = int(episode_steps)
        self.s_env = stream_env if stream_env is not None else env.stream
        self.s_upd = stream_upd if stream_upd is not None else self.policy.behavior_critic.model.stream
        if self.s_env is None or self.s_upd is None:
            raise _lib.PdecError("TrainPipeline needs explicit (non-default) streams for the environment and the networks")
        self.serial = self.s_env.cuda_stream == self.s_upd.cuda_stream
        self.use_replay = bool(use_replay)
        reducer = self.policy.reducer
        self.multi_rank = reducer is not None and reducer.active      # the split update sequence (N > 1, or forced)
        # the all-reduce + ADAM(actor) beside the next critic half instead of in front of it: legal when that critic half cannot
        # see the actor's update -- it reads the target actor, so the targets must be frozen -- and the critic is not exchanged
        self._ar_legal = (self.multi_rank and not reducer.reduce_critic and bool(self.policy.quirk_frozen_targets)
                          and stream_ar is not None and stream_ar.cuda_stream not in (self.s_upd.cuda_stream, self.s_env.cuda_stream))
        if ar_off_chain and not self._ar_legal:
            raise _lib.PdecError("TrainPipeline(ar_off_chain=True) needs an active reducer with reduce_critic=False, frozen target "
                                 "networks (quirk_frozen_targets) and a stream_ar that is neither the env nor the update stream")
        self._stream_ar = stream_ar
        self.ar_off_chain = self._ar_legal if ar_off_chain is None else bool(ar_off_chain)
        self.s_ar = stream_ar if self.ar_off_chain else None
        # a recorded step / a graph holds POINTERS: policy.update must hand the ring tensors through unchanged, which it
        # does only when no dtype conversion makes a temporary (`.to(dt).contiguous()` is the identity then)
        self._batch_aliases = env.dtype == self.policy.behavior_critic.model.dtype
        # (the fluid step forks its batch onto part streams and takes milliseconds: its steps are issued eagerly / from the
        # recorded calls, never from a captured graph)
        self.use_graphs = (bool(use_graphs) and not self.use_replay and not self.multi_rank and self._batch_aliases
                           and not env.is_fluid)
        self.chunks = tuple(sorted({int(c) for c in chunks if c == 1 or c % PERIOD == 0} | {1}, reverse=True))
        setup, B = env.setup, env.B
        ns, A = setup.state_shape
        self.cols = B * A
        self.ns, self.na = ns, setup.action_shape[0]
        dt, dev = env.dtype, env.device
        kw = dict(dtype=dt, device=dev)
        import os
        empty = (lambda shape, **k: torch.full(shape, float("nan"), **k)) if os.environ.get("PDEC_POISON") else torch.empty
        with torch.cuda.stream(self.s_env):
            self.ybuf = [empty(env._yshape, **kw) for _ in range(2)]
            self.sring = [empty(env._sshape, **kw) for _ in range(PERIOD)]
            self.aring = [torch.zeros(env._ashape, **kw) for _ in range(3)]
            self.rring = [torch.zeros((B, setup.reward_len), **kw) for _ in range(3)]
            self.fring = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3)]
            self.tring = [torch.zeros((B, setup.reward_len), **kw) for _ in range(3)]      # per-column terminal flags
            self.pbuf = torch.zeros(env._pshape, **kw)
            self.rbar = [torch.zeros(1, dtype=torch.float32, device=dev) for _ in range(3)]  # batch-mean reward of step k
            self.azero = torch.zeros(env._ashape, **kw)                                    # action0 of a fresh episode
            self.state0 = empty(env._sshape, **kw)
            # per-trajectory episodes: action_prev of step k, written by the clock of step k - 1 (the action ring slot is the
            # transition's action and keeps its values where a trajectory restarts)
            self.aprev = [torch.zeros(env._ashape, **kw) for _ in range(2)] if self.per_traj else None
            # n-step transitions: the batch assembled behind env step k (state, action, reward, terminal of the window that
            # starts at step k - n + 1), a ring of three like the one-step rows it replaces in the update
            self.nstep, self.nbatch = None, None
            if self.n_step > 1:
                self.nstep = _NStep(self.lib, self.n_step, self.cols, self.ns, self.na, dt, self.s_env)
                self.nbatch = [dict(state=torch.zeros((self.cols, self.ns), **kw), action=torch.zeros((self.cols, self.na), **kw),
                                    reward=torch.zeros(self.cols, **kw), terminal=torch.zeros(self.cols, **kw)) for _ in range(3)]
            self._telem = None
            if self.telemetry_capacity > 0:
                pol = self.policy
                self._telem = _Telemetry(self.lib, self.telemetry_capacity, B, self.cols, self.ns, self.na, dt,
                                         pol.behavior_actor.model.handle, pol.behavior_critic.model.handle, self.s_env)
                self._telem_nets = tuple(n.model.handle for n in (pol.behavior_actor, pol.behavior_critic, pol.target_actor,
                                                                  pol.target_critic))
        # the reference's reward broadcast (quirk) needs the batch-mean reward: reduced on the env stream
        # right behind the env step instead of by every workgroup of the critic pass
        # (not with reward groups: the critic call reduces the group means itself, CustomDDPGPolicy.reward_group)
        self.pre_rbar = (bool(self.policy.quirk) and dt == torch.float32 and not self.use_replay
                         and self.policy.reward_group is None)
        # interleave of the reward groups: the fresh batch holds column b A + a, the replay's minibatch is drawn at random
        self.reward_interleave = 1 if self.use_replay else A
        # ... and for the fused KS step + 3-layer fused critic without any extra launch: the env step leaves one reward sum
        # per workgroup, the critic pass adds them
        # (per-trajectory episodes: the partials are summed before the clock sanitises the rows of blown-up trajectories and
        # cannot be corrected afterwards -- the mean is taken by pdec_reward_mean behind the clock; n-step transitions: the
        # reward of the batch is the assembled one, whose mean pdec_reward_mean takes behind the n-step call)
        self.rpart, self.n_rpart = None, 0
        if self.pre_rbar and not self.per_traj and self.n_step == 1:
            npart = C.c_int()
            probe = torch.zeros(B, dtype=torch.float32, device=dev)
            ok = self.lib.pdec_env_set_reward_partials_out(env.handle, _lib.ptr(probe), C.byref(npart)) == 0
            hc = self.policy.behavior_critic.model.handle
            ok = ok and self.lib.pdec_ddpg_set_reward_partials(hc, _lib.ptr(probe), npart.value) == 0    # refused unless fused 3-layer
            self.lib.pdec_ddpg_set_reward_partials(hc, None, 0)
            self.lib.pdec_env_set_reward_partials_out(env.handle, None, None)
            if ok:
                self.n_rpart = npart.value
                self.rpart = [torch.zeros(self.n_rpart, dtype=torch.float32, device=dev) for _ in range(3)]
        import os
        Ev = _TorchEvent if os.environ.get("PDEC_TORCH_EVENTS") == "1" else _Event
        self.ev_fork = Ev(self.lib)
        self.ev_act = [Ev(self.lib), Ev(self.lib)]                  # act_k issued (env stream)
        self.ev_upd = [Ev(self.lib), Ev(self.lib)]                  # update_k issued (update stream)
        self.ev_graph = Ev(self.lib)                                # tail of the last graph launch (env stream)
        self.ev_mid = Ev(self.lib)                                  # critic half of update_k done (update stream)
        self.ev_push = [Ev(self.lib), Ev(self.lib)]                 # replay pushes of step k done (env stream)
        self.ev_samp = Ev(self.lib)                                 # replay sample of update_k done (update stream)
        self.ev_red = Ev(self.lib)                                  # actor gradient of update_k reduced (update stream) -> side stream
        self.ev_env = [Ev(self.lib), Ev(self.lib)]                  # env_k done (env stream; collective off the chain only)
        self.ev_tel = Ev(self.lib)                                  # telemetry launch behind update_k done (update stream, see _issue)
        # collective off the chain, two streams, LAG >= 2: both cross-stream waits of the update stream sit between the halves
        # of an update (between_halves) instead of one there and one at the top of the step
        self._mid_waits = self.ar_off_chain and not self.serial and self.LAG >= 2 and not self.use_replay
        self._samp_pending = False
        self._after_graph = False
        self.tick = 0             # control steps issued so far: every buffer of step k is indexed by k mod 2 / 3 / 6
        self.ep_start = 0         # tick of the first step of the current episode
        self.noise_seed = int(noise_seed)
        self.actor = self.policy.behavior_actor.model
        yes = C.c_int()
        _lib.check(self.lib.pdec_mlp_acts_on_published_copy(self.actor.handle, C.byref(yes)))
        # an actor whose acting kernel reads its parameters in place (2-layer / generic nets) must not be rewritten by the
        # update's actor half while act_k still runs: that half then waits for act_k (the fused 3-layer path reads a
        # published copy instead and needs no such edge)
        self.act_in_place = not bool(yes.value)
        # start env_k behind the critic half of update_k instead of beside the critic pass (see _issue); for the
        # reference-shaped 2-layer nets the env branch is as long as the whole update, so it is not held back there
        # (device replay: the sample of update_{k+1} waits for the pushes behind env_k, so a step held back behind the critic
        # half stalls the update stream -- 158.7 vs 129.1 us per step, r03cm -- and the step is enqueued at once there)
        self.kick_env_after_critic = ((not self.act_in_place and not self.use_replay) if kick_env_after_critic is None
                                      else bool(kick_env_after_critic))
        if os.environ.get("PDEC_KICK") in ("0", "1"):               # diagnostic override
            self.kick_env_after_critic = os.environ["PDEC_KICK"] == "1"
        # events attached to the reduction launches instead of recorded behind them (see _issue); PDEC_STOP_EVENTS=0: records
        # (N > 1: the launch that applies the update after the all-reduce carries the event, pdec_adam_polyak_step)
        self.stop_events = (self.rpart is not None and Ev is _Event and not self.serial
                            and os.environ.get("PDEC_STOP_EVENTS", "1") != "0")
        # The PDE step beside the fused 3-layer passes.  Round 2: its register form (92 VGPRs) could not share a SIMD with two
        # waves of the 222-VGPR critic pass, so the pipeline asked for the 64-VGPR form (csrc/ks_step.hip, SHARE) at priority 3.
        # Round 3: the passes are bounded to 208 allocated VGPRs (2 x 208 + 96 = 512), the register form fits beside them, and
        # at its own priority 1 it takes less from the passes: 117.7 -> 111.4 us per control step (r03bc).  PDEC_SHARE=1 asks for
        # the 64-VGPR form again.
        self.simd_sharing = False
        if not self.serial and self.rpart is not None and os.environ.get("PDEC_SHARE", "0") == "1":
            eff = C.c_int()
            _lib.check(self.lib.pdec_env_set_simd_sharing(env.handle, 1, C.byref(eff)))
            self.simd_sharing = bool(eff.value)
        self._sp_env, self._sp_upd = C.c_void_p(self.s_env.cuda_stream), C.c_void_p(self.s_upd.cuda_stream)
        self._sp_ar = C.c_void_p(self.s_ar.cuda_stream) if self.s_ar is not None else None
        self.graphs = {}          # (chunk, pos) -> graph handle
        self._progs = {}          # ring phase -> recorded library calls of an interior eager step
        # the recorded-call replay re-issues LIBRARY calls only: with torch events (PDEC_TORCH_EVENTS=1) the cross-stream
        # records / waits are torch calls it would not see, so it is off for that event type
        # N > 1: the gradient all-reduce is one more recorded call (a library call with NativeGradReducer, a noted torch call
        # with GradReducer -- _Lib.note), so the multi-rank pipeline issues its steps the same fast way
        # (device replay: the batch is the trajectory's fixed fp32 sample buffers, handed through unchanged to fp32 nets)
        aliases = (self.policy.behavior_critic.model.dtype == torch.float32) if self.use_replay else self._batch_aliases
        self.fast_eager = os.environ.get("PDEC_FAST_EAGER", "1") == "1" and Ev is _Event and aliases
        self._key = None          # per-step scalars baked into _progs / the graphs (see _scalar_key)
        self._recapture = False
        self._captured = False
        self.n_graph_launches = self.n_eager_steps = 0
        self.noise_scale = None   # set_noise_scale: float64 [B] on the device, read by every acting launch
        if noise_scale is not None:
            self.set_noise_scale(noise_scale)
        self._setup_episodes(log_episodes, min_best_episode, random_init, init_seed, init_rng, init_rank)
        self._setup_eval(eval_every, eval_inits, eval_seed, eval_y0, eval_capacity, eval_stream, best_by, Ev)
        self.reset_from(env.y0)
        self._keep_y0 = False

    @staticmethod
    def _check_n_step(n_step, use_replay):
        """the refusals of n_step, by name, before anything is allocated"""
        if isinstance(n_step, bool) or not isinstance(n_step, (int, np.integer)) or not 1 <= int(n_step) <= 32:
            raise _lib.PdecError(f"TrainPipeline(n_step={n_step!r}): an integer from 1 to 32")
        if int(n_step) > 1 and use_replay:
            raise _lib.PdecError(f"TrainPipeline(n_step={int(n_step)}): use_replay=True is not covered (the replay route pushes "
                                 "one-step rows)")

    @staticmethod
    def _check_telemetry(telemetry, telemetry_every, reducer):
        """the refusals of telemetry / telemetry_every, by name, before anything is allocated"""
        def integer(v):
            return not isinstance(v, bool) and isinstance(v, (int, np.integer))
        if not integer(telemetry) or int(telemetry) < 0:
            raise _lib.PdecError(f"TrainPipeline(telemetry={telemetry!r}): an integer >= 0, the ring capacity in rows")
        if not integer(telemetry_every) or int(telemetry_every) not in (1, 2, 3, 6):
            raise _lib.PdecError(f"TrainPipeline(telemetry_every={telemetry_every!r}): one of 1, 2, 3, 6 (a divisor of the ring "
                                 "period, so that a ring phase always holds the same calls)")
        if int(telemetry) > 0 and reducer is not None and reducer.active:
            raise _lib.PdecError(f"TrainPipeline(telemetry={int(telemetry)}): not available with an active reducer (the actor's "
                                 "apply may run on a side stream beside the next critic half: no point of one stream sees a "
                                 "consistent parameter set)")

    @staticmethod
    def _check_episode_mode(env, agent, episodes, stagger, episode_steps, use_replay, eval_every, min_best_episode, best_by):
        """the refusals of episodes="per_trajectory", by name, before anything is allocated"""
        if episodes not in ("lockstep", "per_trajectory"):
            raise _lib.PdecError(f"TrainPipeline(episodes={episodes!r}): 'lockstep' or 'per_trajectory'")
        if episodes == "lockstep":
            if stagger:
                raise _lib.PdecError("TrainPipeline(stagger=True) needs episodes='per_trajectory': lock-stepped episodes share one clock")
            return
        who = "TrainPipeline(episodes='per_trajectory')"
        setup = env.setup
        if getattr(env, "is_fluid", False):
            raise _lib.PdecError(f"{who}: the fluid environment is not covered (its step is a launch sequence with its own sensing)")
        if getattr(setup, "is_kseg2d", False):
            raise _lib.PdecError(f"{who}: the 2-D Keller-Segel environment is not covered (its step is a launch sequence with its "
                                 "own sensing)")
        if int(getattr(setup, "memory_size", 0)) > 0:
            raise _lib.PdecError(f"{who}: memory_size > 0 is not covered")
        if getattr(setup, "mono", False):
            raise _lib.PdecError(f"{who}: the global agent (mono) is not covered")
        if use_replay:
            raise _lib.PdecError(f"{who}: use_replay=True is not covered (the replay route pushes lock-stepped episodes)")
        reducer = agent.policy.reducer
        if reducer is not None and reducer.active:
            raise _lib.PdecError(f"{who}: not available with an active reducer")
        if int(eval_every) > 0 or int(min_best_episode) > 0 or best_by == "eval":
            raise _lib.PdecError(f"{who}: eval_every, min_best_episode and best_by='eval' are not available -- there is no common "
                                 "episode end to snapshot at; score actors with evaluate_actors between run() calls")
        if int(episode_steps) <= 0:
            raise _lib.PdecError(f"{who} needs episodes: episode_steps > 0")

    @staticmethod
    def _check_eval_args(env, agent, episode_steps, stream_env, stream_upd, log_episodes, eval_every, eval_inits, eval_y0,
                         eval_capacity, eval_stream, best_by):
        """the refusals of the evaluation arguments, by name, before anything is allocated"""
        if best_by not in ("train", "eval"):
            raise _lib.PdecError(f"TrainPipeline(best_by={best_by!r}): 'train' or 'eval'")
        if int(eval_every) < 0:
            raise _lib.PdecError(f"TrainPipeline(eval_every={eval_every}): a period >= 0")
        if int(eval_every) == 0:
            if best_by == "eval":
                raise _lib.PdecError("TrainPipeline(best_by='eval') needs evaluations: eval_every > 0")
            return
        if int(log_episodes) <= 0:
            raise _lib.PdecError("TrainPipeline(eval_every=...) needs the episode ledger, which holds the snapshot: log_episodes > 0")
        if int(episode_steps) <= 0:
            raise _lib.PdecError("TrainPipeline(eval_every=...) needs episodes: episode_steps > 0")
        reducer = agent.policy.reducer
        if reducer is not None and reducer.active:
            raise _lib.PdecError("TrainPipeline(eval_every=...) is not available with an active reducer: the ledger keeps no "
                                 "snapshot there")
        if int(eval_inits) < 1:
            raise _lib.PdecError(f"TrainPipeline(eval_inits={eval_inits}): at least one held-out field")
        if int(eval_capacity) < 1:
            raise _lib.PdecError(f"TrainPipeline(eval_capacity={eval_capacity}): at least one row")
        if eval_y0 is not None:
            shape = tuple(eval_y0.shape) if hasattr(eval_y0, "shape") else np.shape(eval_y0)
            if len(shape) != len(env._yshape) or shape[0] < 1 or shape[1:] != tuple(env._yshape[1:]):
                raise _lib.PdecError(f"TrainPipeline(eval_y0=...): expected shape (K,) + {tuple(env._yshape[1:])}, got {shape}")
        if eval_stream is not None:
            s_upd = stream_upd if stream_upd is not None else agent.policy.behavior_critic.model.stream
            s_env = stream_env if stream_env is not None else env.stream
            if s_upd is not None and eval_stream.cuda_stream == s_upd.cuda_stream and (
                    s_env is None or s_env.cuda_stream != s_upd.cuda_stream):
                raise _lib.PdecError("TrainPipeline(eval_stream=...): the update stream cannot carry the evaluation; None (the "
                                     "env stream) or a third stream")

    def _setup_eval(self, eval_every, eval_inits, eval_seed, eval_y0, eval_capacity, eval_stream, best_by, Ev):
        """the evaluation environment, actor, held-out fields and zero-action baseline (one synchronisation); nothing when off"""
        self.eval_every, self.best_by = int(eval_every), best_by
        self.n_evals = 0
        self.eval_env = self.eval_actor = self.eval_y0 = self.eval_zero_score = None
        self.s_eval = None
        if self.eval_every <= 0:
            return
        from .env import PDEenv
        from .nna import HipMLP
        env, lib = self.env, self.lib
        self.eval_capacity = int(eval_capacity)
        self.s_eval = eval_stream if eval_stream is not None else self.s_env
        self._eval_aside = self.s_eval.cuda_stream != self.s_env.cuda_stream
        s = self.s_eval
        with torch.cuda.stream(s):
            if eval_y0 is None:
                K = int(eval_inits)
                ee = PDEenv(env.setup, B=K, dtype=env.dtype, device=env.device, stream=s, autoreset=False)
                if env.is_fluid:
                    y0 = env.setup.random_init_device(ee, np.random.default_rng(int(eval_seed)))
                else:
                    y0 = torch.empty_like(ee.y)
                    ee.random_init(int(eval_seed), 0, out=y0)
                y0 = y0.clone()
            else:
                y0 = (eval_y0 if isinstance(eval_y0, torch.Tensor) else torch.as_tensor(np.array(eval_y0, copy=True)))
                y0 = y0.to(device=env.device, dtype=env.dtype).contiguous().clone()
                K = int(y0.shape[0])
                ee = PDEenv(env.setup, B=K, dtype=env.dtype, device=env.device, stream=s, autoreset=False)
            self.eval_env, self.eval_y0, self.eval_K = ee, y0, K
            m = self.actor
            cols = K * env.setup.state_shape[1]
            self.eval_actor = HipMLP(m.dims, m.acts, None, env.dtype, m.device, max(cols, m.max_cols), s)    # all parameters 0
            self._eval_rsum = torch.zeros((K, env.setup.reward_len), dtype=env.dtype, device=env.device)
            self._eval_done = torch.zeros((2, K), dtype=torch.int32, device=env.device)        # done_any, done_step
        _lib.check(lib.pdec_ledger_eval_attach(self.ledger.h, ee.handle, self.eval_actor.handle, self.eval_capacity))
        self.ev_eload, self.ev_edone = Ev(lib), Ev(lib)     # evaluation actor loaded (env stream) / evaluation closed (eval stream)
        self._eval_pending = False
        # the zero action on the same fields: the rollout of the all-zero actor the evaluation actor still is.  It also makes
        # every lazily created buffer of the rollout path, so that the evaluations of the run enqueue and return.
        self._eval_rollout()
        s.synchronize()
        self.eval_zero_score = eval_score(self._eval_rsum.cpu().numpy(), self._eval_done[1].cpu().numpy())[2]

    def _eval_rollout(self):
        """reset the evaluation env to eval_y0 and enqueue one greedy episode of the evaluation actor, on the eval stream"""
        ee, lib = self.eval_env, self.lib
        with torch.cuda.stream(self.s_eval):
            ee.y.copy_(self.eval_y0)
            _lib.check(lib.pdec_featurize(ee.handle, _lib.ptr(ee.y), None, _lib.ptr(ee.state)))
            ee.action.zero_()
            self._eval_rsum.zero_()
            self._eval_done.zero_()
            _lib.check(lib.pdec_rollout(ee.handle, self.eval_actor.handle, self.E, _lib.ptr(ee.y), _lib.ptr(ee.state),
                                        _lib.ptr(ee.action), 0.0, float(self.policy.act_limit), 0, 0, 0,
                                        _lib.ptr(self._eval_rsum), None, None, None, None, _lib.ptr(self._eval_done[0]),
                                        _lib.ptr(self._eval_done[1])))

    def _eval_load(self):
        """env stream, behind the snapshot of an evaluated episode's last step: the staged parameters -> the evaluation actor"""
        if self._eval_aside and self._eval_pending:
            self.ev_edone.wait(self.s_env)              # the previous evaluation still reads the actor being rewritten
        _lib.check(self.lib.pdec_ledger_eval_load(self.ledger.h))
        if self._eval_aside:
            self.ev_eload.record(self.s_env)

    def _eval_run(self, episode):
        """the evaluation of 1-based `episode`, on the eval stream (the env stream: behind the episode's last env step)"""
        if self._eval_aside:
            self.ev_eload.wait(self.s_eval)
        self._eval_rollout()
        with torch.cuda.stream(self.s_eval):
            _lib.check(self.lib.pdec_ledger_eval_close(self.ledger.h, _lib.ptr(self._eval_rsum), _lib.ptr(self._eval_done[1]),
                                                       self.n_evals, int(episode), self.min_best_episode))
        self.n_evals += 1
        if self._eval_aside:
            self.ev_edone.record(self.s_eval)
            self._eval_pending = True

    def _setup_episodes(self, log_episodes, min_best_episode, random_init, init_seed, init_rng, init_rank):
        env = self.env
        self.log_episodes, self.min_best_episode = int(log_episodes), int(min_best_episode)
        self.ledger, self.track_best, self.n_episodes = None, False, 0
        self.clock = self.clock0 = None
        if self.log_episodes < 0:
            raise _lib.PdecError(f"TrainPipeline(log_episodes={log_episodes}): a capacity >= 0")
        if self.log_episodes > 0 and not self.per_traj:
            if self.E <= 0:
                raise _lib.PdecError("TrainPipeline(log_episodes=...) needs episodes: episode_steps > 0")
            if self.multi_rank and self.min_best_episode != 0:
                raise _lib.PdecError("TrainPipeline: best-actor tracking (min_best_episode) is not available with an active "
                                     "reducer: each rank would choose on its own trajectories")
            self.track_best = not self.multi_rank
            self.ledger = _Ledger(self.lib, env.handle, self.actor.handle if self.track_best else 0, self.log_episodes)
        self.random_init = bool(random_init)
        self.init_seed = int(init_seed)
        self.init_rng = init_rng          # the fluid: None = the device draw of env.random_init, else random_init_device(env, rng)
        r, W = (int(v) for v in init_rank)
        if not 0 <= r < W:
            raise _lib.PdecError(f"TrainPipeline(init_rank={tuple(init_rank)}): rank r of W needs 0 <= r < W")
        self.init_rank = (r, W)
        self.init_offsets = []        # Philox offset of every initial field drawn (KS / Keller-Segel)
        self._init_ep = 0
        if self.random_init:
            if env.is_fluid:
                if init_rng is not None and not hasattr(env.setup, "random_init_device"):
                    raise _lib.PdecError("TrainPipeline(random_init=True): the setup has no random_init_device")
            elif not getattr(env.setup, "device_random_init", True):
                raise _lib.PdecError("TrainPipeline(random_init=True): the setup has no device initialiser")
            if env.y0.data_ptr() == env.y.data_ptr():
                env.y0 = env.y0.clone()
        if self.per_traj:
            self.clock = _Clock(self.lib, env.handle, self.E, max(1, self.log_episodes), self.random_init, self.init_seed, r, W)
            B = env.B
            self.clock0 = np.array([(b * self.E) // B if self.stagger else 0 for b in range(B)], dtype=np.int32)

    def _draw_init(self):
        """a new initial field into env.y0 and its features into state0, on the env stream (the first step of an episode)"""
        env = self.env
        with torch.cuda.stream(self.s_env):
            if env.is_fluid and self.init_rng is not None:
                env.y0.copy_(env.setup.random_init_device(env, self.init_rng))
            else:
                r, W = self.init_rank
                n = env.B * ((env.random_init_coefficients() + 3) // 4)
                off = (self._init_ep * W + r) * n
                env.random_init(self.init_seed, off, out=env.y0)
                self.init_offsets.append(off)
            _lib.check(self.lib.pdec_featurize(env.handle, _lib.ptr(env.y0), None, _lib.ptr(self.state0)))
        self._init_ep += 1

    def set_ar_order(self, off_chain):
        """switch between the two places of the gradient all-reduce (module docstring) in a running pipeline: drains the
        streams, drops the recorded steps.  Both orders compute the same numbers; a caller times both and keeps the faster
        (bench.py: a collective of a few microseconds is cheaper left on the chain than two stream hops are)."""
        off_chain = bool(off_chain)
        if off_chain and not self._ar_legal:
            raise _lib.PdecError("set_ar_order(True): not legal for this pipeline (see TrainPipeline(ar_off_chain=...))")
        self.sync()
        self.ar_off_chain = off_chain
        self.s_ar = self._stream_ar if off_chain else None
        self._sp_ar = C.c_void_p(self.s_ar.cuda_stream) if self.s_ar is not None else None
        self._mid_waits = self.ar_off_chain and not self.serial and self.LAG >= 2 and not self.use_replay
        self._mid_wait_prev = False
        self._progs = {}

    # ------------------------------------------------------------------ state
    def reset_from(self, y0):
        """(re)start: the next step is the first of an episode from initial condition y0 ([B, ...] device tensor)"""
        env = self.env
        self._keep_y0 = True          # (random_init: this episode starts from y0, the next ones draw again)
        if self.ledger is not None and self.tick > self.ep_start:
            _lib.check(self.lib.pdec_ledger_discard(self.ledger.h))      # the cut episode is not logged
        if self.clock is not None:                                       # (nor are the cut episodes of the clock)
            _lib.check(self.lib.pdec_epclock_set(self.clock.h, _lib.ptr(self.clock0)))
        with torch.cuda.stream(self.s_env):
            if y0.data_ptr() != env.y0.data_ptr():
                env.y0.copy_(y0)
            _lib.check(self.lib.pdec_featurize(env.handle, _lib.ptr(env.y0), None, _lib.ptr(self.state0)))
        self.ep_start = self.tick
        if self.tick > 0:
            # a restart in the middle of an episode: the transitions of the steps before it must not be trained on -- the
            # first step of the new episode overwrites sring[tick % 6], which is the next_state of transition tick - 1 and
            # would be bootstrapped across the reset with terminal = 0 -- and the recorded interior steps are dropped
            self._first_tick = self.tick
            self._progs = {}
            tr = self.agent.trajectory
            if self.use_replay and tr.n_rt > 0 and tr.n_sa == tr.n_rt:
                # device-replay route: transition tick-1 is already in the ring with terminal = 0 and no
                # POST_EPISODE dummy follows it, so the first (s, a) row of the new episode becomes its next_state and later
                # samples would bootstrap across the reset.  Its rows are cut off instead: terminal = 1 (the layout a regular
                # episode end leaves once its dummy row has been popped and overwritten).  On the env stream, behind the pushes.
                with torch.cuda.stream(self.s_env):
                    lo = (tr.n_rt - self.cols) % tr.capacity
                    tr.terminal[lo:lo + self.cols].fill_(1.0)

    @property
    def y(self):
        return self.ybuf[self.tick % 2]

    @property
    def state(self):
        return self.sring[self.tick % PERIOD]

    # ------------------------------------------------------------------ one step, issued call by call
    def _issue(self, k, chunk_first=False, chunk_last=False):
        """enqueue control step k.  chunk_first / chunk_last: first / last step of a chunk being CAPTURED (fork / join of
        the update branch); both False for a step issued eagerly."""
        env, pol, lib, L = self.env, self.policy, self.lib, _lib
        first, last = self._first_last(k)
        y_in, y_out = self.ybuf[k % 2], self.ybuf[(k + 1) % 2]
        s_in, s_out = self.sring[k % PERIOD], self.sring[(k + 1) % PERIOD]
        act, act_prev = self.aring[k % 3], (self.aprev[k % 2] if self.per_traj else self.aring[(k - 1) % 3])
        rew, flags, term = self.rring[k % 3], self.fring[k % 3], self.tring[k % 3]
        capturing = chunk_first or chunk_last or self._capturing
        # greedy evaluation behind this step: the last step (eager) of an episode whose 1-based number is a multiple of eval_every
        evaluate = last and self.eval_every > 0 and (self.n_episodes + 1) % self.eval_every == 0
        mid_wait_prev, self._mid_wait_prev = self._mid_wait_prev, False
        if not self.serial:
            if chunk_first:                       # fork: everything before this chunk is ordered before it on the env stream
                self.ev_fork.record(self.s_env)
                self.ev_fork.wait(self.s_upd)
            elif capturing:
                self.ev_act[(k - 1) % 2].wait(self.s_upd)
                self.ev_upd[(k - 1) % 2].wait(self.s_env)
            else:                                 # eager
                if self._after_graph:             # the update branch of the graph just launched ran on the env stream
                    self.ev_graph.wait(self.s_upd)
                    self._after_graph = False
                elif k > 0:
                    # (collective off the chain: update_{k-1} waited for env_{k-2} between its halves, see between_halves)
                    if not mid_wait_prev:
                        self.ev_act[(k - 1) % 2].wait(self.s_upd)
                    self.ev_upd[(k - 1) % 2].wait(self.s_env)

        def act_part():
            nonlocal act_prev
            if self.serial and self.ar_off_chain and k > 0:
                self.ev_upd[(k - 1) % 2].wait(self.s_env)      # ADAM(actor)_{k-1} ran on the side stream
            with torch.cuda.stream(self.s_env):
                if first:                                  # reset!(env): this step starts from the initial condition
                    if self.random_init and not self._keep_y0:
                        self._draw_init()
                    self._keep_y0 = False
                    y_in.copy_(env.y0)
                    s_in.copy_(self.state0)
                    act_prev = self.azero
                # actor forward on all B*A columns + exploration noise (Philox, counter on the device) + clamp: one launch
                L.check(lib.pdec_set_stream(self.actor.handle, self._sp_env))
                L.check(lib.pdec_policy_act_rng_dev(self.actor.handle, L.ptr(s_in), self.cols, float(pol.act_noise),
                                                    float(pol.act_limit), 1, self.noise_seed, L.ptr(act)))
                L.check(lib.pdec_set_stream(self.actor.handle, self._sp_upd))
                if last and self.track_best:
                    # what this acting kernel read, before the actor half that waits for ev_act may rewrite it
                    L.check(lib.pdec_ledger_snapshot(self.ledger.h))
                    if evaluate:
                        self._eval_load()
                if not self.serial and self.LAG >= 2:
                    self.ev_act[k % 2].record(self.s_env)
            if self.drain_between:
                torch.cuda.synchronize()

        j = k - self.LAG
        # one stream + the collective off the chain: act_k needs ADAM(actor)_{k-1}, which waits for the all-reduce on the side
        # stream -- so the critic half of update_k, which needs neither, goes first and hides it (two streams: the critic half is
        # on the other stream anyway)
        late_env = self.serial and self.ar_off_chain and j >= self._first_update and not self.use_replay
        if not late_env:
            act_part()

        def env_part():
            with torch.cuda.stream(self.s_env):
                L.check(lib.pdec_env_set_terminal_out(env.handle, L.ptr(term)))
                if self.rpart is not None:
                    L.check(lib.pdec_env_set_reward_partials_out(env.handle, L.ptr(self.rpart[k % 3]), None))
                L.check(lib.pdec_env_step(env.handle, L.ptr(y_in), L.ptr(act), L.ptr(act_prev), L.ptr(s_in), L.ptr(y_out),
                                          L.ptr(self.pbuf), L.ptr(s_out), L.ptr(rew), L.ptr(flags)))
                if self.clock is not None:
                    # the episode boundary of every trajectory, decided on the device: the same call at every step
                    fixed = not self.random_init
                    L.check(lib.pdec_epclock_step(self.clock.h, L.ptr(rew), L.ptr(flags), L.ptr(term), L.ptr(act),
                                                  L.ptr(self.aprev[(k + 1) % 2]), L.ptr(y_out), L.ptr(s_out),
                                                  L.ptr(env.y0) if fixed else None, L.ptr(self.state0) if fixed else None))
                if self.ledger is not None:
                    L.check(lib.pdec_ledger_step(self.ledger.h, L.ptr(rew), L.ptr(flags)))
                if last:
                    term.fill_(1.0)                    # time-out: done = time >= te -> terminal transition
                    if self.ledger is not None:
                        L.check(lib.pdec_ledger_close(self.ledger.h, self.n_episodes, self.min_best_episode,
                                                      int(self.track_best)))
                        self.n_episodes += 1
                rew_batch = rew
                if self.nstep is not None:
                    # the transition that starts at step k - n + 1, from the rows as the calls above have left them
                    nb = self.nbatch[k % 3]
                    rew_batch = nb["reward"]
                    L.check(lib.pdec_nstep_step(self.nstep.h, L.ptr(s_in), L.ptr(act), L.ptr(rew), L.ptr(term), float(pol.y),
                                                L.ptr(nb["state"]), L.ptr(nb["action"]), L.ptr(rew_batch), L.ptr(nb["terminal"])))
                if self._telem is not None:
                    # one row of facts about step k's own rows (not the assembled batch), as the calls above have left them
                    L.check(lib.pdec_telemetry_step(self._telem.h, L.ptr(s_out), L.ptr(act), L.ptr(rew), L.ptr(term), L.ptr(flags),
                                                    float(pol.act_limit)))
                if self.pre_rbar and self.rpart is None:
                    L.check(lib.pdec_reward_mean(env.handle, L.ptr(rew_batch), self.cols, L.ptr(self.rbar[k % 3])))
                if self.use_replay:
                    # a host function with step-dependent ring positions: re-evaluated, not replayed verbatim (_Lib.note)
                    lib.note(self._replay_push, self.ev_push[k % 2], s_in, act, rew, term, s_out, first, last)
                if not self.serial and self.LAG < 2:
                    # LAG = 1: update_{k+1} trains on the transition env_k is producing, so the event it waits on is
                    # recorded behind the whole env branch, not behind the acting kernel
                    self.ev_act[k % 2].record(self.s_env)
                if self._mid_waits:
                    self.ev_env[k % 2].record(self.s_env)
            if evaluate:
                self._eval_run(self.n_episodes)        # (behind everything step k puts on the env stream)
            if self.drain_between:                     # kernel-timing pass: nothing of the env branch overlaps the update
                torch.cuda.synchronize()

        batch = None
        if j >= self._first_update:
            if self.use_replay:
                with torch.cuda.stream(self.s_upd):
                    lib.note(self._replay_sample, self.ev_push[(k - 1) % 2] if (not self.serial and k > 0) else None)
                batch = self._batch_cur
            elif self.nstep is not None:
                batch = dict(self.nbatch[j % 3], next_state=self.sring[(j + 1) % PERIOD].view(self.cols, self.ns))
            else:
                batch = dict(state=self.sring[j % PERIOD].view(self.cols, self.ns), action=self.aring[j % 3].view(self.cols, self.na),
                             reward=self.rring[j % 3].view(self.cols), terminal=self.tring[j % 3].view(self.cols),
                             next_state=self.sring[(j + 1) % PERIOD].view(self.cols, self.ns))
        # (inside a captured chunk the extra fork / join edge of the kick costs more than it gives: 202 vs 148 us per step)
        kick = self.kick_env_after_critic and batch is not None and not self.serial and not capturing
        if not kick and not late_env:
            env_part()

        def between_halves():
            if late_env:
                act_part()
                env_part()
            # Beside the critic pass the PDE step makes almost no progress and then collides with the whole actor pass;
            # released when the critic half (pass + reduction) is done it runs beside the actor pass, the second
            # reduction and the head of the next critic pass instead (r02i, same box: 152 -> 130 us per control step)
            if kick:
                if use_stop:
                    L.check(lib.pdec_mlp_flush_stop_event(pol.behavior_critic.model.handle))     # no-op when consumed
                else:
                    self.ev_mid.record(self.s_upd)
                self.ev_mid.wait(self.s_env)
                env_part()
            if self.act_in_place and not self.serial:
                self.ev_act[k % 2].wait(self.s_upd)
            if self.ar_off_chain and k > 0:
                # the actor pass reads the actor that ADAM(actor)_{k-1} on the side stream has written (done long ago: it ran
                # beside the critic half that has just ended) ...
                self.ev_upd[(k - 1) % 2].wait(self.s_upd)
                if self._mid_waits:
                    # ... and the wait for the batch of update_{k+1} -- env_{k-1}, done since the middle of this critic pass --
                    # sits here too, instead of at the top of step k + 1.  Why: every cross-stream wait is a barrier packet of
                    # 5 - 7 us on the update chain even when it is satisfied (measured: the step with either wait removed),
                    # two adjacent ones cost less than two apart (116.5 - 117.7 against 118 - 119 us per step), a single
                    # wait on act_k's event (which implies both) or on a join event made on the side stream stalls on events
                    # that complete just before they are needed (123 / 125 us) -- HISTORY.md 6.1
                    self.ev_env[(k - 1) % 2].wait(self.s_upd)
                    self._mid_wait_prev = True

        # eager steps on the fused 3-layer path: the two events the env stream waits for ride on the reduction launches' own
        # dispatch packets (pdec_mlp_set_stop_event) instead of being recorded as packets behind them
        use_stop = self.stop_events and batch is not None and not capturing and not self.serial
        if use_stop:
            if kick:
                L.check(lib.pdec_mlp_set_stop_event(pol.behavior_critic.model.handle, self.ev_mid.h))
            L.check(lib.pdec_mlp_set_stop_event(pol.behavior_actor.model.handle, self.ev_upd[k % 2].h))
        with torch.cuda.stream(self.s_upd):
            if batch is not None:
                if self.rpart is not None:
                    L.check(lib.pdec_ddpg_set_reward_partials(pol.behavior_critic.model.handle, L.ptr(self.rpart[j % 3]), self.n_rpart))
                elif self.pre_rbar:
                    L.check(lib.pdec_ddpg_set_reward_mean(pol.behavior_critic.model.handle, L.ptr(self.rbar[j % 3])))
                if self.ar_off_chain:
                    self._update_ar_off_chain(k, batch, between_halves, use_stop)
                elif kick or (self.act_in_place and not self.serial):
                    pol.update(batch, before_actor_half=between_halves, interleave=self.reward_interleave, gamma=self._gamma_arg)
                else:
                    pol.update(batch, interleave=self.reward_interleave, gamma=self._gamma_arg)
                if self._telem is not None and k % self.telemetry_every == 0:
                    # behind the last launch of update_k: the parameters and losses it leaves (a captured chunk joins through the
                    # event recorded below, so the call stays in front of it)
                    L.check(lib.pdec_telemetry_update(self._telem.h, *self._telem_nets, L.ptr(pol._losses)))
                    if use_stop:
                        # ev_upd[k % 2] rides on the update's own last launch and does not cover this one: a chunk graph launched
                        # on the env stream next -- whose update branch rewrites what this launch reads and shares its ticket,
                        # partials and counter -- waits for this event as well (_sync_streams_for_graph)
                        self.ev_tel.record(self.s_upd)
            if self.ar_off_chain and batch is not None:
                pass                                    # (the completion event was recorded on the side stream)
            elif use_stop:
                L.check(lib.pdec_mlp_flush_stop_event(pol.behavior_actor.model.handle))          # no-op when consumed
            elif not self.serial:
                self.ev_upd[k % 2].record(self.s_upd)
        if chunk_last and not self.serial:
            self.ev_upd[k % 2].wait(self.s_env)    # join: the graph ends on the env stream

    def _update_ar_off_chain(self, k, batch, between_halves, use_stop):
        """update_k of a data-parallel run with the collective off the update chain (module docstring).  On the update stream:
        critic half, actor pass, slab reduction (its completion = `ev_red`, riding on the reduction launch where the fused path
        allows); on the side stream behind that event: all-reduce of the flat actor gradient, then the ADAM launch -- issued
        through the actor's handles while they are set to the side stream -- whose completion is `ev_upd[k % 2]`, the event the
        next acting kernel (env stream) and the next actor pass (update stream) wait for."""
        pol, lib, L = self.policy, self.lib, _lib
        A, At = pol.behavior_actor.model, pol.target_actor.model
        pol.update_critic_half(batch, self.reward_interleave, self._gamma_arg)
        between_halves()
        red_on_launch = use_stop and lib.pdec_mlp_set_reduce_event(A.handle, self.ev_red.h) == 0
        pol.actor_grads(batch)                                      # (records a reduce event its launches did not carry)
        if not red_on_launch:
            self.ev_red.record(self.s_upd)
        self.ev_red.wait(self.s_ar)
        pol.reducer.all_reduce(A, stream=self.s_ar)
        L.check(lib.pdec_set_stream(A.handle, self._sp_ar))
        L.check(lib.pdec_set_stream(At.handle, self._sp_ar))
        try:
            pol.apply_actor()
            if use_stop:
                L.check(lib.pdec_mlp_flush_stop_event(A.handle))    # no-op when the ADAM launch carried ev_upd[k % 2]
            else:
                self.ev_upd[k % 2].record(self.s_ar)
        finally:
            L.check(lib.pdec_set_stream(A.handle, self._sp_upd))
            L.check(lib.pdec_set_stream(At.handle, self._sp_upd))

    _capturing = False
    _first_tick = 0
    _mid_wait_prev = False    # update_{k-1} waited for env_{k-2} between its halves (so step k needs no wait at its top)
    drain_between = False
    per_traj = False          # episodes="per_trajectory"
    n_step = 1
    nstep = None              # the n-step object (n_step > 1)
    telemetry_capacity, telemetry_every = 0, 1
    _telem = None             # the telemetry object (telemetry > 0)

    @property
    def _first_update(self):
        """the first transition after the last restart that an update may train on: the n-step window that ends at step j starts
        at j - n + 1, which must not precede the restart"""
        return self._first_tick + self.n_step - 1

    @property
    def gamma_n(self):
        """w_n of w_0 = 1, w_{i+1} = w_i policy.y: the discount of a full n-step window's bootstrap term, the product the
        assembling kernel forms"""
        w = 1.0
        for _ in range(self.n_step):
            w = w * float(self.policy.y)
        return w

    @property
    def _gamma_arg(self):
        return None if self.n_step == 1 else self.gamma_n

    def nstep_batch(self, j):
        """(state [cols, ns], action [cols, na], reward [cols], terminal [cols], next_state [cols, ns]) of the batch assembled at
        step j -- the transitions that start at step j - n_step + 1 -- as the device holds them (the ring of three: valid until
        step j + 3 is issued; the caller synchronises).  For tests and probes."""
        if self.nstep is None:
            raise _lib.PdecError("TrainPipeline.nstep_batch: n_step = 1 assembles nothing (the update reads the ring slots)")
        nb = self.nbatch[j % 3]
        return nb["state"], nb["action"], nb["reward"], nb["terminal"], self.sring[(j + 1) % PERIOD].view(self.cols, self.ns)

    @property
    def _E_host(self):
        """the episode length the HOST schedules by: with per-trajectory episodes the boundary is the clock's, and the host
        sees one endless episode (episode_steps = 0: step 0 is the only first step, every later one is interior)"""
        return 0 if self.per_traj else self.E

    def _first_last(self, k):
        """is step k the first / the last of an episode"""
        e, E = k - self.ep_start, self._E_host
        if E <= 0:
            return e == 0, False
        return e % E == 0, e % E == E - 1

    # ------------------------------------------------------------------ device replay route (row F1)
    def _replay_push(self, ev_done, s_in, act, rew, term, s_out, first, last):
        """the stage pushes of step k (src/PDEagent.jl:237-314).  They run on the ENV stream (launched through the env's
        handle), behind the env step / the time-out fill that produce their inputs; `ev_push[k % 2]` marks them done and
        the update that samples the replay next waits for it (see _issue).  (launched through the critic's
        handle they ran on the update stream, unordered against env_k, and copied stale rewards / flags.)"""
        tr, lib, h = self.agent.trajectory, self.lib, self.env.handle
        cap1 = tr.capacity + tr.stride
        ns, na = tr.state.shape[1], tr.action.shape[1]
        dtc = _lib.dtype_code(s_in.dtype)

        def push_sa(s, a):
            _lib.check(lib.pdec_replay_push_sa(h, _lib.ptr(tr.state), _lib.ptr(tr.action), cap1, ns, na, tr.n_sa % cap1,
                                               _lib.ptr(s.view(self.cols, self.ns)),
                                               None if a is None else _lib.ptr(a.view(self.cols, self.na)), self.cols, dtc))
            tr.n_sa += self.cols

        if self._samp_pending:
            self.ev_samp.wait(self.s_env)
            self._samp_pending = False
        if first and len(tr) > 0 and tr.n_sa > tr.n_rt:
            tr.pop_sa(tr.stride)                                    # PRE_EPISODE: the dummy (s, a) of the last episode
        push_sa(s_in, act)                                          # PRE_ACT
        # POST_ACT: reward and the per-column terminal flags the env step (and the time-out) produced -- two
        # one-column traces of equal capacity, pushed by the same two-trace kernel as (s, a)
        _lib.check(lib.pdec_replay_push_sa(h, _lib.ptr(tr.reward), _lib.ptr(tr.terminal), tr.capacity, 1, 1,
                                           tr.n_rt % tr.capacity, _lib.ptr(rew.view(self.cols)),
                                           _lib.ptr(term.view(self.cols)), self.cols, _lib.dtype_code(rew.dtype)))
        tr.n_rt += self.cols
        if last:
            push_sa(s_out, None)                                    # POST_EPISODE dummy
        if not self.serial:
            ev_done.record(self.s_env)

    def _replay_sample(self, ev_pushed):
        """the sampled batch of this step's update (pde_sample / pde_fetch!, src/PDEagent.jl:317-340) into the trajectory's
        fixed batch buffers -> self._batch_cur (None while the replay holds less than one step).  Re-evaluated at every step,
        recorded or not: the sample count, the ring fill and the Philox offset are host counters."""
        tr, pol = self.agent.trajectory, self.policy
        self._batch_cur = None
        if ev_pushed is not None:
            # the host counters the sample is drawn against already include env_{k-1}'s pushes: wait for them
            # (the update stream has otherwise only waited for act_{k-1}, which precedes them on the env stream)
            ev_pushed.wait(self.s_upd)
        if len(tr) <= tr.stride:
            return
        self._batch_cur = tr.sample_device(pol._sample_seed, pol._sample_off, self.cols, reuse=True)
        pol._sample_off += (self.cols + 3) // 4
        if not self.serial:
            # ... and env_k's pushes overwrite the oldest rows of a full ring: they wait for this sample
            self.ev_samp.record(self.s_upd)
            self._samp_pending = True

    # ------------------------------------------------------------------ graphs
    def capture(self):
        """record the chunk graphs (needs >= 3 warm-up steps behind it so that every lazily created buffer exists and
        the update has transitions to train on); advances the run by len(chunks) periods of eager-equivalent steps"""
        if self._dtype_refusal:
            raise _lib.PdecError(self._dtype_refusal)
        self._check_key()
        if not self.use_graphs or self._captured:
            return
        if self._E_host > 0:
            assert self.E > 2 * PERIOD, "episodes must be longer than two graph periods"
            self.chunks = tuple(c for c in self.chunks if c <= self.E - 2)
        while self.tick - self.LAG < self._first_update + 2:      # lazily created buffers / first-use uploads happen eagerly
            self._eager()
        self._key = self._scalar_key()
        for c in self.chunks:
            for pos in range(PERIOD):
                if not self._reachable(c, pos):
                    # e.g. chunk 24 with 26-step episodes: the interior offsets 1 .. E-1-c never meet this ring phase
                    # (the search below would issue eager steps for ever); run() falls back to a smaller chunk
                    continue
                while not (self.tick % PERIOD == pos and self._interior(self.tick, c)):
                    self._eager()
                self._sync_streams_for_graph()
                _lib.check(self.lib.pdec_capture_begin(self.env.handle))
                self._capturing = True
                try:
                    for i in range(c):
                        self._issue(self.tick + i, chunk_first=(i == 0), chunk_last=(i == c - 1))
                finally:
                    self._capturing = False
                    h = _lib.Handle()
                    _lib.check(self.lib.pdec_capture_end(self.env.handle, C.byref(h)))
                self.graphs[(c, pos)] = h
                # the capture recorded the steps without running them: replay once so that the run really advances
                self._launch(h)
                self.tick += c
        self._captured = True

    def _reachable(self, c, pos):
        """is there a future tick at ring phase `pos` from which c consecutive steps are interior to an episode?  The
        pattern of (tick mod 6, episode offset) repeats after lcm(E, 6) <= 6 E ticks."""
        E = self._E_host
        if E <= 0:
            return True
        t0 = max(self.tick, self._first_update + self.LAG)
        return any(t % PERIOD == pos and self._interior(t, c) for t in range(t0, t0 + PERIOD * E + PERIOD))

    def set_noise_scale(self, values):
        """Per-trajectory exploration amplitude: `values` [B], a host array (checked: finite, not negative) or a device tensor
        (copied device to device, no host wait; the caller orders its producer before the env stream), or None to return to
        policy.act_noise.  The values are written on the env stream INTO a buffer of B doubles that the pipeline owns
        (self.noise_scale) and that the acting launch reads at column (b A + a) // A = b (pdec_mlp_set_noise_scale), so the
        recorded steps and the captured graphs, which hold its pointer, stay valid: a schedule such as
        pipe.set_noise_scale(0.2 * s) between episodes keeps them, where a change of policy.act_noise drops them
        (_check_key).  Turning the array on or off does change the key.  The array is run state of the pipeline: checkpoints
        store policy.act_noise only."""
        if values is None:
            if self.noise_scale is not None:
                self.actor.set_noise_scale(None)
                self.noise_scale = None
            return
        from .agent import noise_scale_buffer
        buf = noise_scale_buffer(values, self.env.B, self.env.device, "TrainPipeline.set_noise_scale", out=self.noise_scale,
                                 stream=self.s_env)
        if self.noise_scale is None:
            self.actor.set_noise_scale(buf, self.cols // self.env.B)
            self.noise_scale = buf

    def _scalar_key(self):
        """the per-step scalars that a recorded step / a captured graph holds as frozen launch arguments (with a noise scale
        array set, a fixed marker in the place of act_noise: the launches hold the array's pointer, not its values)"""
        pol = self.policy
        return ("noise_scale" if self.noise_scale is not None else float(pol.act_noise), float(pol.act_limit), float(pol.behavior_actor.optimizer.eta),
                float(pol.behavior_critic.optimizer.eta), float(pol.y), float(pol.rho_effective), int(bool(pol.quirk)),
                pol.reward_group, bool(self.kick_env_after_critic), int(self.noise_seed)) + (
                    (self.env.y0.data_ptr(),) if self.per_traj else ())     # (the clock's launch holds the pointer of env.y0)

    def _check_key(self):
        """a noise / learning-rate schedule (or load_agent restoring act_noise) changed a frozen scalar: drop the recorded
        steps and the graphs -- the run continues eagerly with the new values until capture() is called again"""
        key = self._scalar_key()
        if key != self._key:
            self._progs = {}
            if self.graphs:
                for h in self.graphs.values():
                    self.lib.pdec_destroy(h)
                self.graphs = {}
            self._captured = False
            self._key = key

    def _interior(self, k, n):
        """steps k .. k+n-1 are neither the first nor the last of an episode (those run eagerly)"""
        if k - self.LAG < self._first_update:
            return False
        e, E = k - self.ep_start, self._E_host
        if E <= 0:
            return e >= 1
        e %= E
        return e >= 1 and e + n <= E - 1

    def _eager(self):
        """issue step `tick` call by call.  An interior step (not the first / last of an episode) at ring phase
        tick mod 6 makes exactly the library calls, with exactly the arguments, of every other interior step at that
        phase (the property the HIP graphs rest on), so the calls of the first such step are recorded and later ones
        replay the list -- ~20 raw C calls instead of the Python layers of PDEenv / policy / torch stream contexts"""
        k = self.tick
        fast = (self.fast_eager and not self.drain_between and not self._after_graph and k > 0
                and self._interior(k, 1) and self._interior(k - 1, 1))
        prog = self._progs.get(k % PERIOD) if fast else None
        if prog is not None:
            for f, a in prog:
                rc = f(*a)
                if rc:
                    _lib.check(rc)
        elif fast:
            calls = []
            self.lib.record_into(calls)
            try:
                self._issue(k)
            finally:
                self.lib.record_into(None)
            self._progs[k % PERIOD] = calls
        else:
            self._issue(k)
        self.tick += 1
        self.n_eager_steps += 1

    def _sync_streams_for_graph(self):
        """a graph runs wholly on the env stream: order the eager update still queued on the update stream before it"""
        if not self.serial and not self._after_graph and self.tick > 0:
            self.ev_upd[(self.tick - 1) % 2].wait(self.s_env)
            if self._telem is not None and self.stop_events:
                # the last telemetry launch behind an eager update is not covered by ev_upd where that event rode on the update's
                # own launch (a wait for an event never recorded, or recorded steps ago, is satisfied at once)
                self.ev_tel.wait(self.s_env)

    def _launch(self, h):
        _lib.check(self.lib.pdec_graph_launch(h, self._sp_env))
        if not self.serial:
            self.ev_graph.record(self.s_env)
        self._after_graph = True

    def run(self, n):
        """issue n control steps (asynchronous: returns when they are enqueued)"""
        n = int(n)
        if self._dtype_refusal:
            raise _lib.PdecError(self._dtype_refusal)
        self._check_key()
        while n > 0:
            k = self.tick
            done = False
            if self._captured:
                for c in self.chunks:
                    if c <= n and (c, k % PERIOD) in self.graphs and self._interior(k, c):
                        self._sync_streams_for_graph()
                        self._launch(self.graphs[(c, k % PERIOD)])
                        self.tick += c
                        n -= c
                        self.n_graph_launches += 1
                        done = True
                        break
            if not done:
                self._eager()
                n -= 1

    def step(self):
        self.run(1)

    # ------------------------------------------------------------------ episode ledger (host accessors: synchronise)
    def _need_ledger(self, best=False):
        if self.ledger is None:
            raise _lib.PdecError("TrainPipeline: the episode ledger is off (log_episodes=0)")
        if best and not self.track_best:
            raise _lib.PdecError("TrainPipeline: the best actor is not tracked with an active reducer")

    def _need_lockstep(self, what):
        if self.per_traj:
            raise _lib.PdecError(f"TrainPipeline.{what} belongs to lock-stepped episodes; with episodes='per_trajectory' every "
                                 "trajectory ends on its own: read finished_episodes()")

    def finished_episodes(self):
        """episodes="per_trajectory": every logged episode, as a dict of flat arrays sorted by (end_step, trajectory) --
        trajectory, episode (0-based, per trajectory), ret (float64: the ledger's arithmetic, sum over steps of the row mean),
        length (steps it took), blew_up (bool: ended by the blow-up flag), end_step (1-based number of the control step since
        construction that ended it) -- plus dropped: how many earlier episodes the per-trajectory rings of log_episodes
        slots have overwritten.  Synchronises the env stream."""
        if self.clock is None:
            raise _lib.PdecError("TrainPipeline.finished_episodes needs episodes='per_trajectory'")
        if self.log_episodes <= 0:
            raise _lib.PdecError("TrainPipeline: the episode log is off (log_episodes=0)")
        B, N = self.env.B, self.log_episodes
        cnt = np.empty(B, dtype=np.int64)
        ret, ln, blew, end = np.empty((B, N)), np.empty((B, N), dtype=np.int32), np.empty((B, N), dtype=np.int32), np.empty((B, N), dtype=np.int64)
        _lib.check(self.lib.pdec_epclock_read(self.clock.h, _lib.ptr(cnt), _lib.ptr(ret), _lib.ptr(ln), _lib.ptr(blew), _lib.ptr(end)))
        rows = [(int(end[b, e % N]), b, e) for b in range(B) for e in range(max(0, int(cnt[b]) - N), int(cnt[b]))]
        rows.sort()
        tb = np.array([r[1] for r in rows], dtype=np.int64)
        te = np.array([r[2] for r in rows], dtype=np.int64)
        sl = te % N
        return dict(trajectory=tb, episode=te, ret=ret[tb, sl], length=ln[tb, sl], blew_up=blew[tb, sl] != 0, end_step=end[tb, sl],
                    dropped=int(np.maximum(cnt - N, 0).sum()))

    @property
    def episodes_finished(self):
        """episodes="per_trajectory": episodes finished so far per trajectory, int64 [B] (synchronises the env stream)"""
        if self.clock is None:
            raise _lib.PdecError("TrainPipeline.episodes_finished needs episodes='per_trajectory'")
        cnt = np.empty(self.env.B, dtype=np.int64)
        _lib.check(self.lib.pdec_epclock_read(self.clock.h, _lib.ptr(cnt), None, None, None, None))
        return cnt

    def episode_returns(self):
        """(returns [n, B] float64, blew_up [n, B] bool, dropped): the last n = min(episodes, log_episodes) logged
        episodes, oldest first, and how many earlier ones the ring has overwritten"""
        self._need_lockstep("episode_returns()")
        self._need_ledger()
        N, B = self.log_episodes, self.env.B
        ret, blew = np.empty((N, B)), np.empty((N, B), dtype=np.int32)
        _lib.check(self.lib.pdec_ledger_read(self.ledger.h, _lib.ptr(ret), _lib.ptr(blew), None))
        n = min(self.n_episodes, N)
        rows = [e % N for e in range(self.n_episodes - n, self.n_episodes)]
        return ret[rows], blew[rows] != 0, self.n_episodes - n

    @property
    def rewards(self):
        """batch-mean return of each logged episode (PDEhook.rewards), the last min(episodes, log_episodes)"""
        self._need_lockstep("rewards")
        self._need_ledger()
        N = self.log_episodes
        means = np.empty(N)
        _lib.check(self.lib.pdec_ledger_read(self.ledger.h, None, None, _lib.ptr(means)))
        n = min(self.n_episodes, N)
        return [float(means[e % N]) for e in range(self.n_episodes - n, self.n_episodes)]

    def _need_eval(self):
        if self.eval_every <= 0:
            raise _lib.PdecError("TrainPipeline: evaluations are off (eval_every=0)")

    def _eval_rows(self):
        """(ring rows oldest first, dropped) of the last min(evaluations, eval_capacity) evaluations"""
        N = self.eval_capacity
        n = min(self.n_evals, N)
        return [e % N for e in range(self.n_evals - n, self.n_evals)], self.n_evals - n

    def eval_returns(self):
        """(episodes [n] int64, returns [n, K] float64, blew_up [n, K] bool, dropped): the last n = min(evaluations,
        eval_capacity) evaluations, oldest first -- the 1-based episode each one followed, its per-trajectory returns and
        blow-up bits -- and how many earlier ones the ring has overwritten"""
        self._need_eval()
        N, K = self.eval_capacity, self.eval_K
        eps, ret, blew = np.empty(N, dtype=np.int64), np.empty((N, K)), np.empty((N, K), dtype=np.int32)
        _lib.check(self.lib.pdec_ledger_eval_read(self.ledger.h, _lib.ptr(eps), _lib.ptr(ret), _lib.ptr(blew), None))
        rows, dropped = self._eval_rows()
        return eps[rows], ret[rows], blew[rows] != 0, dropped

    @property
    def eval_scores(self):
        """score of each kept evaluation (module docstring), oldest first; NaN: a trajectory stopped or is not finite"""
        self._need_eval()
        sc = np.empty(self.eval_capacity)
        _lib.check(self.lib.pdec_ledger_eval_read(self.ledger.h, None, None, None, _lib.ptr(sc)))
        return sc[self._eval_rows()[0]]

    def _best(self):
        v, e = C.c_double(), C.c_int64()
        if self.best_by == "eval":
            _lib.check(self.lib.pdec_ledger_eval_best(self.ledger.h, C.byref(v), C.byref(e)))
            return v.value, e.value
        self._need_ledger(best=True)
        _lib.check(self.lib.pdec_ledger_best(self.ledger.h, C.byref(v), C.byref(e)))
        return v.value, e.value

    @property
    def bestreward(self):
        """PDEhook.bestreward: -1e6 until an episode has been chosen (best_by="eval": the best evaluation score)"""
        return self._best()[0]

    @property
    def bestepisode(self):
        """PDEhook.bestepisode: 1-based number of the best episode (0: none yet)"""
        return self._best()[1]

    def best_actor(self):
        """the actor of the best episode as it acted in that episode's last step: a CustomNeuralNetworkApproximator
        shaped like the behaviour actor (PDEhook.bestNNA)"""
        from .nna import CustomNeuralNetworkApproximator, HipMLP
        if self.bestepisode == 0:
            raise _lib.PdecError("TrainPipeline.best_actor: no episode has been chosen yet")
        A = self.policy.behavior_actor
        m = A.model
        out = HipMLP(m.dims, m.acts, None, m.dtype, m.device, m.max_cols, m.stream)
        if self.best_by == "eval":
            _lib.check(self.lib.pdec_ledger_eval_best_params(self.ledger.h, out.handle))
        else:
            _lib.check(self.lib.pdec_ledger_best_params(self.ledger.h, out.handle))
        import copy
        return CustomNeuralNetworkApproximator(out, copy.copy(A.optimizer))

    # ------------------------------------------------------------------ telemetry (host accessors: synchronise)
    @staticmethod
    def _telemetry_rows(rows, calls, columns):
        """(name -> column of the last min(calls, N) rows of a ring of N, oldest first; how many earlier rows were overwritten)"""
        N = rows.shape[0]
        n = min(int(calls), N)
        order = [c % N for c in range(int(calls) - n, int(calls))]
        kept = rows[order]
        return {name: kept[:, i].copy() for i, name in enumerate(columns)}, int(calls) - n

    def telemetry(self):
        """the telemetry rings (TrainPipeline(telemetry=N)) as a dict: step and update -- name -> float64 array, the last
        min(calls, N) rows oldest first, columns TELEMETRY_STEP_COLUMNS / TELEMETRY_UPDATE_COLUMNS, counts as doubles; step also holds
        action_saturated_fraction = action_saturated / columns, divided here on the host --, dropped_steps / dropped_updates: rows
        the rings have overwritten, first_nonfinite_step / first_nonfinite_update: the `step` / `update` value of the first row
        with a non-finite reward or state entry / loss or parameter since construction or telemetry_reset(), None when there was
        none (sticky: later clean rows do not clear it).  Synchronises the env and the update stream."""
        if self._telem is None:
            raise _lib.PdecError("TrainPipeline.telemetry: telemetry is off (telemetry=0)")
        N = self.telemetry_capacity
        srows, urows = np.empty((N, len(TELEMETRY_STEP_COLUMNS))), np.empty((N, len(TELEMETRY_UPDATE_COLUMNS)))
        ns, nu, sent = C.c_int64(), C.c_int64(), np.empty(2, dtype=np.int64)
        _lib.check(self.lib.pdec_telemetry_read(self._telem.h, _lib.ptr(srows), C.byref(ns), _lib.ptr(urows), C.byref(nu),
                                                _lib.ptr(sent)))
        step, ds = self._telemetry_rows(srows, ns.value, TELEMETRY_STEP_COLUMNS)
        upd, du = self._telemetry_rows(urows, nu.value, TELEMETRY_UPDATE_COLUMNS)
        step["action_saturated_fraction"] = step["action_saturated"] / float(self.cols)
        return dict(step=step, update=upd, dropped_steps=ds, dropped_updates=du,
                    first_nonfinite_step=None if sent[0] < 0 else int(sent[0]),
                    first_nonfinite_update=None if sent[1] < 0 else int(sent[1]))

    def telemetry_reset(self):
        """clear the telemetry rings, their counters, the sentinel and theta_prev (synchronises the env and the update stream)"""
        if self._telem is None:
            raise _lib.PdecError("TrainPipeline.telemetry_reset: telemetry is off (telemetry=0)")
        _lib.check(self.lib.pdec_telemetry_reset(self._telem.h))

    def sync(self):
        self.s_env.synchronize()
        self.s_upd.synchronize()
        if self.s_ar is not None:
            self.s_ar.synchronize()
        if self.s_eval is not None:
            self.s_eval.synchronize()

    def close(self):
        if self.s_eval is not None:
            self.s_eval.synchronize()                  # an evaluation still running reads objects this pipeline owns
        if getattr(self, "simd_sharing", False):
            self.lib.pdec_env_set_simd_sharing(self.env.handle, 0, None)
            self.simd_sharing = False
        for h in self.graphs.values():
            self.lib.pdec_destroy(h)
        self.graphs = {}
        self._captured = False
