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

Frozen target networks, one rank, inside run(): the finish launch of the actor half of update_k (slab reduction, ADAM, image
refresh) is not a launch of its own -- the critic half of update_{k+1} reads nothing it writes, so its blocks ride in the
critic's finish launch of update_{k+1} (pdec_ddpg_defer_actor_finish):

    update stream:  wait act_{k-1} -> critic pass_k -> [critic finish_k + actor finish_{k-1}] -> actor pass_k
    env stream:                                         wait that launch -> act_k -> env_k

Three launches on the update chain instead of four and one cross-stream wait fewer; the same bits.  run() flushes the last
finish before it returns, so nothing is pending outside it (PDEC_DEFER_ACTOR_FINISH=0: the four-launch step).

Data-parallel runs (N > 1, policy-gradient-only exchange, frozen target networks): the all-reduce of the actor's gradient and
the ADAM launch that consumes it leave the update stream (`stream_ar`):

    update stream:  critic half_k -> [wait apply_{k-1}] actor pass_k -> slab reduction_k ---------> critic half_{k+1} -> ...
    side stream:                                                        wait reduction_k -> all-reduce_k -> ADAM(actor)_k

The critic half reads the TARGET actor only (a' = At(s'), src/PDEagent.jl:385), which never moves (quirk_frozen_targets), so
critic half_{k+1} does not depend on ADAM(actor)_k and hides the collective; the next readers of the updated actor -- act_{k+1} on
the env stream and actor pass_{k+1} -- wait for the event on the ADAM launch.  Same kernels, same arguments, same order of
arithmetic as the in-chain order: bit-identical (tests/test_gpu_pipeline.py, tests/test_aa_multirank_gpu.py).

Every buffer a step touches is a pure function of the step counter k (rings indexed by k mod 2 / 3 / 6: _slots) and every
per-step scalar lives on the device (noise counter: pdec_policy_act_rng_dev; ADAM beta powers), so the launch arguments
of step k + 6 are those of step k: chunks of 24 / 6 / 1 consecutive steps starting at each of the six ring phases are
captured ONCE into HIP graphs (pdec_capture_begin / _end) and replayed with one host call per chunk instead of ~12 ctypes
calls per step.  Inside a chunk the cross-stream events above become graph edges; a chunk forks the update branch off
the env stream at its first step and joins it at its last.  The first and the last step of an episode
(initial-condition pointers, time-out terminal flags; te / dt + 1 = 51 steps in scripts/KS/KS22) are issued eagerly.  Eager and replayed runs enqueue the same kernels with the same arguments and are
bit-identical (tests/test_gpu_agent.py).

The opt-in features each live in a module of their own, which owns their checks, buffers, launches and readers and whose docstring
states their mechanism; _issue names each of their calls at its place in the step:

    pipeline_episodes.py    the episode ledger (log_episodes), the episode-start draws (random_init), the per-trajectory episode
                            clock (episodes="per_trajectory")
    pipeline_eval.py        greedy held-out evaluation behind every eval_every-th episode (eval_every, best_by="eval")
    pipeline_nstep.py       n-step transitions assembled on the device (n_step)
    pipeline_telemetry.py   per-step training telemetry kept on the device (telemetry, telemetry_every)
    pipeline_replay.py      the device-replay route of the update (use_replay)"""
import copy
import ctypes as C
import os
from types import SimpleNamespace

import torch

from . import _lib
from .pipeline_episodes import check_episode_mode, setup_episodes
from .pipeline_eval import Evaluation, check_eval_args, eval_score  # noqa: F401  (eval_score: part of this module's surface)
from .pipeline_nstep import NStep, check_n_step, gamma_n
from .pipeline_replay import Replay
from .pipeline_telemetry import (TELEMETRY_STEP_COLUMNS, TELEMETRY_UPDATE_COLUMNS, Telemetry, check_telemetry,  # noqa: F401
                                 ring_columns)

PERIOD = 6            # lcm of the ring lengths (2: y / published actor / beta-power and noise-counter slots; 3; 6)


class _Event(_lib.Owned):
    """device-scope event of the library (pdec_event_create: no system-scope fence), torch.cuda.Event-like surface"""

    def __init__(self, lib):
        super().__init__(lib)
        _lib.check(lib.pdec_event_create(C.byref(self.h)))

    def record(self, stream):
        _lib.check(self.lib.pdec_event_record(self.h, C.c_void_p(stream.cuda_stream)))

    def wait(self, stream):
        _lib.check(self.lib.pdec_stream_wait_event(C.c_void_p(stream.cuda_stream), self.h))


class _TorchEvent:
    """the same surface on a default torch event (diagnostic: PDEC_TORCH_EVENTS=1)"""

    def __init__(self, lib=None):
        self.ev = torch.cuda.Event()

    def record(self, stream):
        self.ev.record(stream)

    def wait(self, stream):
        stream.wait_event(self.ev)


def _of(feature, name, off=None):
    """a one-line forward: the attribute `name` of the feature object self.<feature>, `off` while that feature is off"""
    return property(lambda self: getattr(getattr(self, feature), name, off))


_LEDGER_OFF, _EVAL_OFF = ("TrainPipeline: the episode ledger is off (log_episodes=0)",
                          "TrainPipeline: evaluations are off (eval_every=0)")


_NOISE_CORR_PER_TRAJ = ("TrainPipeline(noise_corr=...) belongs to lock-stepped episodes: with episodes='per_trajectory' a "
                        "restarted trajectory would have to zero its noise states inside the boundary launch")


class TrainPipeline:
    def __init__(self, env, agent, lag=2, episode_steps=51, stream_env=None, stream_upd=None, use_graphs=True,
                 chunks=(24, 6, 1), use_replay=False, noise_seed=1234, kick_env_after_critic=None, stream_ar=None,
                 ar_off_chain=None, log_episodes=0, min_best_episode=0, random_init=False, init_seed=0, init_rng=None,
                 init_rank=(0, 1), eval_every=0, eval_inits=8, eval_seed=0, eval_y0=None, eval_capacity=64, eval_stream=None,
                 best_by="train", noise_scale=None, episodes="lockstep", stagger=False, n_step=1,
                 telemetry=0, telemetry_every=1, noise_corr=None):
        """env: PDEenv on `stream_env`; agent: create_agent(..., stream=stream_upd).  lag: the update of step k trains on
        the transition of step k - lag (>= 1).  episode_steps: lock-stepped episodes of that many control steps (0: one
        endless episode): the last transition is terminal (done = time >= te, src/PDEenv.jl:227) and the next step starts
        from env.y0 (reset!, :183-193).  use_replay: route the update through the device-resident replay (pipeline_replay.py):
        every transition is pushed (src/PDEagent.jl:254-289) and the update trains on B * A transitions drawn from it
        (:317-340) instead of the B * A fresh ones (eager only).  stream_ar: a third stream for the gradient all-reduce + the
        actor's ADAM launch of a data-parallel run (module docstring); ar_off_chain: None = whenever that order is legal
        (split update, policy-gradient-only exchange, frozen targets, stream_ar given), False = keep the collective on the update
        stream, True = insist (raises when illegal).

        log_episodes = N > 0: the episode ledger (pipeline_episodes.py) keeps the last N episodes' per-trajectory returns and
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

        eval_every = N > 0: greedy held-out evaluation (pipeline_eval.py) behind the last step of every episode whose 1-based
        number is a multiple of N -- one episode of episode_steps control steps, learning = 0, the policy's act_limit, on an
        environment of its own (B = K, the training env's setup and dtype) from the fields eval_y0 [K, ...], or, None,
        eval_inits fields drawn once as population.evaluate_actors draws its own (pipeline_eval.held_out_fields: Philox stream
        (eval_seed, 0) of env.random_init; the fluid: setup.random_init_device(env, np.random.default_rng(eval_seed))).
        pipe.eval_y0: the fields; pipe.eval_zero_score: the score of the zero action on them (an actor with all parameters 0,
        run once here).  The last eval_capacity evaluations are kept: eval_returns(), eval_scores.  eval_stream: None = the env
        stream, or a stream that is neither the env nor the update stream (made by the same make_streams call) on which the
        evaluation runs beside training.  best_by: "train" -- best_actor() / bestreward / bestepisode follow the training
        return, as without evaluations -- or "eval": the hook's rule on the evaluation scores (episode >= min_best_episode,
        score not NaN and >= every earlier such score), keeping the evaluated parameters.  Needs log_episodes > 0 (the snapshot
        lives in the ledger), episode_steps > 0 and no active reducer.

        noise_scale = [B] (host array or device tensor): trajectory b explores at noise_scale[b] in the place of the policy's
        act_noise -- see set_noise_scale.  None: the policy's scalar.

        noise_corr = a scalar or [B] (host array or device tensor) in [0, 1): temporally correlated exploration noise, trajectory b's
        step-to-step correlation -- see set_noise_corr.  pipe.noise_state [B A na] holds the AR(1) states; it is zeroed on the env
        stream ahead of an episode's first acting launch (a first step is always issued eagerly, so the eager, the recorded and the
        captured forms all see it) and by reset_from().  Lock-stepped episodes only; n_step, telemetry, the ledger, evaluations
        (greedy: they touch nothing), noise_scale, use_replay and a reducer (each rank has its own states) are served.  It is run
        state of the pipeline: checkpoints do not store it.  noise_corr = None builds nothing and issues the launches it always
        did.

        An environment that holds fault arrays (PDEenv.set_faults, called before the pipeline is made) needs no argument here:
        the arrays are read by the kernels, so eager steps, recorded calls and captured graphs all step through them, writing
        new values into them between two run() calls keeps the recorded steps and the graphs, the reset image of the episode
        start is featurized through them and the per-trajectory episode clock re-featurizes a restarted trajectory through its
        own sensor faults.  The evaluation environment (eval_every) is this pipeline's own and stays healthy.  (The flag-synchronised
        single-trajectory step of run(..., device_episodes) has no fault-carrying form; run() orders such an environment's streams
        with events.)

        episodes = "per_trajectory": every trajectory keeps its own episode clock on the device (pipeline_episodes.py,
        csrc/episode_clock.hip).  One boundary call behind every env step ends the episode of trajectory b IN that
        step when its blow-up flag is raised or its clock reaches episode_steps: the row's transition is terminal, its return is
        logged, and the trajectory restarts from row b of env.y0 -- or, with random_init, from row b of env.random_init(init_seed,
        off) at off = (n W + r) B ceil(nc / 4), n the number of episodes b has finished: the field the lock-stepped pipeline draws
        for its episode n (the host-issued step 0 draws episode 0).  The other trajectories go on.  The host
        schedules as for episode_steps = 0 -- step 0 is the only first step, every later one is interior -- so capture() and
        the recorded calls cover every step and chunks need not fit an episode.  stagger=True starts the clock of trajectory
        b at floor(b E / B): the time-outs spread evenly over the E phases of an episode (the first episode of b is shorter by
        that much and is logged with the steps it really took).  log_episodes = C > 0 is then the log capacity PER TRAJECTORY
        (finished_episodes(), episodes_finished); episode_returns() / rewards belong to the lock-stepped mode.  reset_from()
        sets every clock back to its initial value and drops the running returns.  The 1-D environments with per-actuator
        agents and memory_size = 0 only; not with use_replay, an active reducer, evaluations or best-actor tracking (score
        actors with population.evaluate_actors between run() calls).

        n_step = n > 1 (1 .. 32): the update trains on n-step transitions assembled on the device (pipeline_nstep.py;
        csrc/nstep.hip).  Step k emits, per column, the transition that starts at step k - n + 1: its state and action, the
        discounted sum of the rewards up to its first terminal step (at most n of them), terminal = 1 where the window was cut by
        one; the next state is the one-step batch's.  update_k trains on the batch assembled at step k - lag
        with gamma_n (policy.y multiplied n times) in the place of policy.y, so the first update after a restart is n - 1 steps
        later than with n = 1.  pipe.n_step, pipe.gamma_n; pipe.nstep_batch(j): the batch assembled at step j.  Both episode
        modes, every environment, the ledger, evaluations, noise_scale and a reducer are served; use_replay=True is refused
        (the replay route pushes one-step rows).  n_step is run state of the pipeline: checkpoints do not store it.  n_step = 1
        builds nothing and issues the launches it always did.

        telemetry = N > 0: per-step training telemetry kept on the device (pipeline_telemetry.py; csrc/telemetry.hip), the last N
        rows of each of two rings.  One row per control step -- step, reward_mean / _min / _max over the finite rewards and
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
        check_n_step(n_step, use_replay)
        self.n_step = int(n_step)
        check_telemetry(telemetry, telemetry_every, agent.policy.reducer)
        self.telemetry_capacity, self.telemetry_every = int(telemetry), int(telemetry_every)
        # pdec_policy_act_rng_dev reads the state ring in the actor's type: a fluid environment of another dtype cannot step.
        # Refused by name at the first run() / capture(), not here: an object of that combination may be constructed and asked
        # for its episode-start draw (tests/test_gpu_pipeline_episodes.py::test_random_inits_fluid does).
        mixed = getattr(env, "is_fluid", False) and env.dtype != agent.policy.behavior_actor.model.dtype
        self._dtype_refusal = (f"TrainPipeline: the fluid environment ({env.dtype}) and the networks "
                               f"({agent.policy.behavior_actor.model.dtype}) must have one dtype: the acting kernel reads "
                               "the environment's state ring in the actor's type") if mixed else None
        check_episode_mode(env, agent, episodes, stagger, episode_steps, use_replay, eval_every, min_best_episode, best_by)
        self.per_traj, self.stagger = episodes == "per_trajectory", bool(stagger)
        if noise_corr is not None and self.per_traj:
            raise _lib.PdecError(_NOISE_CORR_PER_TRAJ)
        if getattr(agent.policy, "noise_corr", None) is not None:
            raise _lib.PdecError("TrainPipeline: a noise correlation is set on the policy (set_noise_corr); the pipeline zeroes the "
                                 "states it owns at its episode starts: unset it and pass noise_corr= here")
        self.env, self.agent, self.policy = env, agent, agent.policy
        self.s_env = stream_env if stream_env is not None else env.stream
        self.s_upd = stream_upd if stream_upd is not None else self.policy.behavior_critic.model.stream
        check_eval_args(env, agent, episode_steps, self.s_env, self.s_upd, log_episodes, eval_every, eval_inits, eval_y0,
                        eval_capacity, eval_stream, best_by)
        self.eval_every, self.best_by = int(eval_every), best_by
        self.lib, self.E, self.LAG = env.lib, int(episode_steps), max(1, int(lag))
        assert self.LAG in (1, 2), "rings hold the last 3 transitions: lag 1 or 2"
        if self.s_env is None or self.s_upd is None:
            raise _lib.PdecError("TrainPipeline needs explicit (non-default) streams for the environment and the networks")
        self.serial = self.s_env.cuda_stream == self.s_upd.cuda_stream
        self._sp_env, self._sp_upd = C.c_void_p(self.s_env.cuda_stream), C.c_void_p(self.s_upd.cuda_stream)
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
        self._place_collective(self._ar_legal if ar_off_chain is None else ar_off_chain)
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
        self.cols, self.ns, self.na = B * A, ns, setup.action_shape[0]
        dt, dev = env.dtype, env.device
        kw = dict(dtype=dt, device=dev)
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
        Ev = self._Ev = _TorchEvent if os.environ.get("PDEC_TORCH_EVENTS") == "1" else _Event
        self.ev_fork = Ev(self.lib)
        self.ev_act = [Ev(self.lib), Ev(self.lib)]                  # act_k issued (env stream)
        self.ev_upd = [Ev(self.lib), Ev(self.lib)]                  # update_k issued (update stream)
        self.ev_graph = Ev(self.lib)                                # tail of the last graph launch (env stream)
        self.ev_mid = Ev(self.lib)                                  # critic half of update_k done (update stream)
        self.ev_red = Ev(self.lib)                                  # actor gradient of update_k reduced (update stream) -> side stream
        self.ev_env = [Ev(self.lib), Ev(self.lib)]                  # env_k done (env stream; collective off the chain only)
        self._after_graph = False
        # tick: control steps issued so far (every buffer of step k is indexed by k mod 2 / 3 / 6); ep_start: tick of the first
        # step of the current episode
        self.tick = self.ep_start = 0
        self.noise_seed = int(noise_seed)
        self.actor = self.policy.behavior_actor.model
        yes = C.c_int()
        _lib.check(self.lib.pdec_mlp_acts_on_published_copy(self.actor.handle, C.byref(yes)))
        # an actor whose acting kernel reads its parameters in place (2-layer / generic nets) must not be rewritten by the
        # update's actor half while act_k still runs: that half then waits for act_k (the fused 3-layer path reads a
        # published copy instead and needs no such edge)
        self.act_in_place = not bool(yes.value)
        # start env_k behind the critic half of update_k instead of beside the critic pass (see _between_halves); for the
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
        # The same step over two waves per trajectory pair (csrc/ks_engines.hpp, FftWave256x2): 0.6 of the vector instructions
        # per wave, bit for bit the one-wave step.  Measured: the C2 step 1.9 % shorter, although the passes' own durations do
        # not show why.  PDEC_TWO_WAVE=0 keeps the one-wave kernel.
        self.two_wave = False
        if (not self.serial and self.rpart is not None and not self.simd_sharing
                and os.environ.get("PDEC_TWO_WAVE", "1") != "0"):
            eff = C.c_int()
            _lib.check(self.lib.pdec_env_set_two_wave_step(env.handle, 1, C.byref(eff)))
            self.two_wave = bool(eff.value)
        self.graphs = {}          # (chunk, pos) -> graph handle
        self._progs = {}          # (ring phase, armed) -> recorded library calls of an interior eager step (_eager)
        # the recorded-call replay re-issues LIBRARY calls only: with torch events (PDEC_TORCH_EVENTS=1) the cross-stream
        # records / waits are torch calls it would not see, so it is off for that event type
        # N > 1: the gradient all-reduce is one more recorded call (a library call with NativeGradReducer, a noted torch call
        # with GradReducer -- _Lib.note), so the multi-rank pipeline issues its steps the same fast way
        # (device replay: the batch is the trajectory's fixed fp32 sample buffers, handed through unchanged to fp32 nets)
        aliases = (self.policy.behavior_critic.model.dtype == torch.float32) if self.use_replay else self._batch_aliases
        self.fast_eager = os.environ.get("PDEC_FAST_EAGER", "1") == "1" and Ev is _Event and aliases
        self._key, self._captured = None, False       # _key: per-step scalars baked into _progs / the graphs (see _scalar_key)
        self.n_graph_launches = self.n_eager_steps = 0
        self.noise_scale = None   # set_noise_scale: float64 [B] on the device, read by every acting launch
        self.set_noise_scale(noise_scale)
        self.noise_ab = self.noise_state = None   # set_noise_corr: float64 [B, 2] and [B A na] on the device
        self.set_noise_corr(noise_corr)
        # the opt-in features: each object owns its buffers and launches, and is None -- nothing built, nothing issued -- when off
        self.nstep = NStep(self) if self.n_step > 1 else None
        self._telem = Telemetry(self) if self.telemetry_capacity > 0 else None
        self.replay = Replay(self) if self.use_replay else None
        self.ledger, self.inits, self.clock = setup_episodes(self, log_episodes, min_best_episode, random_init, init_seed, init_rng,
                                                             init_rank)
        self.evals = (Evaluation(self, eval_every, eval_inits, eval_seed, eval_y0, eval_capacity, eval_stream)
                      if self.eval_every > 0 else None)
        # Frozen targets: the actor's finish launch of update_k rides in the critic's finish launch of update_{k+1} (module
        # docstring; pdec_ddpg_defer_actor_finish) -- inside run(), in the eager two-stream step that kicks env_k behind the critic
        # half and carries its events on the launches, on fresh transitions, one rank, no telemetry (its update row reads the
        # actor behind the update).  PDEC_DEFER_ACTOR_FINISH=0: the four-launch sequence (A/B runs).
        self.defer_actor_finish = (self.stop_events and self.kick_env_after_critic and not self.serial and not self.act_in_place
                                   and not self.use_replay and not self.multi_rank and not self.ar_off_chain
                                   and self._telem is None and os.environ.get("PDEC_DEFER_ACTOR_FINISH", "1") != "0")
        self._armed = self._pending = False   # armed: inside run() with the library armed; pending: the last step left a finish
        self.reset_from(env.y0)
        self.inits.keep_y0 = False

    def _place_collective(self, off_chain):
        """the place of the gradient all-reduce (module docstring) and what follows from it"""
        self.ar_off_chain = bool(off_chain)
        self.s_ar = self._stream_ar if self.ar_off_chain else None
        self._sp_ar = C.c_void_p(self.s_ar.cuda_stream) if self.s_ar is not None else None
        # collective off the chain, two streams, LAG >= 2: both cross-stream waits of the update stream sit between the halves
        # of an update (_between_halves) instead of one there and one at the top of the step
        self._mid_waits = self.ar_off_chain and not self.serial and self.LAG >= 2 and not self.use_replay

    def set_ar_order(self, off_chain):
        """switch between the two places of the gradient all-reduce (module docstring) in a running pipeline: drains the
        streams, drops the recorded steps.  Both orders compute the same numbers; a caller times both and keeps the faster
        (bench.py: a collective of a few microseconds is cheaper left on the chain than two stream hops are)."""
        if off_chain and not self._ar_legal:
            raise _lib.PdecError("set_ar_order(True): not legal for this pipeline (see TrainPipeline(ar_off_chain=...))")
        self.sync()
        self._place_collective(off_chain)
        self._mid_wait_prev = False
        self._progs = {}

    # ------------------------------------------------------------------ state
    def reset_from(self, y0):
        """(re)start: the next step is the first of an episode from initial condition y0 ([B, ...] device tensor)"""
        env = self.env
        self.inits.keep_y0 = True     # (random_init: this episode starts from y0, the next ones draw again)
        if self.ledger is not None and self.tick > self.ep_start:
            self.ledger.discard()
        if self.clock is not None:
            self.clock.reset()
        with torch.cuda.stream(self.s_env):
            if self.noise_state is not None:
                self.noise_state.zero_()
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
            if self.replay is not None:
                self.replay.cut()

    def _slots(self, k):
        """the ring slots of step k: every buffer a step touches is a function of k mod 2 / 3 / 6, written here and nowhere else.
        cur / prev: the parity of k / k - 1, the index into the event pairs.  act_prev: the action in front of a_k -- with
        per-trajectory episodes the buffer the clock of step k - 1 wrote, and act_next the one the clock of step k writes.
        nb: the n-step batch assembled at step k."""
        i2, i3, clock = k % 2, k % 3, self.clock
        return SimpleNamespace(
            k=k, cur=i2, prev=1 - i2, y_in=self.ybuf[i2], y_out=self.ybuf[1 - i2], s_in=self.sring[k % PERIOD],
            s_out=self.sring[(k + 1) % PERIOD], act=self.aring[i3], rew=self.rring[i3], flags=self.fring[i3], term=self.tring[i3],
            rbar=self.rbar[i3], rpart=None if self.rpart is None else self.rpart[i3],
            act_prev=self.aring[(k - 1) % 3] if clock is None else clock.aprev[i2],
            act_next=None if clock is None else clock.aprev[1 - i2], nb=None if self.nstep is None else self.nstep.nbatch[i3])

    def _batch(self, r):
        """the transitions of the step whose ring slots are r as the update's batch: the one-step rows, or the n-step windows
        assembled at that step; the next state is sring[(k + 1) % 6] for both"""
        nxt = r.s_out.view(self.cols, self.ns)
        if r.nb is not None:
            return dict(r.nb, next_state=nxt)
        return dict(state=r.s_in.view(self.cols, self.ns), action=r.act.view(self.cols, self.na), reward=r.rew.view(self.cols),
                    terminal=r.term.view(self.cols), next_state=nxt)

    y = property(lambda self: self._slots(self.tick).y_in)        # the field / the observation the next step starts from
    state = property(lambda self: self._slots(self.tick).s_in)

    # ------------------------------------------------------------------ one step, issued call by call
    def _plan(self, k, chunk_first, chunk_last):
        """what step k is and touches, decided before anything is enqueued: its ring slots (_slots) and
        first / last: of an episode; capturing: inside a chunk being captured; evaluate: a greedy evaluation follows this step --
        the last step (eager) of an episode whose 1-based number is a multiple of eval_every;
        j, src, batch: update_k trains on the transition of step j = k - LAG, whose slots are src (batch None: no update; the
        replay route draws its batch behind act_k, _issue, and `updating` says beforehand whether it will get one);
        late_env: one stream + the collective off the chain: act_k needs ADAM(actor)_{k-1}, which waits for the all-reduce on
        the side stream -- so the critic half of update_k, which needs neither, goes first and hides it (two streams: the critic
        half is on the other stream anyway);
        kick: env_k starts behind the critic half of update_k (_between_halves; inside a captured chunk the extra fork / join
        edge of the kick costs more than it gives: 202 vs 148 us per step);
        use_stop: eager steps on the fused 3-layer path: the two events the env stream waits for ride on the reduction launches'
        own dispatch packets (pdec_mlp_set_stop_event) instead of being recorded as packets behind them."""
        st, fresh = self._slots(k), self.replay is None
        st.first, st.last = self._first_last(k)
        st.capturing, st.j = chunk_first or chunk_last or self._capturing, k - self.LAG
        st.evaluate = st.last and self.evals is not None and self.evals.due()
        if st.first:
            st.act_prev = self.azero                   # reset!(env): the action in front of a fresh episode
        st.sample = st.j >= self._first_update and not fresh
        st.updating = st.j >= self._first_update and (fresh or self.replay.ready())
        st.src = self._slots(st.j) if st.updating else None
        st.batch = self._batch(st.src) if st.updating and fresh else None
        st.late_env = self.serial and self.ar_off_chain and st.updating and fresh
        st.kick = self.kick_env_after_critic and st.updating and not self.serial and not st.capturing
        st.use_stop = self.stop_events and st.updating and not st.capturing and not self.serial
        st.defer = self._armed and st.kick and st.use_stop and fresh
        return st

    # ------------------------------------------------------------------ the deferred actor finish (frozen targets)
    def _arm_deferral(self, on):
        """run() entry / exit: arm the library (declined with moving targets: the steps are then the four-launch ones), or
        disarm it behind a flush -- outside run() nothing is pending, and every host reader sees what it always saw"""
        if not self.defer_actor_finish:
            return
        if not on:
            self._flush_actor_finish()
        armed = C.c_int()
        _lib.check(self.lib.pdec_ddpg_defer_actor_finish(self.actor.handle, int(on), float(self.policy.rho_effective),
                                                         C.byref(armed)))
        self._armed = bool(armed.value)

    def _flush_actor_finish(self):
        """the pending finish of update_{tick-1} as a launch of its own carrying ev_upd, what that update's last launch always
        carried (recorded behind the update where the library had nothing pending)"""
        if self._pending:
            h = self.actor.handle
            _lib.check(self.lib.pdec_mlp_set_stop_event(h, self.ev_upd[(self.tick - 1) % 2].h))
            _lib.check(self.lib.pdec_ddpg_flush_actor_finish(h))
            _lib.check(self.lib.pdec_mlp_flush_stop_event(h))
            self._pending = False

    def _issue(self, k, chunk_first=False, chunk_last=False):
        """enqueue control step k.  chunk_first / chunk_last: first / last step of a chunk being CAPTURED (fork / join of
        the update branch); both False for a step issued eagerly."""
        pol, lib, L = self.policy, self.lib, _lib
        st = self._plan(k, chunk_first, chunk_last)
        # 1. the waits at the top of the step
        mid_wait_prev, self._mid_wait_prev = self._mid_wait_prev, False
        if self._pending and not st.defer:        # a step of the four-launch sequence behind a deferred one
            self._flush_actor_finish()
        if not self.serial:
            if chunk_first:                       # fork: everything before this chunk is ordered before it on the env stream
                self.ev_fork.record(self.s_env)
                self.ev_fork.wait(self.s_upd)
            elif st.capturing:
                self.ev_act[st.prev].wait(self.s_upd)
                self.ev_upd[st.prev].wait(self.s_env)
            else:                                 # eager
                if self._after_graph:             # the update branch of the graph just launched ran on the env stream
                    self.ev_graph.wait(self.s_upd)
                    self._after_graph = False
                elif k > 0:
                    # (collective off the chain: update_{k-1} waited for env_{k-2} between its halves, see _between_halves)
                    if not mid_wait_prev:
                        self.ev_act[st.prev].wait(self.s_upd)
                    # (deferred: everything step k puts on the env stream waits for ev_mid of update_k, which the update
                    # stream reaches behind update_{k-1} -- whose actor finish, if pending, is part of that very launch)
                    if not st.defer:
                        self.ev_upd[st.prev].wait(self.s_env)
        # 2. act_k and env_k, unless they go between the halves of update_k (late_env: both; kick: env_k; deferred: both)
        if not st.late_env and not st.defer:
            self._act(st)
        if st.sample:
            # the replay route: a host function with step-dependent ring positions, re-evaluated, not replayed verbatim (_Lib.note)
            with torch.cuda.stream(self.s_upd):
                lib.note(self.replay.sample, self.replay.ev_push[st.prev] if (not self.serial and k > 0) else None)
            st.batch = self.replay.batch_cur
        if not st.kick and not st.late_env:
            self._env(st)
        # 3. the events the env stream waits for, armed on the reduction launches
        if st.use_stop:
            if st.kick:
                L.check(lib.pdec_mlp_set_stop_event(pol.behavior_critic.model.handle, self.ev_mid.h))
            if not st.defer:        # (deferred: ev_upd is carried by the flush, if this finish is ever one: _flush_actor_finish)
                L.check(lib.pdec_mlp_set_stop_event(pol.behavior_actor.model.handle, self.ev_upd[st.cur].h))
        with torch.cuda.stream(self.s_upd):
            # 4. update_k
            if st.batch is not None:
                if st.src.rpart is not None:
                    L.check(lib.pdec_ddpg_set_reward_partials(pol.behavior_critic.model.handle, L.ptr(st.src.rpart), self.n_rpart))
                elif self.pre_rbar:
                    L.check(lib.pdec_ddpg_set_reward_mean(pol.behavior_critic.model.handle, L.ptr(st.src.rbar)))
                if self.ar_off_chain:
                    self._update_ar_off_chain(st)
                elif st.kick or (self.act_in_place and not self.serial):
                    pol.update(st.batch, before_actor_half=lambda: self._between_halves(st), interleave=self.reward_interleave,
                               gamma=self._gamma_arg)
                else:
                    pol.update(st.batch, interleave=self.reward_interleave, gamma=self._gamma_arg)
                if self._telem is not None:
                    self._telem.update(st)
            # 5. its completion event
            if self.ar_off_chain and st.batch is not None:
                pass                                    # (the completion event was recorded on the side stream)
            elif st.defer:
                self._pending = True                    # (its last launch is yet to come)
            elif st.use_stop:
                L.check(lib.pdec_mlp_flush_stop_event(pol.behavior_actor.model.handle))          # no-op when consumed
            elif not self.serial:
                self.ev_upd[st.cur].record(self.s_upd)
        # 6. join: the graph ends on the env stream
        if chunk_last and not self.serial:
            self.ev_upd[st.cur].wait(self.s_env)

    def _act(self, st):
        """act_k on the env stream: actor forward on all B*A columns + exploration noise (Philox, counter on the device) + clamp,
        one launch; in front of it the reset of an episode's first step, behind it the snapshot of its last"""
        env, pol, lib, L = self.env, self.policy, self.lib, _lib
        if self.serial and self.ar_off_chain and st.k > 0:
            self.ev_upd[st.prev].wait(self.s_env)          # ADAM(actor)_{k-1} ran on the side stream
        with torch.cuda.stream(self.s_env):
            if st.first:                                   # reset!(env): this step starts from the initial condition
                if self.inits.random_init and not self.inits.keep_y0:      # (a field given to reset_from() is used as it is)
                    self.inits.draw()
                self.inits.keep_y0 = False
                st.y_in.copy_(env.y0)
                st.s_in.copy_(self.state0)
                if self.noise_state is not None:           # the AR(1) states of set_noise_corr start an episode at zero
                    self.noise_state.zero_()
            L.check(lib.pdec_set_stream(self.actor.handle, self._sp_env))
            L.check(lib.pdec_policy_act_rng_dev(self.actor.handle, L.ptr(st.s_in), self.cols, float(pol.act_noise),
                                                float(pol.act_limit), 1, self.noise_seed, L.ptr(st.act)))
            L.check(lib.pdec_set_stream(self.actor.handle, self._sp_upd))
            if st.last and self.track_best:
                self.ledger.snapshot()
                if st.evaluate:
                    self.evals.load()
            if not self.serial and self.LAG >= 2:
                self.ev_act[st.cur].record(self.s_env)
        if self.drain_between:
            torch.cuda.synchronize()

    def _env(self, st):
        """env_k on the env stream: the fused env step and, behind it, what the features put there, in this order"""
        env, lib, L = self.env, self.lib, _lib
        with torch.cuda.stream(self.s_env):
            L.check(lib.pdec_env_set_terminal_out(env.handle, L.ptr(st.term)))
            if st.rpart is not None:
                L.check(lib.pdec_env_set_reward_partials_out(env.handle, L.ptr(st.rpart), None))
            L.check(lib.pdec_env_step(env.handle, L.ptr(st.y_in), L.ptr(st.act), L.ptr(st.act_prev), L.ptr(st.s_in), L.ptr(st.y_out),
                                      L.ptr(self.pbuf), L.ptr(st.s_out), L.ptr(st.rew), L.ptr(st.flags)))
            if self.clock is not None:
                self.clock.step(st)
            if self.ledger is not None:
                self.ledger.step(st)
            if st.last:
                st.term.fill_(1.0)                     # time-out: done = time >= te -> terminal transition
                if self.ledger is not None:
                    self.ledger.close()
            rew_batch = st.rew if self.nstep is None else self.nstep.step(st)
            if self._telem is not None:
                self._telem.step(st)
            if self.pre_rbar and self.rpart is None:
                L.check(lib.pdec_reward_mean(env.handle, L.ptr(rew_batch), self.cols, L.ptr(st.rbar)))
            if self.replay is not None:
                # a host function with step-dependent ring positions: re-evaluated, not replayed verbatim (_Lib.note)
                lib.note(self.replay.push, self.replay.ev_push[st.cur], st.s_in, st.act, st.rew, st.term, st.s_out, st.first, st.last)
            if not self.serial and self.LAG < 2:
                # LAG = 1: update_{k+1} trains on the transition env_k is producing, so the event it waits on is
                # recorded behind the whole env branch, not behind the acting kernel
                self.ev_act[st.cur].record(self.s_env)
            if self._mid_waits:
                self.ev_env[st.cur].record(self.s_env)
        if st.evaluate:
            self.evals.run()                           # (behind everything step k puts on the env stream)
        if self.drain_between:                         # kernel-timing pass: nothing of the env branch overlaps the update
            torch.cuda.synchronize()

    def _between_halves(self, st):
        """on the update stream between the critic half and the actor half of update_k"""
        pol, lib, L = self.policy, self.lib, _lib
        if st.late_env:
            self._act(st)
            self._env(st)
        # Beside the critic pass the PDE step makes almost no progress and then collides with the whole actor pass;
        # released when the critic half (pass + reduction) is done it runs beside the actor pass, the second
        # reduction and the head of the next critic pass instead (r02i, same box: 152 -> 130 us per control step)
        if st.kick:
            if st.use_stop:
                L.check(lib.pdec_mlp_flush_stop_event(pol.behavior_critic.model.handle))     # no-op when consumed
            else:
                self.ev_mid.record(self.s_upd)
            self.ev_mid.wait(self.s_env)
            if st.defer:
                # act_k reads the actor of update_{k-1}, whose finish was part of the launch ev_mid rode on (or a launch in
                # front of the critic pass); the host has issued that launch, so the published copy is the new one
                self._act(st)
            self._env(st)
        if self.act_in_place and not self.serial:
            self.ev_act[st.cur].wait(self.s_upd)
        if self.ar_off_chain and st.k > 0:
            # the actor pass reads the actor that ADAM(actor)_{k-1} on the side stream has written (done long ago: it ran
            # beside the critic half that has just ended) ...
            self.ev_upd[st.prev].wait(self.s_upd)
            if self._mid_waits:
                # ... and the wait for the batch of update_{k+1} -- env_{k-1}, done since the middle of this critic pass --
                # sits here too, instead of at the top of step k + 1.  Why: every cross-stream wait is a barrier packet of
                # 5 - 7 us on the update chain even when it is satisfied (measured: the step with either wait removed),
                # two adjacent ones cost less than two apart (116.5 - 117.7 against 118 - 119 us per step), a single
                # wait on act_k's event (which implies both) or on a join event made on the side stream stalls on events
                # that complete just before they are needed (123 / 125 us) -- HISTORY.md 6.1
                self.ev_env[st.prev].wait(self.s_upd)
                self._mid_wait_prev = True

    def _update_ar_off_chain(self, st):
        """update_k of a data-parallel run with the collective off the update chain (module docstring).  On the update stream:
        critic half, actor pass, slab reduction (its completion = `ev_red`, riding on the reduction launch where the fused path
        allows); on the side stream behind that event: all-reduce of the flat actor gradient, then the ADAM launch -- issued
        through the actor's handles while they are set to the side stream -- whose completion is `ev_upd[k % 2]`, the event the
        next acting kernel (env stream) and the next actor pass (update stream) wait for."""
        pol, lib, L = self.policy, self.lib, _lib
        A, At = pol.behavior_actor.model, pol.target_actor.model
        pol.update_critic_half(st.batch, self.reward_interleave, self._gamma_arg)
        self._between_halves(st)
        red_on_launch = st.use_stop and lib.pdec_mlp_set_reduce_event(A.handle, self.ev_red.h) == 0
        pol.actor_grads(st.batch)                                   # (records a reduce event its launches did not carry)
        if not red_on_launch:
            self.ev_red.record(self.s_upd)
        self.ev_red.wait(self.s_ar)
        pol.reducer.all_reduce(A, stream=self.s_ar)
        L.check(lib.pdec_set_stream(A.handle, self._sp_ar))
        L.check(lib.pdec_set_stream(At.handle, self._sp_ar))
        try:
            pol.apply_actor()
            if st.use_stop:
                L.check(lib.pdec_mlp_flush_stop_event(A.handle))    # no-op when the ADAM launch carried ev_upd[k % 2]
            else:
                self.ev_upd[st.cur].record(self.s_ar)
        finally:
            L.check(lib.pdec_set_stream(A.handle, self._sp_upd))
            L.check(lib.pdec_set_stream(At.handle, self._sp_upd))

    # class-level values of an object that is not (yet) initialised, and of the features that are off
    _capturing = False
    _first_tick = 0
    _mid_wait_prev = False    # update_{k-1} waited for env_{k-2} between its halves (so step k needs no wait at its top)
    drain_between = False
    per_traj = False          # episodes="per_trajectory"
    n_step = 1
    telemetry_capacity, telemetry_every = 0, 1
    ledger = inits = clock = nstep = _telem = replay = evals = None

    # what lives in a feature object and is read through the pipeline
    n_episodes, track_best = _of("ledger", "n_episodes", 0), _of("ledger", "track_best", False)
    random_init, init_seed, init_rng, init_rank = (_of("inits", n) for n in ("random_init", "init_seed", "init_rng", "init_rank"))
    # init_offsets: Philox offset of every initial field drawn (KS / Keller-Segel); _draw_init(): one episode-start draw
    init_offsets, _draw_init = _of("inits", "init_offsets"), _of("inits", "draw")
    clock0, aprev = _of("clock", "clock0"), _of("clock", "aprev")
    nbatch = _of("nstep", "nbatch")
    n_evals, s_eval = _of("evals", "n_evals", 0), _of("evals", "s_eval")
    eval_y0, eval_zero_score, eval_env, eval_actor = (_of("evals", n) for n in ("eval_y0", "eval_zero_score", "eval_env", "eval_actor"))
    # the names the host tests reach the features' checks and read-outs by
    _check_n_step, _check_telemetry, _telemetry_rows = (staticmethod(f) for f in (check_n_step, check_telemetry, ring_columns))

    def _on(self, feature, off):
        """the feature object self.<feature>, or the refusal `off` that names what is switched off"""
        f = getattr(self, feature)
        if f is None:
            raise _lib.PdecError(off)
        return f

    @property
    def _first_update(self):
        """the first transition after the last restart that an update may train on: the n-step window that ends at step j starts
        at j - n + 1, which must not precede the restart"""
        return self._first_tick + self.n_step - 1

    @property
    def gamma_n(self):
        """policy.y multiplied n_step times: the discount of a full n-step window's bootstrap term (pipeline_nstep.gamma_n)"""
        return gamma_n(self.policy.y, self.n_step)

    @property
    def _gamma_arg(self):
        return None if self.n_step == 1 else self.gamma_n

    def nstep_batch(self, j):
        """(state [cols, ns], action [cols, na], reward [cols], terminal [cols], next_state [cols, ns]) of the batch assembled at
        step j -- the transitions that start at step j - n_step + 1 -- as the device holds them (the ring of three: valid until
        step j + 3 is issued; the caller synchronises).  For tests and probes."""
        self._on("nstep", "TrainPipeline.nstep_batch: n_step = 1 assembles nothing (the update reads the ring slots)")
        return tuple(self._batch(self._slots(j)).values())

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
        # (every eager step of this method is one of run()'s -- one kind of recorded step per pipeline --, and a captured step is
        # a four-launch one: the library is armed around the eager steps and disarmed while a chunk records)
        self._arm_deferral(True)
        try:
            while self.tick - self.LAG < self._first_update + 2:  # lazily created buffers / first-use uploads happen eagerly
                self._eager()
        finally:
            self._arm_deferral(False)
        self._key = self._scalar_key()
        for c in self.chunks:
            for pos in range(PERIOD):
                if not self._reachable(c, pos):
                    # e.g. chunk 24 with 26-step episodes: the interior offsets 1 .. E-1-c never meet this ring phase
                    # (the search below would issue eager steps for ever); run() falls back to a smaller chunk
                    continue
                self._arm_deferral(True)
                try:
                    while not (self.tick % PERIOD == pos and self._interior(self.tick, c)):
                        self._eager()
                finally:
                    self._arm_deferral(False)
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

    def set_noise_corr(self, values):
        """Temporally correlated exploration noise (CustomDDPGPolicy.set_noise_corr, pdec_mlp_set_noise_color): `values` the
        step-to-step correlation in [0, 1), a scalar or [B] as a host array (checked) or a [B] device tensor (copied device to
        device, b = sqrt(1 - a^2) taken on the device, no host wait), or None for white noise.  They are written on the env stream
        INTO the [B, 2] buffer the pipeline owns (self.noise_ab), whose pointer the acting launches hold beside that of
        self.noise_state: a schedule between episodes keeps the recorded steps and the captured graphs; turning it on or off
        changes the key (_check_key).  Setting it does not touch the states: they are zeroed at the next episode's first step."""
        if values is None:
            if self.noise_state is not None:
                self.actor.set_noise_color(None)
                self.noise_ab = self.noise_state = None
            return
        if self.per_traj:
            raise _lib.PdecError(_NOISE_CORR_PER_TRAJ)
        B, dev = self.env.B, self.env.device
        if isinstance(values, torch.Tensor) and values.is_cuda:
            if values.dim() != 1 or int(values.shape[0]) != B:
                raise ValueError(f"TrainPipeline.set_noise_corr: expected {B} correlations in a 1-D array, got shape {tuple(values.shape)}")
            src = None
        else:
            from .agent import noise_corr_ab
            src = torch.from_numpy(noise_corr_ab(values, B, "TrainPipeline.set_noise_corr"))
        with torch.cuda.stream(self.s_env):
            ab = self.noise_ab if self.noise_ab is not None else torch.empty((B, 2), dtype=torch.float64, device=dev)
            if src is not None:
                ab.copy_(src)
            else:
                a = values.to(torch.float64)
                ab[:, 0].copy_(a)
                ab[:, 1].copy_(torch.sqrt(1.0 - a * a))
            if self.noise_state is None:
                self.noise_state = torch.zeros(self.cols * self.na, dtype=torch.float64, device=dev)
        if self.noise_ab is None:
            self.noise_ab = ab
            self.actor.set_noise_color(self.noise_state, ab, self.cols // B)

    def _scalar_key(self):
        """the per-step scalars that a recorded step / a captured graph holds as frozen launch arguments (with a noise scale
        array set, a fixed marker in the place of act_noise: the launches hold the array's pointer, not its values)"""
        pol = self.policy
        return ("noise_scale" if self.noise_scale is not None else float(pol.act_noise), float(pol.act_limit), float(pol.behavior_actor.optimizer.eta),
                float(pol.behavior_critic.optimizer.eta), float(pol.y), float(pol.rho_effective), int(bool(pol.quirk)),
                pol.reward_group, bool(self.kick_env_after_critic), int(self.noise_seed)) + (
                    ("noise_corr",) if self.noise_state is not None else ()) + (
                    (self.env.y0.data_ptr(),) if self.per_traj else ())     # (the clock's launch holds the pointer of env.y0)

    def _drop_graphs(self):
        for h in self.graphs.values():
            self.lib.pdec_destroy(h)
        self.graphs = {}
        self._captured = False

    def _check_key(self):
        """a noise / learning-rate schedule (or load_agent restoring act_noise) changed a frozen scalar: drop the recorded
        steps and the graphs -- the run continues eagerly with the new values until capture() is called again"""
        key = self._scalar_key()
        if key != self._key:
            self._progs = {}
            self._drop_graphs()
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
        # armed (run() with the actor's finish deferred): an interior step is a deferred one, another list of calls than the
        # four-launch step's; the lists are those of steps that FOUND a finish pending -- not of the first step of a run() or
        # of the step behind a flush, whose top differs
        fast = fast and (self._pending or not self._armed)
        key = (k % PERIOD, self._armed)
        prog = self._progs.get(key) if fast else None
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
            self._progs[key] = calls
        else:
            self._issue(k)
        self.tick += 1
        self.n_eager_steps += 1

    def _sync_streams_for_graph(self):
        """a graph runs wholly on the env stream: order the eager update still queued on the update stream before it"""
        self._flush_actor_finish()            # (a graph's steps are the four-launch ones; the flush carries ev_upd)
        if not self.serial and not self._after_graph and self.tick > 0:
            self.ev_upd[(self.tick - 1) % 2].wait(self.s_env)
            if self._telem is not None and self.stop_events:
                self._telem.wait_before_graph()

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
        self._arm_deferral(True)
        try:
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
        finally:
            self._arm_deferral(False)

    def step(self):
        self.run(1)

    # ------------------------------------------------------------------ the features' host readers (they synchronise)
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
        return self._on("clock", "TrainPipeline.finished_episodes needs episodes='per_trajectory'").finished_episodes()

    @property
    def episodes_finished(self):
        """episodes="per_trajectory": episodes finished so far per trajectory, int64 [B] (synchronises the env stream)"""
        return self._on("clock", "TrainPipeline.episodes_finished needs episodes='per_trajectory'").finished()

    def episode_returns(self):
        """(returns [n, B] float64, blew_up [n, B] bool, dropped): the last n = min(episodes, log_episodes) logged
        episodes, oldest first, and how many earlier ones the ring has overwritten"""
        self._need_lockstep("episode_returns()")
        return self._on("ledger", _LEDGER_OFF).returns()

    @property
    def rewards(self):
        """batch-mean return of each logged episode (PDEhook.rewards), the last min(episodes, log_episodes)"""
        self._need_lockstep("rewards")
        return self._on("ledger", _LEDGER_OFF).means()

    def eval_returns(self):
        """(episodes [n] int64, returns [n, K] float64, blew_up [n, K] bool, dropped): the last n = min(evaluations,
        eval_capacity) evaluations, oldest first -- the 1-based episode each one followed, its per-trajectory returns and
        blow-up bits -- and how many earlier ones the ring has overwritten"""
        return self._on("evals", _EVAL_OFF).returns()

    @property
    def eval_scores(self):
        """score of each kept evaluation (pipeline_eval.py), oldest first; NaN: a trajectory stopped or is not finite"""
        return self._on("evals", _EVAL_OFF).scores()

    def _best_by(self):
        """who chooses the best actor: the evaluations (best_by="eval") or the ledger"""
        return self.evals if self.best_by == "eval" else self._on("ledger", _LEDGER_OFF)

    @property
    def bestreward(self):
        """PDEhook.bestreward: -1e6 until an episode has been chosen (best_by="eval": the best evaluation score)"""
        return self._best_by().best()[0]

    @property
    def bestepisode(self):
        """PDEhook.bestepisode: 1-based number of the best episode (0: none yet)"""
        return self._best_by().best()[1]

    def best_actor(self):
        """the actor of the best episode as it acted in that episode's last step: a CustomNeuralNetworkApproximator
        shaped like the behaviour actor (PDEhook.bestNNA)"""
        from .nna import CustomNeuralNetworkApproximator, HipMLP
        if self.bestepisode == 0:
            raise _lib.PdecError("TrainPipeline.best_actor: no episode has been chosen yet")
        A = self.policy.behavior_actor
        m = A.model
        out = HipMLP(m.dims, m.acts, None, m.dtype, m.device, m.max_cols, m.stream)
        self._best_by().best_params(out)
        return CustomNeuralNetworkApproximator(out, copy.copy(A.optimizer))

    def telemetry(self):
        """the telemetry rings (TrainPipeline(telemetry=N)) as a dict: step and update -- name -> float64 array, the last
        min(calls, N) rows oldest first, columns TELEMETRY_STEP_COLUMNS / TELEMETRY_UPDATE_COLUMNS, counts as doubles; step also holds
        action_saturated_fraction = action_saturated / columns, divided here on the host --, dropped_steps / dropped_updates: rows
        the rings have overwritten, first_nonfinite_step / first_nonfinite_update: the `step` / `update` value of the first row
        with a non-finite reward or state entry / loss or parameter since construction or telemetry_reset(), None when there was
        none (sticky: later clean rows do not clear it).  Synchronises the env and the update stream."""
        return self._on("_telem", "TrainPipeline.telemetry: telemetry is off (telemetry=0)").read()

    def telemetry_reset(self):
        """clear the telemetry rings, their counters, the sentinel and theta_prev (synchronises the env and the update stream)"""
        self._on("_telem", "TrainPipeline.telemetry_reset: telemetry is off (telemetry=0)").reset()

    def sync(self):
        self._flush_actor_finish()
        for s in (self.s_env, self.s_upd, self.s_ar, self.s_eval):
            if s is not None:
                s.synchronize()

    def close(self):
        if self.s_eval is not None:
            self.s_eval.synchronize()                  # an evaluation still running reads objects this pipeline owns
        if getattr(self, "simd_sharing", False):
            self.lib.pdec_env_set_simd_sharing(self.env.handle, 0, None)
            self.simd_sharing = False
        if getattr(self, "two_wave", False):
            self.lib.pdec_env_set_two_wave_step(self.env.handle, 0, None)
            self.two_wave = False
        self._drop_graphs()
