"""Populations: M independently seeded reference-shaped learners trained side by side on one GPU.

Every member is an ordinary `Agent` (create_agent(setup=..., B=1, stream=s_upd)) with its own `PDEhook`; `Population.run`
leaves each of them bit for bit where `run(agent_m, PDEenv(setup, B=1, ...), stops[m], hook_m)` leaves it.  The control steps
of an episode are issued as in run._run_device_episodes, but each of the three per-step launches is ONE launch of M workgroups,
workgroup m working from member m's pointers and from row m of a device counter table.

Members may differ in their hyper-parameters (gamma, Polyak rho, the two learning rates, act_noise, act_limit): the agents' own
attributes are read into the row table of every episode, so a sweep is M agents created with different values, and a change
between two `run` calls takes effect as it does in a solo run.  `Population.clone` copies a member's learner into others in one
launch, and `Population.exploit` applies it to an evaluation's ranking (population-based selection: the worst members take
over the best members' learners and go on with perturbed hyper-parameters).

This module holds the class; each mechanism lives in a module of its own, whose docstring states it:

    population_slots.py      the counter table and the book: slot names, and the functions that write a member's rows
    population_episodes.py   the episode machinery: the step loop, the episode opening, the host-settled episode
    population_blocks.py     blocks of episodes per read-back (run(stops, episodes_per_sync > 1)), the fluid's vortex tables
    population_eval.py       evaluate_actors: every member scored on the same held-out fields, on three routes
    population_select.py     the exploit plan and its perturbation"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .agent import Agent, PRE_EXPERIMENT_STAGE, POST_EPISODE_STAGE, POST_EXPERIMENT_STAGE
from .env import PDEenv, _on_stream
from .hook import PDEhook
from .population_blocks import (block_length, draw_block_tables, episode_log_bytes, episodes_still_needed,  # noqa: F401
                                own_error_detection, python_max_state, restore_block_rngs, run_block)
from .population_episodes import run_episode
from .population_eval import (ACT_MEMBERS_LDS, FAULT_KEYS, _handle_int, _has_batched_rollout, _has_persistent_rollout,  # noqa: F401
                              act_members_tiles, evaluate_actors, fault_arrays, member_workgroups, score_members)
from .population_select import PERTURBED, perturb_factors, plan_exploit
from .population_slots import (ROW, USTEP, NSA, NRT, NOISE, SAMPLE, HALT, ACTIVE, BPA, BPC, NOISE_AMP, LIMIT,  # noqa: F401
                               GAMMA, RHO, ETA_A, ETA_C, BOOK, BK_EP, BK_MIN_BEST, BK_COLLECT_NNA, BK_CMP_HAS, BK_CMP, BK_BESTREWARD,
                               BK_BESTEPISODE, BK_STOP_KIND, BK_STOP_CUR, BK_STOP_LIMIT, BK_RANDOM_INIT, BK_INIT_SEED, BK_INIT_OFF,
                               BK_INIT_INC, BK_FIRED, BK_SPARE, ELOG, EL_REWARD, EL_STEPS, EL_NEW_BEST, EL_RAN, HYPER_KEYS)
from .run import StopAfterEpisode, StopAfterEpisodeWithMinSteps, _episode_steps, _join, device_episodes_ok


def _refuse(msg):
    raise _lib.PdecError("Population: " + msg)


def _refuse_member(m, table):
    """the first refusal of `table` [(refused, why), ...] that applies to member m"""
    for refused, why in table:
        if refused:
            _refuse(f"member {m}: {why}")


def _not_of_this_setup(setup, ag):
    """a member's refusals that come before anything is allocated: it must be a learner of THIS setup"""
    if not isinstance(ag, Agent):
        return [(True, "an Agent with a PDEhook is needed")]
    pol, name, (ns, A) = ag.policy, type(setup).__name__, setup.state_shape
    rows, stride = pol.behavior_actor.model.dims[0], ag.trajectory.stride
    # (the global/mono agent and reward groups are refused by name, on the path's table)
    per_actuator = not (getattr(pol, "mono", None) or getattr(pol, "reward_group", None) is not None)
    return [
        (getattr(pol.behavior_actor.model, "noise_scale", None) is not None,
         "a noise scale array is set on its actor (set_noise_scale); a member explores at its own act_noise, which may differ from "
         "member to member"),
        (getattr(pol, "noise_corr", None) is not None or getattr(pol.behavior_actor.model, "noise_color", None) is not None,
         "a noise correlation is set on its policy (set_noise_corr); the member glue draws white noise only"),
        (per_actuator and (rows != ns or stride != A),
         f"its actor reads {rows} state rows and its replay takes {stride} columns per step, but {name} has {ns} state rows and {A} "
         "actuators: the member was not made for this setup"),
        (per_actuator and getattr(setup, "is_fluid", False) and stride > 256,
         f"{stride} actuators per step, and the device-episode path serves at most 256 (run.device_episodes_ok); of {name}'s "
         "experiments Fluid_8 and Fluid_16 are served, Fluid_32 is not")]


def _not_on_the_path(ag, hk, a0, probe):
    """a member's refusals on the device-episode path beside member 0 (`a0`), `probe` a B = 1 environment of the setup.
    (gamma, rho, the learning rates, act_noise and act_limit are each member's own: Population._hyper_rows)"""
    pol, tr, pol0, tr0 = ag.policy, ag.trajectory, a0.policy, a0.trajectory
    differs = [(getattr(pol, k) != getattr(pol0, k), f"hyper-parameter {k} differs from member 0's")
               for k in ("update_after", "update_freq", "update_loops", "batch_size", "start_steps", "quirk")]
    shapes = any(getattr(pol, k).model.dims != getattr(pol0, k).model.dims for k in ("behavior_actor", "behavior_critic"))
    return [
        (type(hk) is not PDEhook, "an Agent with a PDEhook is needed"),
        (getattr(pol, "mono", None) or getattr(pol, "reward_group", None) is not None,
         "the global/mono agent and reward groups are not served"),
        (pol.reducer is not None, "a reducer is not on the device-episode path"),
        (pol.memory_size, "memory_size > 0 is not on the device-episode path"),
        (pol.sampling != "device", "host sampling is not on the device-episode path"),
        (getattr(hk, "log_trajectory", 0) != 0, "log_trajectory != 0 is not on the device-episode path"),
        (not device_episodes_ok(ag, probe, StopAfterEpisode(1), hk),
         "a solo run would not take the device-episode path (run.device_episodes_ok: start policy, sampling, small update, streams)"),
        *differs,
        (shapes, "network shapes differ from member 0's"),
        (type(pol.start_policy) is not type(pol0.start_policy), "start policy differs from member 0's"),
        (tr.capacity != tr0.capacity or tr.stride != tr0.stride, "replay capacity differs from member 0's"),
        (getattr(tr.stream, "cuda_stream", None) != getattr(tr0.stream, "cuda_stream", None), "update stream differs from member 0's")]


class Population(_lib.Owned):
    def __init__(self, setup, agents, hooks, stream_env, dtype=torch.float64, device="cuda:0", part_streams=None,
                 max_log_bytes=8 << 30):
        """part_streams: handed to the population's PDEenv (the fluid steps its batch in parts on them where it splits it).
        max_log_bytes: the most the per-step slots of one episode (and the best-row copies of the block path) may take on the
        device; a fluid member's are (T + 1) + T full spectra and more (episode_log_bytes)."""
        M = len(agents)
        name = type(setup).__name__
        for refused, why in (
                (M < 1 or len(hooks) != M, "needs one hook per agent and at least one member"),
                (getattr(setup, "is_kseg2d", False),
                 f"{name} is not served (its batched step, part streams and initialisers need their own check); KSSetup, "
                 "KellerSegelSetup and FluidSetup are"),
                (dtype != torch.float64, "fp64 environments only (the shape of every reference-shaped run)"),
                (getattr(setup, "memory_size", 0), "memory_size > 0 is not on the device-episode path"),
                (stream_env is None, "needs an explicit environment stream (make_streams)")):
            if refused:
                _refuse(why)
        # a member is visited once per table: the probe stands between them, and the order of the refusals is kept across members
        for m, ag in enumerate(agents):
            _refuse_member(m, _not_of_this_setup(setup, ag))
        self.setup, self.agents, self.hooks, self.M = setup, list(agents), list(hooks), M
        probe = PDEenv(setup, B=1, dtype=dtype, device=device, stream=stream_env, autoreset=False)
        a0 = agents[0]
        for m, (ag, hk) in enumerate(zip(agents, hooks)):
            _refuse_member(m, _not_on_the_path(ag, hk, a0, probe))
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
        super().__init__(self.env.lib)
        lib = self.lib
        if not self.is_fluid:       # (the fluid step is per trajectory as it stands: no pairing of trajectories to re-arrange)
            _lib.check(lib.pdec_env_set_member_layout(self.env.handle, 1))
        self.cols = A = setup.state_shape[1]
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
        _lib.check(lib.pdec_population_create(
            C.byref(self.h), M, hs[0], hs[1], hs[2], hs[3], traces, seeds, losses, _lib.dtype_code(dtype), A, tr0.capacity,
            tr0.stride, int(pol0.update_loops), int(pol0.batch_size), float(pol0.y), pol0.rho_effective, int(pol0.quirk),
            float(pol0.behavior_actor.optimizer.eta), float(pol0.behavior_critic.optimizer.eta), int(pol0.update_after * tr0.stride),
            int(pol0.update_freq), int(pol0.start_steps), _lib.ptr(self.rows)))
        # (refused for network shapes whose update kernel takes one set for the whole launch: members then must not differ)
        if lib.pdec_population_set_member_hyper(self.h, 1) != 0:
            self._launch_wide = (lib.pdec_last_error().decode(errors="replace"), self._hyper_rows()[0, :4].copy())
            self._hyper_rows()
        for ag in agents:
            ag.policy.set_reward_interleave(1)
        with _on_stream(self.stream_upd):
            self._which = torch.zeros(M, dtype=torch.int32, device=self.env.device)
        # device buffers made at their first use and kept: the per-step slots and done flags of an episode
        # (population_episodes.episode_buffers), the book, episode log, best rows and error flags of a block (population_blocks)
        self._logs = self._flags = self._book = self._elog = self._best_rows = self._err = None
        self.episode_steps = []       # per episode: the control steps each member executed (0: idle)
        # host seconds per phase, summed over episodes: issue = initialisers + every enqueue up to the read-back,
        # readback = waiting for the device, settle = the members' host bookkeeping and the boundary launches
        # (blocks: read-backs; with episodes_per_sync = 1 every episode is one)
        self.timing = dict(episodes=0, issue_s=0.0, readback_s=0.0, settle_s=0.0, blocks=0)

    @property
    def _h(self):
        """the library's population object (the handle _lib.Owned releases)"""
        return self.h

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.pdec_destroy(self.h)
            self.h = _lib.Handle()

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
            _lib.check(self.lib.pdec_population_clone(self.h, src.ctypes.data_as(C.c_void_p), rows_sa.ctypes.data_as(C.c_void_p),
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
            post0 = self.agents[0].policy.reset_stage == POST_EPISODE_STAGE
            for m, (ag, hk) in enumerate(zip(self.agents, self.hooks)):
                _refuse_member(m, (
                    (hk.collect_history, "collect_history needs every episode's rows on the host; run it with episodes_per_sync=1"),
                    (hk.error_detection_given and not own_error_detection(self, hk),
                     "a hook with an error_detection callable is settled on the host every episode; run it with "
                     "episodes_per_sync=1"),
                    ((ag.policy.reset_stage == POST_EPISODE_STAGE) != post0,
                     "reset_stage differs from member 0's (one boundary launch serves all members)")))
        env, M = self.env, self.M
        s_env, s_upd = self.stream_env, self.stream_upd
        for ag, hk in zip(self.agents, self.hooks):
            hk(PRE_EXPERIMENT_STAGE, ag, env)
            ag(PRE_EXPERIMENT_STAGE, env)
        # the hooks' best / current actors (made at PRE_EXPERIMENT): the targets of the one copy launch per episode
        best = (_lib.Handle * M)(*[_handle_int(hk.bestNNA.model) if hk.collect_NNA else 0 for hk in self.hooks])
        cur = (_lib.Handle * M)(*[_handle_int(hk.currentNNA.model) if hk.collect_NNA else 0 for hk in self.hooks])
        _lib.check(self.lib.pdec_population_set_actor_copies(self.h, best, cur))
        active = np.ones(M, dtype=bool)
        while active.any():
            _join(s_upd, s_env)
            if E == 1:
                run_episode(self, active, stops)
            else:
                run_block(self, active, stops, block_length(stops, active, _episode_steps(env), E))
        _join(s_upd, s_env)
        for ag, hk in zip(self.agents, self.hooks):
            hk(POST_EXPERIMENT_STAGE, ag, env)
        return self.hooks
