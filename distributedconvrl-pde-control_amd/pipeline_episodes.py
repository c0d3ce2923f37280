"""Episode bookkeeping of TrainPipeline (opt-in; PDEhook's, src/PDEhook.jl:42-97): the episode ledger, the episode-start draws and
the per-trajectory episode clock.

Ledger (`log_episodes`, lock-stepped episodes): one small launch behind every env step adds the step's per-trajectory mean reward
to an fp64 running return (a library call like the others, so recorded steps and graphs carry it), and the episode's last step,
which is eager, snapshots the parameters its acting kernel read, writes the episode's row and makes the hook's best-episode decision
without a read-back.

Draws (`random_init`): a new initial field for every episode at its (eager) first step, on the env stream, before the acting kernel
reads it.

Per-trajectory episodes (episodes="per_trajectory"; csrc/episode_clock.hip): the episode boundary is decided on the device.
pdec_epclock_step right behind pdec_env_step -- on the ring slots of step k: rring, fring, tring, aring[k % 3], ybuf[(k+1) % 2],
sring[(k+1) % 6] -- ends the episode of every trajectory whose blow-up flag is raised or whose own clock has reached
episode_steps, in that step: terminal row, log entry, restart field and its features, zero action_prev (a ring of two buffers the
clock writes and the next env step reads).  The host schedules as for episode_steps = 0: only step 0 is a first step, there is no
last step, every other step is interior -- the same launch sequence, recorded and captured.  The batch-mean reward of the reward
broadcast is taken by pdec_reward_mean behind the clock, on the rows it has sanitised; the env step's reward partials are not armed."""
import ctypes as C

import numpy as np
import torch

from . import _lib


def check_episode_mode(env, agent, episodes, stagger, episode_steps, use_replay, eval_every, min_best_episode, best_by):
    """the refusals of episodes="per_trajectory", by name, before anything is allocated"""
    if episodes not in ("lockstep", "per_trajectory"):
        raise _lib.PdecError(f"TrainPipeline(episodes={episodes!r}): 'lockstep' or 'per_trajectory'")
    if episodes == "lockstep":
        if stagger:
            raise _lib.PdecError("TrainPipeline(stagger=True) needs episodes='per_trajectory': lock-stepped episodes share one clock")
        return
    who = "TrainPipeline(episodes='per_trajectory')"
    setup, reducer = env.setup, agent.policy.reducer
    for refused, why in (
            (getattr(env, "is_fluid", False), ": the fluid environment is not covered (its step is a launch sequence with its own "
                                              "sensing)"),
            (getattr(setup, "is_kseg2d", False), ": the 2-D Keller-Segel environment is not covered (its step is a launch sequence "
                                                 "with its own sensing)"),
            (int(getattr(setup, "memory_size", 0)) > 0, ": memory_size > 0 is not covered"),
            (getattr(setup, "mono", False), ": the global agent (mono) is not covered"),
            (use_replay, ": use_replay=True is not covered (the replay route pushes lock-stepped episodes)"),
            (reducer is not None and reducer.active, ": not available with an active reducer"),
            (int(eval_every) > 0 or int(min_best_episode) > 0 or best_by == "eval",
             ": eval_every, min_best_episode and best_by='eval' are not available -- there is no common episode end to snapshot at; "
             "score actors with evaluate_actors between run() calls"),
            (int(episode_steps) <= 0, " needs episodes: episode_steps > 0")):
        if refused:
            raise _lib.PdecError(who + why)


def setup_episodes(p, log_episodes, min_best_episode, random_init, init_seed, init_rng, init_rank):
    """(ledger, draws, clock) of the pipeline p: the ledger and the clock None where their mode is off"""
    if int(log_episodes) < 0:
        raise _lib.PdecError(f"TrainPipeline(log_episodes={log_episodes}): a capacity >= 0")
    ledger = Ledger(p, log_episodes, min_best_episode) if int(log_episodes) > 0 and not p.per_traj else None
    inits = Inits(p, random_init, init_seed, init_rng, init_rank)
    return ledger, inits, Clock(p, log_episodes, inits) if p.per_traj else None


class Ledger(_lib.Owned):
    """the episode ledger of a pipeline (pdec_ledger_create): the last `capacity` lock-stepped episodes and the best actor"""

    def __init__(self, p, capacity, min_best_episode):
        super().__init__(p.lib)
        self.capacity, self.min_best_episode, self.B, self.n_episodes = int(capacity), int(min_best_episode), p.env.B, 0
        if p.E <= 0:
            raise _lib.PdecError("TrainPipeline(log_episodes=...) needs episodes: episode_steps > 0")
        if p.multi_rank and self.min_best_episode != 0:
            raise _lib.PdecError("TrainPipeline: best-actor tracking (min_best_episode) is not available with an active "
                                 "reducer: each rank would choose on its own trajectories")
        self.track_best = not p.multi_rank
        _lib.check(self.lib.pdec_ledger_create(C.byref(self.h), p.env.handle, p.actor.handle if self.track_best else 0, self.capacity))

    def step(self, st):
        """env stream, behind env step k: its per-trajectory mean reward onto the running returns"""
        _lib.check(self.lib.pdec_ledger_step(self.h, _lib.ptr(st.rew), _lib.ptr(st.flags)))

    def snapshot(self):
        """env stream, behind the acting kernel of an episode's last step: what that kernel read, before the actor half that waits
        for ev_act may rewrite it"""
        _lib.check(self.lib.pdec_ledger_snapshot(self.h))

    def close(self):
        """env stream, behind the last step of an episode: its row and the hook's best-episode decision"""
        _lib.check(self.lib.pdec_ledger_close(self.h, self.n_episodes, self.min_best_episode, int(self.track_best)))
        self.n_episodes += 1

    def discard(self):
        """reset_from() in the middle of an episode: the cut episode is not logged"""
        _lib.check(self.lib.pdec_ledger_discard(self.h))

    def returns(self):
        """TrainPipeline.episode_returns()"""
        N, B = self.capacity, self.B
        ret, blew = np.empty((N, B)), np.empty((N, B), dtype=np.int32)
        _lib.check(self.lib.pdec_ledger_read(self.h, _lib.ptr(ret), _lib.ptr(blew), None))
        rows, dropped = _lib.ring_rows(self.n_episodes, N)
        return ret[rows], blew[rows] != 0, dropped

    def means(self):
        """TrainPipeline.rewards"""
        means = np.empty(self.capacity)
        _lib.check(self.lib.pdec_ledger_read(self.h, None, None, _lib.ptr(means)))
        return [float(means[r]) for r in _lib.ring_rows(self.n_episodes, self.capacity)[0]]

    def best(self):
        """(batch-mean return, 1-based episode) of the best episode (best_by="train")"""
        if not self.track_best:
            raise _lib.PdecError("TrainPipeline: the best actor is not tracked with an active reducer")
        v, e = C.c_double(), C.c_int64()
        _lib.check(self.lib.pdec_ledger_best(self.h, C.byref(v), C.byref(e)))
        return v.value, e.value

    def best_params(self, out):
        """the parameters of the best episode's actor -> the network `out` (best_by="train")"""
        _lib.check(self.lib.pdec_ledger_best_params(self.h, out.handle))


class Inits:
    """the episode-start draws of a pipeline: which field the first step of an episode starts from"""

    def __init__(self, p, random_init, init_seed, init_rng, init_rank):
        env = self.env = p.env
        self.lib, self.s_env, self.state0 = p.lib, p.s_env, p.state0
        # init_rng, the fluid: None = the device draw of env.random_init, else random_init_device(env, rng)
        self.random_init, self.init_seed, self.init_rng = bool(random_init), int(init_seed), init_rng
        r, W = (int(v) for v in init_rank)
        if not 0 <= r < W:
            raise _lib.PdecError(f"TrainPipeline(init_rank={tuple(init_rank)}): rank r of W needs 0 <= r < W")
        self.init_rank = (r, W)
        # init_offsets: Philox offset of every initial field drawn (KS / Keller-Segel); keep_y0 (reset_from): this episode starts
        # from the field it was given, the next ones draw again
        self.init_offsets, self._init_ep, self.keep_y0 = [], 0, False
        if self.random_init:
            if env.is_fluid:
                if init_rng is not None and not hasattr(env.setup, "random_init_device"):
                    raise _lib.PdecError("TrainPipeline(random_init=True): the setup has no random_init_device")
            elif not getattr(env.setup, "device_random_init", True):
                raise _lib.PdecError("TrainPipeline(random_init=True): the setup has no device initialiser")
            if env.y0.data_ptr() == env.y.data_ptr():
                env.y0 = env.y0.clone()

    def draw(self):
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


class Clock(_lib.Owned):
    """the per-trajectory episode clock of a pipeline (pdec_epclock_create) and its log of `capacity` episodes per trajectory"""

    def __init__(self, p, capacity, inits):
        super().__init__(p.lib)
        env = self.env = p.env
        self.capacity, self.state0, self.fixed = int(capacity), p.state0, not inits.random_init
        _lib.check(self.lib.pdec_epclock_create(C.byref(self.h), env.handle, p.E, max(1, self.capacity), int(inits.random_init),
                                                inits.init_seed, *inits.init_rank))
        self.clock0 = np.array([(b * p.E) // env.B if p.stagger else 0 for b in range(env.B)], dtype=np.int32)
        # action_prev of step k, written by the clock of step k - 1 (the action ring slot is the transition's action and keeps its
        # values where a trajectory restarts)
        with torch.cuda.stream(p.s_env):
            self.aprev = [torch.zeros(env._ashape, dtype=env.dtype, device=env.device) for _ in range(2)]

    def step(self, st):
        """env stream, right behind env step k: the episode boundary of every trajectory, decided on the device -- the same call
        at every step"""
        L, env = _lib, self.env
        L.check(self.lib.pdec_epclock_step(self.h, L.ptr(st.rew), L.ptr(st.flags), L.ptr(st.term), L.ptr(st.act), L.ptr(st.act_next),
                                           L.ptr(st.y_out), L.ptr(st.s_out), L.ptr(env.y0) if self.fixed else None,
                                           L.ptr(self.state0) if self.fixed else None))

    def reset(self):
        """reset_from(): every clock back to its initial value; the cut episodes are not logged"""
        _lib.check(self.lib.pdec_epclock_set(self.h, _lib.ptr(self.clock0)))

    def finished(self):
        """TrainPipeline.episodes_finished"""
        cnt = np.empty(self.env.B, dtype=np.int64)
        _lib.check(self.lib.pdec_epclock_read(self.h, _lib.ptr(cnt), None, None, None, None))
        return cnt

    def finished_episodes(self):
        """TrainPipeline.finished_episodes()"""
        if self.capacity <= 0:
            raise _lib.PdecError("TrainPipeline: the episode log is off (log_episodes=0)")
        B, N = self.env.B, self.capacity
        cnt = np.empty(B, dtype=np.int64)
        ret, ln, blew, end = np.empty((B, N)), np.empty((B, N), dtype=np.int32), np.empty((B, N), dtype=np.int32), np.empty((B, N), dtype=np.int64)
        _lib.check(self.lib.pdec_epclock_read(self.h, _lib.ptr(cnt), _lib.ptr(ret), _lib.ptr(ln), _lib.ptr(blew), _lib.ptr(end)))
        rows = [(int(end[b, e % N]), b, e) for b in range(B) for e in range(max(0, int(cnt[b]) - N), int(cnt[b]))]
        rows.sort()
        tb = np.array([r[1] for r in rows], dtype=np.int64)
        te = np.array([r[2] for r in rows], dtype=np.int64)
        sl = te % N
        return dict(trajectory=tb, episode=te, ret=ret[tb, sl], length=ln[tb, sl], blew_up=blew[tb, sl] != 0, end_step=end[tb, sl],
                    dropped=int(np.maximum(cnt - N, 0).sum()))
