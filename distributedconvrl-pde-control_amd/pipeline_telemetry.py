"""Per-step training telemetry of TrainPipeline (opt-in, telemetry = N > 0; csrc/telemetry.hip), kept on the device.

Two more launches, each reducing what its stream has just written to one row of doubles in a device ring of N rows.
pdec_telemetry_step sits on the env stream behind the n-step call -- behind everything step k puts there -- and reads
sring[(k+1) % 6], aring / rring / tring / fring[k % 3] as those calls leave them: reward mean / min / max, action mean and
saturation, the largest state entry, blown-up and terminal counts, non-finite counts.  pdec_telemetry_update sits on the update
stream behind the last launch of update_k (in front of the event act_{k+1} waits for where that event is a record; where it rides
on the update's own launch, an event of its own behind the telemetry launch, `ev_tel`, orders it before the next chunk graph) and
reads the four networks' flat parameters and the loss pair: both losses, sum theta^2, the squared distance to the targets and to
the parameters at the previous call, the largest entry, non-finite counts.  It is issued at the updating steps with
k % telemetry_every == 0; telemetry_every divides the ring period, so a ring phase always holds the same calls.  The row counters
live on the device and are advanced by the one thread that writes the row, so no argument depends on the step and recorded steps
and graphs carry both calls.  Nothing is read back until pipe.telemetry()."""
import ctypes as C

import numpy as np

from . import _lib

# the columns of a telemetry row, in the device's order (csrc/telemetry.hip)
TELEMETRY_STEP_COLUMNS = ("step", "reward_mean", "reward_min", "reward_max", "reward_nonfinite", "action_mean", "action_abs_mean",
                          "action_saturated", "state_abs_max", "state_nonfinite", "blown_up", "terminal")
TELEMETRY_UPDATE_COLUMNS = ("update", "critic_loss", "actor_loss", "actor_norm2", "critic_norm2", "actor_target_dist2",
                            "critic_target_dist2", "actor_step2", "critic_step2", "actor_abs_max", "critic_abs_max",
                            "actor_nonfinite", "critic_nonfinite")


def check_telemetry(telemetry, telemetry_every, reducer):
    """the refusals of telemetry / telemetry_every, by name, before anything is allocated"""
    def integer(v):
        return not isinstance(v, bool) and isinstance(v, (int, np.integer))
    for refused, why in (
            (not integer(telemetry) or int(telemetry) < 0, f"(telemetry={telemetry!r}): an integer >= 0, the ring capacity in rows"),
            (not integer(telemetry_every) or int(telemetry_every) not in (1, 2, 3, 6),
             f"(telemetry_every={telemetry_every!r}): one of 1, 2, 3, 6 (a divisor of the ring period, so that a ring phase always "
             "holds the same calls)"),
            (integer(telemetry) and int(telemetry) > 0 and reducer is not None and reducer.active,
             f"(telemetry={telemetry}): not available with an active reducer (the actor's apply may run on a side stream beside the "
             "next critic half: no point of one stream sees a consistent parameter set)")):
        if refused:
            raise _lib.PdecError("TrainPipeline" + why)


def ring_columns(rows, calls, columns):
    """(name -> column of the last min(calls, N) rows of a ring of N, oldest first; how many earlier rows were overwritten)"""
    order, dropped = _lib.ring_rows(calls, rows.shape[0])
    kept = rows[order]
    return {name: kept[:, i].copy() for i, name in enumerate(columns)}, dropped


class Telemetry(_lib.Owned):
    """the telemetry object of a pipeline (pdec_telemetry_create), its step launch on the env stream, released with it"""

    def __init__(self, p):
        super().__init__(p.lib)
        pol = self.policy = p.policy
        self.capacity, self.every, self.cols, self.s_env, self.s_upd = p.telemetry_capacity, p.telemetry_every, p.cols, p.s_env, p.s_upd
        _lib.check(self.lib.pdec_telemetry_create(C.byref(self.h), self.capacity, p.env.B, p.cols, p.ns, p.na,
                                                  _lib.dtype_code(p.env.dtype), pol.behavior_actor.model.handle,
                                                  pol.behavior_critic.model.handle))
        _lib.check(self.lib.pdec_set_stream(self.h, p._sp_env))
        self.nets = tuple(n.model.handle for n in (pol.behavior_actor, pol.behavior_critic, pol.target_actor, pol.target_critic))
        self.ev_tel = p._Ev(self.lib)               # the telemetry launch behind update_k done (update stream)

    def step(self, st):
        """env stream: one row of facts about step k's own rows (not the assembled batch), as the calls in front have left them"""
        L = _lib
        L.check(self.lib.pdec_telemetry_step(self.h, L.ptr(st.s_out), L.ptr(st.act), L.ptr(st.rew), L.ptr(st.term), L.ptr(st.flags),
                                             float(self.policy.act_limit)))

    def update(self, st):
        """update stream, behind the last launch of update_k: the parameters and losses it leaves (a captured chunk joins through
        the event recorded behind this call, so the call stays in front of it)"""
        if st.k % self.every == 0:
            _lib.check(self.lib.pdec_telemetry_update(self.h, *self.nets, _lib.ptr(self.policy._losses)))
            if st.use_stop:
                # ev_upd[k % 2] rides on the update's own last launch and does not cover this one: a chunk graph launched on the
                # env stream next -- whose update branch rewrites what this launch reads and shares its ticket, partials and
                # counter -- waits for this event as well (wait_before_graph)
                self.ev_tel.record(self.s_upd)

    def wait_before_graph(self):
        """the last telemetry launch behind an eager update is not covered by ev_upd where that event rode on the update's own
        launch (a wait for an event never recorded, or recorded steps ago, is satisfied at once)"""
        self.ev_tel.wait(self.s_env)

    def read(self):
        """TrainPipeline.telemetry()"""
        N = self.capacity
        srows, urows = np.empty((N, len(TELEMETRY_STEP_COLUMNS))), np.empty((N, len(TELEMETRY_UPDATE_COLUMNS)))
        ns, nu, sent = C.c_int64(), C.c_int64(), np.empty(2, dtype=np.int64)
        _lib.check(self.lib.pdec_telemetry_read(self.h, _lib.ptr(srows), C.byref(ns), _lib.ptr(urows), C.byref(nu), _lib.ptr(sent)))
        step, ds = ring_columns(srows, ns.value, TELEMETRY_STEP_COLUMNS)
        upd, du = ring_columns(urows, nu.value, TELEMETRY_UPDATE_COLUMNS)
        step["action_saturated_fraction"] = step["action_saturated"] / float(self.cols)
        return dict(step=step, update=upd, dropped_steps=ds, dropped_updates=du,
                    first_nonfinite_step=None if sent[0] < 0 else int(sent[0]),
                    first_nonfinite_update=None if sent[1] < 0 else int(sent[1]))

    def reset(self):
        """TrainPipeline.telemetry_reset()"""
        _lib.check(self.lib.pdec_telemetry_reset(self.h))
