"""The device-replay route of TrainPipeline (opt-in, use_replay=True; eager only).

Every transition is pushed into the agent's device-resident replay (src/PDEagent.jl:254-289) and update_k trains on B * A
transitions drawn from it (:317-340) instead of the B * A fresh ones.  The pushes of step k run on the env stream behind
everything step k puts there; `ev_push[k % 2]` marks them done, and the sample of update_{k+1} -- on the update stream, drawn
against host counters that already include them -- waits for it.  The pushes of step k overwrite the oldest rows of a full ring, so
they in turn wait for the sample of update_k (`ev_samp`).  Ring positions, the sample count and the Philox offset are host
counters: both functions are re-evaluated at every step, recorded or not (_Lib.note), never replayed verbatim."""
import torch

from . import _lib


class Replay:
    """the pushes and the sample of a pipeline's control step, and the events that order them"""

    def __init__(self, p):
        self.lib, self.trajectory, self.policy, self.env_handle = p.lib, p.agent.trajectory, p.policy, p.env.handle
        self.cols, self.ns, self.na, self.serial, self.s_env, self.s_upd = p.cols, p.ns, p.na, p.serial, p.s_env, p.s_upd
        # replay pushes of step k done (env stream) / replay sample of update_k done (update stream)
        self.ev_push, self.ev_samp = [p._Ev(p.lib), p._Ev(p.lib)], p._Ev(p.lib)
        self._samp_pending, self.batch_cur = False, None

    def ready(self):
        """does the replay hold more than one step, so that the next sample() draws a batch"""
        return len(self.trajectory) > self.trajectory.stride

    def push(self, ev_done, s_in, act, rew, term, s_out, first, last):
        """the stage pushes of step k (src/PDEagent.jl:237-314).  They run on the ENV stream (launched through the env's
        handle), behind the env step / the time-out fill that produce their inputs; `ev_push[k % 2]` marks them done and
        the update that samples the replay next waits for it (see _issue).  (launched through the critic's
        handle they ran on the update stream, unordered against env_k, and copied stale rewards / flags.)"""
        tr, lib, h = self.trajectory, self.lib, self.env_handle
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

    def sample(self, ev_pushed):
        """the sampled batch of this step's update (pde_sample / pde_fetch!, src/PDEagent.jl:317-340) into the trajectory's
        fixed batch buffers -> self.batch_cur (None while the replay holds less than one step).  Re-evaluated at every step,
        recorded or not: the sample count, the ring fill and the Philox offset are host counters."""
        tr, pol = self.trajectory, self.policy
        self.batch_cur = None
        if ev_pushed is not None:
            # the host counters the sample is drawn against already include env_{k-1}'s pushes: wait for them
            # (the update stream has otherwise only waited for act_{k-1}, which precedes them on the env stream)
            ev_pushed.wait(self.s_upd)
        if not self.ready():
            return
        self.batch_cur = tr.sample_device(pol._sample_seed, pol._sample_off, self.cols, reuse=True)
        pol._sample_off += (self.cols + 3) // 4
        if not self.serial:
            # ... and env_k's pushes overwrite the oldest rows of a full ring: they wait for this sample
            self.ev_samp.record(self.s_upd)
            self._samp_pending = True

    def cut(self):
        """reset_from() in the middle of an episode: transition tick-1 is already in the ring with terminal = 0 and
        no POST_EPISODE dummy follows it, so the first (s, a) row of the new episode becomes its next_state and later samples
        would bootstrap across the reset.  Its rows are cut off instead: terminal = 1 (the layout a regular episode end leaves
        once its dummy row has been popped and overwritten).  On the env stream, behind the pushes."""
        tr = self.trajectory
        if tr.n_rt > 0 and tr.n_sa == tr.n_rt:
            with torch.cuda.stream(self.s_env):
                lo = (tr.n_rt - self.cols) % tr.capacity
                tr.terminal[lo:lo + self.cols].fill_(1.0)
