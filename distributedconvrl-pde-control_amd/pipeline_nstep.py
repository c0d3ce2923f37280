"""n-step transitions of TrainPipeline (opt-in, n_step = n > 1; csrc/nstep.hip), assembled on the device.

One more launch on the env stream, pdec_nstep_step, behind everything that writes the rows of step k -- pdec_env_step, the clock
call, the ledger call, the last step's time-out fill -- and in front of pdec_reward_mean.  It stores (s_k, a_k, r_k, t_k) in a device
ring of depth n and writes nbatch[k % 3]: per column the transition that starts at step u = k - n + 1 -- s_u, a_u,
R = sum_{i <= m} gamma^i r_{u+i} up to the first terminal step u + m (m <= n - 1), T = 1 where there was one.  update_k trains on
nbatch[(k - LAG) % 3] with next_state = sring[(k - LAG + 1) % 6] and the scalar gamma_n; a cut window has T = 1 and does not
bootstrap, so one discount serves every column.  Every step emits cols transitions, each start once; transitions that start before
the last restart are not consumed: the first update is at k - LAG >= _first_tick + n - 1 (TrainPipeline._first_update), n - 1 steps
later than with n = 1.  pdec_reward_mean runs on the assembled reward and the env step's reward partials are not armed.  The ring
position is a device counter, so recorded steps and graphs carry the call."""
import ctypes as C

import numpy as np
import torch

from . import _lib


def check_n_step(n_step, use_replay):
    """the refusals of n_step, by name, before anything is allocated"""
    if isinstance(n_step, bool) or not isinstance(n_step, (int, np.integer)) or not 1 <= int(n_step) <= 32:
        raise _lib.PdecError(f"TrainPipeline(n_step={n_step!r}): an integer from 1 to 32")
    if int(n_step) > 1 and use_replay:
        raise _lib.PdecError(f"TrainPipeline(n_step={int(n_step)}): use_replay=True is not covered (the replay route pushes "
                             "one-step rows)")


def gamma_n(y, n):
    """w_n of w_0 = 1, w_{i+1} = w_i y: the discount of a full n-step window's bootstrap term, the product the assembling kernel
    forms"""
    w = 1.0
    for _ in range(n):
        w = w * float(y)
    return w


class NStep(_lib.Owned):
    """the n-step object of a pipeline (pdec_nstep_create) on the env stream and the batches it assembles, released with it"""

    def __init__(self, p):
        super().__init__(p.lib)
        self.policy, dt = p.policy, p.env.dtype
        _lib.check(self.lib.pdec_nstep_create(C.byref(self.h), p.n_step, p.cols, p.ns, p.na, _lib.dtype_code(dt)))
        _lib.check(self.lib.pdec_set_stream(self.h, p._sp_env))
        kw = dict(dtype=dt, device=p.env.device)
        # the batch assembled behind env step k (state, action, reward, terminal of the window that starts at step k - n + 1), a
        # ring of three like the one-step rows it replaces in the update
        with torch.cuda.stream(p.s_env):
            self.nbatch = [dict(state=torch.zeros((p.cols, p.ns), **kw), action=torch.zeros((p.cols, p.na), **kw),
                                reward=torch.zeros(p.cols, **kw), terminal=torch.zeros(p.cols, **kw)) for _ in range(3)]

    def step(self, st):
        """env stream: the transition that starts at step k - n + 1, from the rows as the calls in front have left them; returns
        the assembled reward, the one whose batch mean the reward broadcast takes"""
        L, nb = _lib, st.nb
        L.check(self.lib.pdec_nstep_step(self.h, L.ptr(st.s_in), L.ptr(st.act), L.ptr(st.rew), L.ptr(st.term), float(self.policy.y),
                                         L.ptr(nb["state"]), L.ptr(nb["action"]), L.ptr(nb["reward"]), L.ptr(nb["terminal"])))
        return nb["reward"]
