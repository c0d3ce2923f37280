"""Greedy held-out evaluation of TrainPipeline (opt-in, `eval_every`; needs the episode ledger of pipeline_episodes.py).

Behind the last step of every eval_every-th episode the ledger's snapshot of that step is rolled out without noise on an
environment of its own from K fixed held-out fields, and the ledger scores it on the device -- per trajectory b, from the rollout's
reward_sum [K][R] and done_step [K]: ret_b = (sum_a (double) reward_sum[b][a]) / R in a order, blew_b = done_step[b] >= 0;
score = (sum_b ret_b) / K in b order, NaN when any blew_b is set or any ret_b is not finite (population.score_members' rule;
`eval_score` restates it on the host).  Enqueued at the (eager) last step, never inside a capture or a recorded step:

    env stream:   [wait eval_{n-1} done] -> pdec_ledger_eval_load (staging -> evaluation actor) -> event
    eval stream:  wait event -> reset the evaluation env to eval_y0 -> pdec_rollout -> pdec_ledger_eval_close -> done event

With eval_stream=None the eval stream is the env stream (behind the episode's last env step, no events)."""
import ctypes as C

import numpy as np
import torch

from . import _lib


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


def held_out_fields(setup, K, seed, dtype, device, stream):
    """(environment of B = K trajectories on `stream`, K held-out fields [K, ...] of their own storage): the Philox stream
    (seed, 0) of env.random_init; the fluid: setup.random_init_device(env, np.random.default_rng(seed)), the vortex tables of its
    own initialiser.  The one draw of TrainPipeline(eval_every=...) and population.evaluate_actors: both score on the same fields."""
    from .env import PDEenv
    env = PDEenv(setup, B=int(K), dtype=dtype, device=device, stream=stream, autoreset=False)
    if getattr(setup, "is_fluid", False):
        y0 = setup.random_init_device(env, np.random.default_rng(int(seed)))
    else:
        y0 = torch.empty_like(env.y)
        env.random_init(int(seed), 0, out=y0)
    return env, y0.clone()


def check_eval_args(env, agent, episode_steps, s_env, s_upd, log_episodes, eval_every, eval_inits, eval_y0, eval_capacity,
                    eval_stream, best_by):
    """the refusals of the evaluation arguments, by name, before anything is allocated (s_env, s_upd: the pipeline's streams, None
    where neither the caller nor the environment / the networks name one)"""
    if best_by not in ("train", "eval"):
        raise _lib.PdecError(f"TrainPipeline(best_by={best_by!r}): 'train' or 'eval'")
    if int(eval_every) < 0:
        raise _lib.PdecError(f"TrainPipeline(eval_every={eval_every}): a period >= 0")
    if int(eval_every) == 0:
        if best_by == "eval":
            raise _lib.PdecError("TrainPipeline(best_by='eval') needs evaluations: eval_every > 0")
        return
    reducer = agent.policy.reducer
    for refused, why in (
            (int(log_episodes) <= 0, "(eval_every=...) needs the episode ledger, which holds the snapshot: log_episodes > 0"),
            (int(episode_steps) <= 0, "(eval_every=...) needs episodes: episode_steps > 0"),
            (reducer is not None and reducer.active, "(eval_every=...) is not available with an active reducer: the ledger keeps no "
                                                     "snapshot there"),
            (int(eval_inits) < 1, f"(eval_inits={eval_inits}): at least one held-out field"),
            (int(eval_capacity) < 1, f"(eval_capacity={eval_capacity}): at least one row")):
        if refused:
            raise _lib.PdecError("TrainPipeline" + why)
    if eval_y0 is not None:
        shape = tuple(eval_y0.shape) if hasattr(eval_y0, "shape") else np.shape(eval_y0)
        if len(shape) != len(env._yshape) or shape[0] < 1 or shape[1:] != tuple(env._yshape[1:]):
            raise _lib.PdecError(f"TrainPipeline(eval_y0=...): expected shape (K,) + {tuple(env._yshape[1:])}, got {shape}")
    if eval_stream is not None and s_upd is not None and eval_stream.cuda_stream == s_upd.cuda_stream and (
            s_env is None or s_env.cuda_stream != s_upd.cuda_stream):
        raise _lib.PdecError("TrainPipeline(eval_stream=...): the update stream cannot carry the evaluation; None (the "
                             "env stream) or a third stream")


class Evaluation:
    """the evaluation environment, actor, held-out fields and zero-action baseline of a pipeline (one synchronisation when made),
    its launches and its readers; the rows and the best evaluated actor live in the pipeline's ledger"""

    def __init__(self, p, eval_every, eval_inits, eval_seed, eval_y0, eval_capacity, eval_stream):
        from .env import PDEenv
        from .nna import HipMLP
        env, lib = p.env, p.lib
        self.lib, self.ledger, self.policy, self.E, self.s_env = lib, p.ledger, p.policy, p.E, p.s_env
        self.every, self.capacity, self.n_evals = int(eval_every), int(eval_capacity), 0
        s = self.s_eval = eval_stream if eval_stream is not None else p.s_env
        self._aside = s.cuda_stream != p.s_env.cuda_stream
        with torch.cuda.stream(s):
            if eval_y0 is None:
                ee, y0 = held_out_fields(env.setup, eval_inits, eval_seed, env.dtype, env.device, s)
            else:
                y0 = (eval_y0 if isinstance(eval_y0, torch.Tensor) else torch.as_tensor(np.array(eval_y0, copy=True)))
                y0 = y0.to(device=env.device, dtype=env.dtype).contiguous().clone()
                ee = PDEenv(env.setup, B=int(y0.shape[0]), dtype=env.dtype, device=env.device, stream=s, autoreset=False)
            K = int(y0.shape[0])
            self.eval_env, self.eval_y0, self.K = ee, y0, K
            m = p.actor
            self.eval_actor = HipMLP(m.dims, m.acts, None, env.dtype, m.device, max(K * env.setup.state_shape[1], m.max_cols),
                                     s)                                                    # all parameters 0
            self._eval_rsum = torch.zeros((K, env.setup.reward_len), dtype=env.dtype, device=env.device)
            self._eval_done = torch.zeros((2, K), dtype=torch.int32, device=env.device)        # done_any, done_step
        _lib.check(lib.pdec_ledger_eval_attach(self.ledger.h, ee.handle, self.eval_actor.handle, self.capacity))
        # evaluation actor loaded (env stream) / evaluation closed (eval stream) / an evaluation may still be running
        self.ev_eload, self.ev_edone, self._pending = p._Ev(lib), p._Ev(lib), False
        # the zero action on the same fields: the rollout of the all-zero actor the evaluation actor still is.  It also makes
        # every lazily created buffer of the rollout path, so that the evaluations of the run enqueue and return.
        self._rollout()
        s.synchronize()
        self.eval_zero_score = eval_score(self._eval_rsum.cpu().numpy(), self._eval_done[1].cpu().numpy())[2]

    def due(self):
        """is the episode the ledger closes next (1-based number n_episodes + 1) an evaluated one"""
        return (self.ledger.n_episodes + 1) % self.every == 0

    def _rollout(self):
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

    def load(self):
        """env stream, behind the snapshot of an evaluated episode's last step: the staged parameters -> the evaluation actor"""
        if self._aside and self._pending:
            self.ev_edone.wait(self.s_env)              # the previous evaluation still reads the actor being rewritten
        _lib.check(self.lib.pdec_ledger_eval_load(self.ledger.h))
        if self._aside:
            self.ev_eload.record(self.s_env)

    def run(self):
        """the evaluation of the episode the ledger has just closed, on the eval stream (the env stream: behind everything the
        episode's last step puts there)"""
        if self._aside:
            self.ev_eload.wait(self.s_eval)
        self._rollout()
        with torch.cuda.stream(self.s_eval):
            _lib.check(self.lib.pdec_ledger_eval_close(self.ledger.h, _lib.ptr(self._eval_rsum), _lib.ptr(self._eval_done[1]),
                                                       self.n_evals, self.ledger.n_episodes, self.ledger.min_best_episode))
        self.n_evals += 1
        if self._aside:
            self.ev_edone.record(self.s_eval)
            self._pending = True

    def returns(self):
        """TrainPipeline.eval_returns()"""
        N, K = self.capacity, self.K
        eps, ret, blew = np.empty(N, dtype=np.int64), np.empty((N, K)), np.empty((N, K), dtype=np.int32)
        _lib.check(self.lib.pdec_ledger_eval_read(self.ledger.h, _lib.ptr(eps), _lib.ptr(ret), _lib.ptr(blew), None))
        rows, dropped = _lib.ring_rows(self.n_evals, N)
        return eps[rows], ret[rows], blew[rows] != 0, dropped

    def scores(self):
        """TrainPipeline.eval_scores"""
        sc = np.empty(self.capacity)
        _lib.check(self.lib.pdec_ledger_eval_read(self.ledger.h, None, None, None, _lib.ptr(sc)))
        return sc[_lib.ring_rows(self.n_evals, self.capacity)[0]]

    def best(self):
        """(score, 1-based episode) of the best evaluation (best_by="eval")"""
        v, e = C.c_double(), C.c_int64()
        _lib.check(self.lib.pdec_ledger_eval_best(self.ledger.h, C.byref(v), C.byref(e)))
        return v.value, e.value

    def best_params(self, out):
        """the parameters of the best evaluated actor -> the network `out` (best_by="eval")"""
        _lib.check(self.lib.pdec_ledger_eval_best_params(self.ledger.h, out.handle))
