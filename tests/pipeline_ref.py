"""fp64 reference of TrainPipeline's control step, teacher-forced one step at a time (pipeline.py's module docstring:
act_k, env_k, update_k on the transition of step k - LAG).  Test infrastructure, host only; built on oracle/ and on
tests/small_update_ref.py (Snap, check_launch).

A run is a `Trace`: the learner state before step 0 and, after every step k, what the device holds -- y_k and y_{k+1}, the
ring slots of step k (s_k, a_k, r_k, t_k, flags, s_{k+1}), the four networks with both behaviour nets' ADAM moments and
beta powers, the losses, the device noise counter and, on the replay route, the replay traces with their counters.  Step k
is judged against the state the device had before it, never against an earlier reference result, so fp32 rounding does
not compound:

  act_k     a_k = clamp(A_k(s_k) + act_noise n_k, +-act_limit): A_k the actor after update_{k-1}; s_k = featurize(y0) at an
            episode's first step, else the s_{k+1} step k - 1 left; n_k = oracle.rng.randn(noise_seed, ctr_{k-1}, cols na).
            The counter advances by ceil(cols na / 4), what one acting call consumes.
  env_k     y_{k+1}, s_{k+1}, r_k, flags from the env oracle, starting from the read-back y_k -- from the episode's y0 with
            action_prev = 0 at its first step; t_k = 1 at an episode's last step, else the blow-up flag.
  update_k  none while k - LAG precedes the last restart (pipeline._first_tick), else one oracle.nn.ddpg_update on the
            transition j = k - LAG taken from the host history (the replay route: the rows oracle.rng.sample_slots names),
            judged by check_launch with reward groups / ReLU kinks as configured.

The env oracles: KSEnv (oracle/ks.py, the C2 / C3 shape) and KSeg2DEnv (oracle/keller_segel2d.py, the C4 shape).
Episodes are derived here, not read from the pipeline: they start at every restart tick and every E steps after it.  Every
check keeps its worst error as a fraction of its tolerance (`worst`), so a run can report how close it came.

Terminal transitions: at a regular episode end the act of the next episode's first step overwrites the s' slot of the
terminal transition with featurize(y0) (pipeline.py, `s_in.copy_(self.state0)`) before update_{j+LAG} reads it.  With
t = 1 the target gamma (1 - t) qt is 0, so nothing may depend on s' there; the reference uses the true s_{j+1}, which the
trace holds, and a kernel that wrongly bootstrapped across the end would show up as a gradient error."""
from dataclasses import dataclass, field

import numpy as np

from oracle import keller_segel2d as k2
from oracle import ks, nn
from oracle import rng as orng
from small_update_ref import B1, B2, Snap, check_launch

TOL_F = 1e-5          # fp32 forward (the acting kernel) vs fp64, relative to max(1, |ref|)
TOL_Y = 2e-5          # fp32 env step vs fp64, relative to max(1, |ref|) (tests/test_gpu_ks.py: y 2e-5, state / reward 1e-5)
TOL_SR = 1e-5
TOL_K2 = 2e-5         # fp32 2-D Keller-Segel step vs fp64, y / reward / state (tests/test_gpu_kseg2d.py)


@dataclass
class Config:
    """what the reference needs to know of a pipeline; nets as oracle.nn acts, arrays in the device layouts"""
    cols: int
    ns: int
    na: int
    lag: int
    E: int
    noise_seed: int
    act_noise: float
    act_limit: float
    gamma: float
    rho: float                  # the Polyak factor the update uses (1 under frozen targets)
    quirk: bool
    eta_a: float
    eta_c: float
    acts_a: list
    acts_c: list
    env: object                 # KSEnv-like: B, step(y, a_prev, a, s_prev), featurize(y), tolerances
    group: tuple = None         # (g, L) reward groups
    random_init: tuple = None   # (seed, counters per draw): every episode not started by reset_from draws a new y0
    replay: bool = False
    kinks: bool = True


@dataclass
class Rec:
    """what the device held after one step (or, for `init`, before step 0)"""
    snap: Snap
    ctr: int
    y_in: np.ndarray = None
    y_out: np.ndarray = None
    s_in: np.ndarray = None     # [cols, ns]
    s_out: np.ndarray = None
    a: np.ndarray = None        # [cols, na]
    r: np.ndarray = None        # [cols]
    t: np.ndarray = None        # [cols]
    flags: np.ndarray = None    # [B]
    replay: dict = None         # replay counters as the NEXT step's sample sees them


@dataclass
class Trace:
    init: Rec
    steps: list = field(default_factory=list)
    resets: dict = field(default_factory=dict)      # tick -> y0 [B, ...] handed to reset_from (0: the pipeline's own)


class KSEnv:
    """the 1-D Kuramoto-Sivashinsky env step of B lock-stepped trajectories, fp64 (oracle.ks), in the pipeline's layouts:
    y [B, nx], state [B A, ns], action [B A, na], reward [B A]"""

    def __init__(self, cfg, B):
        self.cfg, self.B = cfg, int(B)
        self.A = len(cfg.actuator_positions)
        self.tol = dict(y=TOL_Y, state=TOL_SR, reward=TOL_SR)

    def featurize(self, y):
        return np.concatenate([ks.featurize(self.cfg, yb).T for yb in np.asarray(y, np.float64)])

    def step(self, y, a_prev, a, s_prev=None):
        cfg, B, A = self.cfg, self.B, self.A
        a, a_prev = (np.asarray(x, np.float64).reshape(B, A, -1).transpose(0, 2, 1) for x in (a, a_prev))   # [B, na, A]
        p = np.stack([ks.prepare_action(cfg, a[b]) for b in range(B)])
        yn = ks.do_step(cfg, np.asarray(y, np.float64), p)                   # (batched over the leading axis)
        r = np.concatenate([ks.reward_function(cfg, yn[b], a[b], a[b] - a_prev[b]) for b in range(B)])
        done = np.abs(yn).max(axis=1) > cfg.max_value
        return dict(y=yn, state=self.featurize(yn), reward=r, done=done)

    def random_init(self, seed, off):
        """pdec_env_random_init as the oracle names it (oracle.rng.random_init_coefficients, KSSetup.jl:288-298)"""
        a = orng.random_init_coefficients(seed, off, self.B, 8)
        xx = self.cfg.dx * np.arange(1, self.cfg.nx + 1)
        y = sum(a[:, i - 1:i] * np.sin(i * xx / (2 * np.pi))[None] for i in range(1, 9))
        return y * 30 / np.linalg.norm(y, axis=1, keepdims=True)


class KSeg2DEnv:
    """the 2-D Keller-Segel env step (oracle/keller_segel2d.py) of B trajectories in the pipeline's layouts: y [B, ny, nx, 2]
    (u, v interleaved per cell), state [B A, ns] (temporal stack: the fresh rows over the newest rows of s_prev), action
    [B A, na], reward [B A]"""

    def __init__(self, cfg, B):
        self.cfg, self.B, self.A = cfg, int(B), cfg.A
        self.tol = dict(y=TOL_K2, state=TOL_K2, reward=TOL_K2)

    def _feat(self, yh, s_prev):
        A = self.A
        return np.concatenate([k2.featurize(self.cfg, yh[b], None if s_prev is None else s_prev[b * A:(b + 1) * A].T).T
                               for b in range(self.B)])

    def featurize(self, y):
        return self._feat(np.moveaxis(np.asarray(y, np.float64), -1, 1), None)

    def step(self, y, a_prev, a, s_prev=None):
        cfg, B, A = self.cfg, self.B, self.A
        yh = np.moveaxis(np.asarray(y, np.float64), -1, 1)                   # [B, 2, ny, nx]
        a, a_prev = (np.asarray(x, np.float64).reshape(B, A, -1).transpose(0, 2, 1) for x in (a, a_prev))
        p = np.stack([k2.prepare_action(cfg, a[b]) for b in range(B)])
        # batched over a trailing axis: the oracle's neighbours / RK4 act on the leading (species, y, x) axes only
        yn = k2.do_step(cfg, yh.transpose(1, 2, 3, 0), p.transpose(1, 2, 0)).transpose(3, 0, 1, 2)
        r = np.concatenate([k2.reward_function(cfg, yn[b], a[b], a[b] - a_prev[b]) for b in range(B)])
        done = np.abs(yn).reshape(B, -1).max(axis=1) > cfg.max_value
        return dict(y=np.moveaxis(yn, 1, -1), state=self._feat(yn, np.asarray(s_prev, np.float64)), reward=r, done=done)


def kseg2d_config(setup, border=2):
    """the oracle configuration of a KellerSegel2DSetup built with `border`"""
    cfg = k2.KSeg2DConfig(nx=setup.nx, ny=setup.ny, Lx=setup.Lx, sensor_x=setup.sensor_x, sensor_y=setup.sensor_y,
                          border_x=border, half_window=setup.half_window, dt=setup.dt, te=setup.te,
                          agent_power=setup.agent_power, window_size=setup.window_size, temporal_steps=setup.temporal_steps,
                          action_punish=setup.action_punish, delta_action_punish=setup.delta_action_punish,
                          max_value=setup.max_value, substeps=setup.oversampling)
    assert np.array_equal(cfg.a2s, setup.actuators_to_sensors - 1)
    return cfg


def ks_config(setup):
    """the oracle configuration of a KSSetup (the fields the C2 / C3 benches set)"""
    return ks.KSConfig(setup.nx, setup.Lx, setup.sensor_positions, actuator_positions=setup.actuator_positions,
                       sigma_sensors=setup.sigma_sensors, sigma_actuators=setup.sigma_actuators, mu=setup.mu, dt=setup.dt,
                       oversampling=setup.oversampling, max_value=setup.max_value, agent_power=setup.agent_power,
                       action_punish=setup.action_punish, delta_action_punish=setup.delta_action_punish,
                       window_size=setup.window_size, te=setup.te)


# ---------------------------------------------------------------------------------------------------- episodes
def schedule(cfg, trace, n):
    """per step k < n: (first, last, first_tick, episode start tick).  Episodes start at every restart and every E steps
    after it; first_tick is the last restart at or before k (updates of transitions before it are dropped)"""
    starts = sorted(set(trace.resets) | {0})
    out = []
    for k in range(n):
        r = max(t for t in starts if t <= k)
        e = k - r
        first = e % cfg.E == 0 if cfg.E > 0 else e == 0
        last = cfg.E > 0 and e % cfg.E == cfg.E - 1
        out.append((first, last, r, k - (e % cfg.E if cfg.E > 0 else e)))
    return out


def episode_y0(cfg, trace, n):
    """tick of every episode start < n -> the y0 it must start from (fp64): the field handed to reset_from at a restart,
    a new random field otherwise when random_init is on (draw i from Philox offset i x counters per draw; the first
    episode draws too: the constructor's own restart does not keep its field), else the last"""
    out, y0, draws = {}, None, 0
    for k, (first, _l, _r, _s) in enumerate(schedule(cfg, trace, n)):
        if not first:
            continue
        if k in trace.resets:
            y0 = np.asarray(trace.resets[k], np.float64)
        elif cfg.random_init is not None:
            seed, per = cfg.random_init
            y0 = cfg.env.random_init(seed, draws * per)
            draws += 1
        out[k] = y0
    return out


# ---------------------------------------------------------------------------------------------------- checks
def _keep(worst, key, ratio):
    worst[key] = max(worst.get(key, 0.0), float(ratio))


def _same_snap(a, b):
    return all(np.array_equal(x, y) for fa, fb in ((a.A, b.A), (a.C, b.C), (a.At, b.At), (a.Ct, b.Ct), (a.mA, b.mA),
                                                    (a.vA, b.vA), (a.mC, b.mC), (a.vC, b.vC)) for x, y in zip(fa, fb)) \
        and np.array_equal(a.bpA, b.bpA) and np.array_equal(a.bpC, b.bpC)


def check_act(cfg, k, prev, rec, s_k, worst):
    errs = []
    ref_pre = nn.forward([np.asarray(p, np.float64) for p in prev.snap.A], cfg.acts_a, np.asarray(s_k, np.float64).T).T
    noise = orng.randn(cfg.noise_seed, prev.ctr, cfg.cols * cfg.na).reshape(cfg.cols, cfg.na)
    ref_pre = ref_pre + cfg.act_noise * noise
    ref = np.clip(ref_pre, -cfg.act_limit, cfg.act_limit)
    e = float((np.abs(rec.a - ref) / (TOL_F * np.maximum(1.0, np.abs(ref_pre)))).max())
    _keep(worst, "act", e)
    if not e <= 1:
        errs.append(f"act (step {k}): action off by {e:.3g} x its tolerance (actor after update_{k - 1}, noise offset "
                    f"{prev.ctr})")
    want = prev.ctr + (cfg.cols * cfg.na + 3) // 4
    if rec.ctr != want:
        errs.append(f"noise counter (step {k}): {prev.ctr} -> {rec.ctr}, one acting call advances it to {want}")
    return errs


def check_env(cfg, k, rec, y_k, s_k, a_prev, first, last, drawn, worst):
    """drawn: the step starts from a random field the device computed itself (fp32 rounding allowed); every other y_k is
    an exact copy"""
    errs, env = [], cfg.env
    tol_in = TOL_F * max(1.0, float(np.abs(y_k).max())) if drawn else 0.0
    e = float(np.abs(rec.y_in.astype(np.float64) - y_k).max())
    if not e <= tol_in:
        errs.append(f"env y_in (step {k}): the step started {e:.3g} away from {'y0' if first else 'y_k'}")
    o = env.step(np.asarray(y_k, np.float64), a_prev, rec.a, s_k)
    for name, got, ref in (("y", rec.y_out, o["y"]), ("state", rec.s_out, o["state"]), ("reward", rec.r, o["reward"])):
        ratio = float(np.abs(np.asarray(got, np.float64).reshape(ref.shape) - ref).max()) / (
            env.tol[name] * max(1.0, float(np.abs(ref).max())))
        _keep(worst, f"env {name}", ratio)
        if not ratio <= 1:
            errs.append(f"env {name} (step {k}): off by {ratio:.3g} x its tolerance")
    if not np.array_equal(rec.flags != 0, o["done"]):
        errs.append(f"env flags (step {k}): blow-up flags {np.flatnonzero(rec.flags)} vs {np.flatnonzero(o['done'])}")
    want_t = np.repeat(np.ones(env.B) if last else (rec.flags != 0).astype(np.float64), cfg.cols // env.B)
    if not np.array_equal(rec.t.astype(np.float64), want_t):
        errs.append(f"env term (step {k}): terminal flags {'not all 1 at the episode end' if last else 'differ from the blow-up flags'}")
    return errs, o


def replay_rows(cfg, rp):
    """(step, column) of the host history behind every row update_k samples: oracle.rng.sample_slots for the counters step
    k - 1 left.  Every step pushes its cols transitions in column order, so logical row lg (the r / t slot lg % capacity,
    lg in the window [max(0, n_rt - capacity), n_rt)) is column lg % cols of step lg // cols"""
    slots = orng.sample_slots(rp["seed"], rp["offset"], cfg.cols, rp["n_valid"], rp["n_rt"], rp["capacity"], rp["stride"])
    base = max(0, rp["n_rt"] - rp["capacity"])
    lg = base + (slots[1] - base) % rp["capacity"]
    return lg // cfg.cols, lg % cfg.cols


def transition(cfg, trace, j, k):
    """the minibatch update_k trains on, from the host history -- transition j, or on the replay route the rows
    sample_slots names -- in the oracle's [features, columns] layout (s' of a terminal row: see the module doc)"""
    if cfg.replay:
        rp = trace.steps[k - 1].replay if k > 0 else trace.init.replay
        if rp["n_valid"] <= rp["stride"]:
            return None
        step, col = replay_rows(cfg, rp)
        pick = lambda name: np.stack([getattr(trace.steps[i], name)[c] for i, c in zip(step, col)])
        return pick("s_in").T, pick("a").T, pick("r"), pick("t"), pick("s_out").T
    st = trace.steps[j]
    return st.s_in.T, st.a.T, st.r, st.t, st.s_out.T


def check_update(cfg, trace, k, prev, rec, upd, worst):
    j = k - cfg.lag
    if not upd:
        if not _same_snap(prev.snap, rec.snap):
            return [f"update (step {k}): the learner changed, but transition {j} precedes the episode's first update"]
        return []
    mb = transition(cfg, trace, j, k)
    if mb is None:
        return [] if _same_snap(prev.snap, rec.snap) else [f"update (step {k}): the learner changed with an empty replay"]
    errs = check_launch(prev.snap, rec.snap, [mb], cfg.acts_a, cfg.acts_c, cfg.gamma, cfg.rho, cfg.quirk, cfg.eta_a,
                        cfg.eta_c, group=cfg.group, kinks=cfg.kinks, worst=worst)
    return [f"update (step {k}, transition {j}): {e}" for e in errs]


def check_trace(cfg, trace):
    """(errors, worst): what is wrong with every step of the trace, and the worst error of each check as a fraction of its
    tolerance"""
    n = len(trace.steps)
    sch = schedule(cfg, trace, n)
    y0s = episode_y0(cfg, trace, n)
    errs, worst = [], {}
    for k, rec in enumerate(trace.steps):
        first, last, first_tick, start = sch[k]
        prev = trace.steps[k - 1] if k > 0 else trace.init
        drawn = first and k not in trace.resets and cfg.random_init is not None
        if cfg.replay and rec.replay["n_rt"] != (k + 1) * cfg.cols:
            errs.append(f"replay (step {k}): {rec.replay['n_rt']} transitions pushed after {k + 1} steps of {cfg.cols}")
        if first:
            y_k = np.asarray(y0s[k], np.float64)
            y_dev = np.asarray(y_k, dtype=rec.y_in.dtype).astype(np.float64)       # the y0 the device holds, rounded
            s_k = cfg.env.featurize(y_dev)
            a_prev = np.zeros_like(rec.a)
            e = float(np.abs(rec.s_in - s_k).max()) / cfg.env.tol["state"]
            _keep(worst, "state0", e)
            if not e <= 1:
                errs.append(f"act s_k (step {k}): the first state is {e:.3g} x its tolerance from featurize(y0)")
        else:
            y_k = prev.y_out.astype(np.float64)
            y_dev = y_k
            s_k = prev.s_out
            a_prev = prev.a
            if not np.array_equal(rec.s_in, s_k):
                errs.append(f"act s_k (step {k}): the acting kernel's state is not the s_(k+1) step {k - 1} left")
        errs += check_act(cfg, k, prev, rec, s_k, worst)
        e_env, _ = check_env(cfg, k, rec, y_dev, s_k, a_prev, first, last, drawn, worst)
        errs += e_env
        errs += check_update(cfg, trace, k, prev, rec, k - cfg.lag >= first_tick, worst)
    return errs, worst


def n_updates(cfg, trace, n):
    """the updates n steps issue: one per step whose transition k - LAG is at or after the last restart"""
    return sum(1 for k, (_f, _l, ft, _s) in enumerate(schedule(cfg, trace, n)) if k - cfg.lag >= ft)


# ---------------------------------------------------------------------------------------------------- device read-back
def snap_of(pkg, pipe):
    """the learner as the device holds it (synchronise first)"""
    ck = pkg.checkpoint
    pol = pipe.policy
    nets = [getattr(pol, n).model for n in ("behavior_actor", "behavior_critic", "target_actor", "target_critic")]
    P = [[np.array(p) for p in m.params()] for m in nets]
    (mA, vA, bpA), (mC, vC, bpC) = (ck._adam_state(m) for m in nets[:2])
    # before its first step the library reports the beta powers as -1 (not initialised); Flux's state then holds beta
    bpA, bpC = (np.array([B1, B2]) if bp[0] < 0 else bp for bp in (bpA, bpC))
    al, cl = pol.losses()
    return Snap(P[0], P[1], P[2], P[3], nets[0]._unflatten(mA), nets[0]._unflatten(vA), nets[1]._unflatten(mC),
                nets[1]._unflatten(vC), np.array(bpA), np.array(bpC), (cl, al))


def noise_counter(pipe):
    import ctypes as C
    v = C.c_uint64()
    pipe.lib.pdec_noise_counter_get(pipe.actor.handle, C.byref(v))
    return int(v.value)


def _np(x):
    return x.detach().cpu().numpy().copy()


def replay_of(pipe):
    """the host counters the next replay sample is drawn against (its rows are taken from the trace's history)"""
    tr, pol = pipe.agent.trajectory, pipe.policy
    return dict(n_valid=len(tr), n_rt=tr.n_rt, capacity=tr.capacity, stride=tr.stride, seed=pol._sample_seed,
                offset=pol._sample_off)


def record_step(pkg, pipe, k):
    """read back what step k left (after pipe.sync())"""
    P = 6
    cols = pipe.cols
    rec = Rec(snap_of(pkg, pipe), noise_counter(pipe), y_in=_np(pipe.ybuf[k % 2]), y_out=_np(pipe.ybuf[(k + 1) % 2]),
              s_in=_np(pipe.sring[k % P]).reshape(cols, -1), s_out=_np(pipe.sring[(k + 1) % P]).reshape(cols, -1),
              a=_np(pipe.aring[k % 3]).reshape(cols, -1), r=_np(pipe.rring[k % 3]).reshape(-1),
              t=_np(pipe.tring[k % 3]).reshape(-1), flags=_np(pipe.fring[k % 3]))
    if pipe.use_replay:
        rec.replay = replay_of(pipe)
    return rec


def run_teacher_forced(pkg, pipe, n, resets=None):
    """step the pipeline eagerly one step at a time (run(1), sync) and record every step; resets: tick -> y0 device
    tensor handed to reset_from() before that step"""
    pipe.sync()
    trace = Trace(Rec(snap_of(pkg, pipe), noise_counter(pipe)))
    if pipe.use_replay:
        trace.init.replay = replay_of(pipe)
    if not pipe.random_init:            # (with random inits the first episode draws its field as well)
        trace.resets[0] = _np(pipe.env.y0).astype(np.float64)
    for k in range(n):
        if resets and k in resets:
            pipe.reset_from(resets[k])
            pipe.sync()
            trace.resets[k] = _np(resets[k]).astype(np.float64)
        assert pipe.tick == k
        pipe.run(1)
        pipe.sync()
        trace.steps.append(record_step(pkg, pipe, k))
    return trace


def config_of(pipe, env_ref, **kw):
    pol = pipe.policy
    A, Cn = pol.behavior_actor.model, pol.behavior_critic.model
    group = None if pol.reward_group is None else (pol.reward_group, pipe.reward_interleave)
    ri = None
    if pipe.random_init:
        ri = (pipe.init_seed, pipe.env.B * ((pipe.env.random_init_coefficients() + 3) // 4))
    return Config(cols=pipe.cols, ns=pipe.ns, na=pipe.na, lag=pipe.LAG, E=pipe.E, noise_seed=pipe.noise_seed,
                  act_noise=float(pol.act_noise), act_limit=float(pol.act_limit), gamma=float(pol.y),
                  rho=float(pol.rho_effective), quirk=bool(pol.quirk), eta_a=float(pol.behavior_actor.optimizer.eta),
                  eta_c=float(pol.behavior_critic.optimizer.eta), acts_a=list(A.acts), acts_c=list(Cn.acts), env=env_ref,
                  group=group, random_init=ri, replay=pipe.use_replay, **kw)
