"""GPU tests of the trajectory glue at its seams: csrc/replay.hip (replay_push2_kernel, replay_push_rt_kernel, replay_sample_kernel,
autoreset_kernel), the pushes of csrc/act.hip's step_glue_kernel and the slot table of csrc/small_args.hpp, every row of
replay_ring_cases.py against the plain model of replay_ring_ref.py.  These kernels copy, cast fp64 -> fp32 and do integer
arithmetic, so every comparison is exact (np.array_equal; NaN positions by mask where NaNs are planted).
test_replay_ring_table.py holds the table's claims and shows that each comparison rejects the mistake it is there for."""
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

import replay_ring_cases as rc
import replay_ring_ref as ref
from oracle import rng as orng

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TRACES = ("state", "action", "reward", "terminal")


@pytest.fixture(scope="module")
def net(pkg):
    """any live handle serves as any_handle: a 1 -> 1 network on the default stream"""
    return import_module(pkg.__name__ + ".nna").HipMLP([1, 1], ["identity"])


def dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


class Driver:
    """the ops of a row on the device: through CircularArraySARTTrajectory bound to the handle where the class can express the
    row, through the C entry points otherwise.  Counters move as the host's do."""

    def __init__(self, pkg, net, row):
        self.L, self.lib, self.h, self.row = pkg._lib, net.lib, net.handle, row
        self.cap, self.cap1 = row.cap, row.cap + row.stride
        self.tr = None
        if rc.expressible(row):
            self.tr = pkg.CircularArraySARTTrajectory(row.cap, row.ns, row.na, row.stride, torch.device("cuda:0")).bind(net)
            assert self.tr.capacity == row.cap
            self.traces = {k: getattr(self.tr, k) for k in TRACES}
        else:
            kw = dict(dtype=torch.float32, device="cuda:0")
            self.traces = dict(state=torch.zeros((self.cap1, row.ns), **kw), action=torch.zeros((self.cap1, row.na), **kw),
                               reward=torch.zeros(row.cap, **kw), terminal=torch.zeros(row.cap, **kw))
        if row.prefill:
            for k, v in rc.sentinel(row).items():
                self.traces[k].copy_(dev(v))
        self._n_sa = self._n_rt = 0
        self.halt = None
        self.dt = torch.float64 if row.dtype == "f64" else torch.float32
        torch.cuda.synchronize()

    n_sa = property(lambda self: self._n_sa if self.tr is None else self.tr.n_sa)
    n_rt = property(lambda self: self._n_rt if self.tr is None else self.tr.n_rt)

    def set_halt(self, v):
        assert self.tr is None
        self.halt = None if v is None else torch.full((1,), int(v), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        self.L.check(self.lib.pdec_set_episode_halt(self.h, self.L.ptr(self.halt)))

    def close(self):
        torch.cuda.synchronize()
        self.L.check(self.lib.pdec_set_episode_halt(self.h, None))

    def _buf(self, x):
        """a device copy of x (never a null pointer: an empty push still names a buffer)"""
        x = np.asarray(x)
        if x.shape[0] == 0:
            x = np.zeros((1,) + x.shape[1:], dtype=x.dtype)
        return dev(x)

    def push_sa(self, s, a=None):
        n = s.shape[0]
        if self.tr is not None:
            return self.tr.push_sa(dev(s), None if a is None else dev(a))
        sd, ad = self._buf(s), (None if a is None else self._buf(a))
        P = self.L.ptr
        self.L.check(self.lib.pdec_replay_push_sa(self.h, P(self.traces["state"]), P(self.traces["action"]), self.cap1, self.row.ns,
                                                  self.row.na, self._n_sa % self.cap1, P(sd), P(ad), n, self.L.dtype_code(self.dt)))
        self._n_sa += n

    def pop_sa(self, n):
        if self.tr is not None:
            return self.tr.pop_sa(n)
        self._n_sa -= n

    def push_rt(self, r, flags, cols, force):
        n = r.shape[0]
        fd = None if flags is None else dev(flags)
        if self.tr is not None:
            return self.tr.push_rt_flags(dev(r), fd, cols, bool(force))
        rd = self._buf(r)
        P = self.L.ptr
        self.L.check(self.lib.pdec_replay_push_rt(self.h, P(self.traces["reward"]), P(self.traces["terminal"]), self.cap,
                                                  self._n_rt % self.cap, P(rd), P(fd), int(cols), int(force), n,
                                                  self.L.dtype_code(self.dt)))
        self._n_rt += n

    def image(self):
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.traces.items()}

    def sample(self, seed, offset, Bu, n_valid, with_slots):
        row, kw = self.row, dict(dtype=torch.float32, device="cuda:0")
        out = [torch.full((Bu, row.ns), 9.0, **kw), torch.full((Bu, row.na), 9.0, **kw), torch.full((Bu,), 9.0, **kw),
               torch.full((Bu,), 9.0, **kw), torch.full((Bu, row.ns), 9.0, **kw)]
        slots = torch.full((3, Bu), -1, dtype=torch.int32, device="cuda:0") if with_slots else None
        torch.cuda.synchronize()
        P, t = self.L.ptr, self.traces
        self.L.check(self.lib.pdec_replay_sample(self.h, P(t["state"]), P(t["action"]), P(t["reward"]), P(t["terminal"]), row.ns, row.na,
                                                 row.cap, row.stride, n_valid, self.n_rt, seed, offset, Bu, *(P(o) for o in out), P(slots)))
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in out], (None if slots is None else slots.cpu().numpy())


@pytest.mark.parametrize("name", list(rc.ROWS))
def test_pushes_leave_the_models_image_and_samples_fetch_its_batch(pkg, net, name):
    """every row: all four traces over their whole allocation == the model's image, the halt flag and the counters the model's;
    every sampling row: slots_out == oracle.rng.sample_slots, the five outputs == the logical entries lg and lg + stride, and the
    same outputs without slots_out"""
    row = rc.ROWS[name]
    m = rc.play(name, ref.Replay(row.ns, row.na))
    d = Driver(pkg, net, row)
    try:
        rc.play(name, d)
    finally:
        d.close()
    got, want = d.image(), m.image(row.cap, row.stride, init=rc.sentinel(row) if row.prefill else None)
    for k in TRACES:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (name, k)
    assert (d.n_sa, d.n_rt) == (m.n_sa, m.n_rt)
    assert (None if d.halt is None else int(d.halt.item())) == m.halt
    for seed, off, Bu in row.samples:
        nv = m.n_valid(row.cap)
        sl = orng.sample_slots(seed, off, Bu, nv, m.n_rt, row.cap, row.stride)
        out, slots = d.sample(seed, off, Bu, nv, True)
        assert np.array_equal(slots, sl), (name, seed, off, Bu)
        for key, a, b in zip(ref.BATCH_NAMES, out, m.batch(sl, row.cap, row.stride)):
            assert a.shape == b.shape and np.array_equal(a, b), (name, key, Bu)
        out2, none = d.sample(seed, off, Bu, nv, False)
        assert none is None
        for key, a, b in zip(ref.BATCH_NAMES, out, out2):
            assert np.array_equal(a, b), (name, key, "without slots_out")


def test_host_refusals_return_the_invalid_argument_code(pkg, net):
    """argument checks: PDEC_E_INVALID before anything is launched, nothing written; one step inside each bound is accepted"""
    L, lib, h, P = pkg._lib, net.lib, net.handle, pkg._lib.ptr
    kw = dict(dtype=torch.float32, device="cuda:0")

    def call(what, cap, n=1, stride=3, halt=False, n_valid=0, n_rt=0):
        cap1 = cap + stride
        tr = [torch.full((cap1, 1), 5.0, **kw), torch.full((cap1, 1), 5.0, **kw), torch.full((cap,), 5.0, **kw), torch.full((cap,), 5.0, **kw)]
        src = torch.ones((max(n, 4) * 4,), **kw)
        flag = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        if halt:
            L.check(lib.pdec_set_episode_halt(h, P(flag)))
        try:
            if what == "push_sa":
                code = lib.pdec_replay_push_sa(h, P(tr[0]), P(tr[1]), cap, 1, 1, 0, P(src), P(src), n, L.PDEC_F32)
            elif what == "push_rt":
                code = lib.pdec_replay_push_rt(h, P(tr[2]), P(tr[3]), cap, 0, P(src), None, 1, 0, n, L.PDEC_F32)
            else:
                out = [torch.zeros((4, 1), **kw) for _ in range(5)]
                code = lib.pdec_replay_sample(h, P(tr[0]), P(tr[1]), P(tr[2]), P(tr[3]), 1, 1, cap, stride, n_valid, n_rt, 1, 0, 4,
                                              P(out[0]), P(out[1]), P(out[2].view(-1)), P(out[3].view(-1)), P(out[4]), None)
        finally:
            torch.cuda.synchronize()
            L.check(lib.pdec_set_episode_halt(h, None))
        return code, [bool((t == 5.0).all()) for t in tr]

    for name, (what, args) in rc.REFUSALS.items():
        code, untouched = call(what, **args)
        assert code == rc.E_INVALID, (name, code)
        assert all(untouched), name
    for name, (what, args) in rc.ACCEPTED.items():
        code, _ = call(what, **args)
        assert code == 0, (name, code)


# --------------------------------------------------------------------------------------------------------------------
def _fill(tr, steps, extra, A, ns, g):
    """`steps` control steps, the next step's (s, a) and `extra` of its reward columns"""
    for _ in range(steps):
        tr.push_sa(torch.randn(A, ns, generator=g).cuda(), (torch.rand(A, 1, generator=g) * 2 - 1).cuda())
        tr.push_rt(-torch.rand(A, generator=g).cuda(), (torch.rand(A, generator=g) < 0.2).float().cuda())
    tr.push_sa(torch.randn(A, ns, generator=g).cuda(), (torch.rand(A, 1, generator=g) * 2 - 1).cuda())
    if extra:
        tr.push_rt(-torch.rand(extra, generator=g).cuda(), torch.zeros(extra).cuda())


@pytest.mark.parametrize("state", list(rc.SMALL_STATES))
@pytest.mark.parametrize("which", ["two_layer_register_kernel", "three_layer_generic_kernel"])
def test_in_kernel_sampler_at_the_ring_states(pkg, which, state):
    """pdec_ddpg_update_small_rng (the slot table of csrc/small_args.hpp) at the table's ring states: ONE update of SMALL_BU columns
    == pdec_ddpg_update_small fed the oracle's slots of the same stream, bit for bit"""
    setup = pkg.KSSetup.KS22() if which.startswith("two") else pkg.KSSetup.bench_C2(256)
    ns, A = setup.state_shape
    steps, extra, seed, off = rc.SMALL_STATES[state]
    agents = [pkg.create_agent(setup=setup, B=1, rng=np.random.default_rng(5), trajectory_length=rc.SMALL_STEPS_CAP * A,
                               batch_size=rc.SMALL_BU, update_loops=1) for _ in range(2)]
    g = torch.Generator()
    for ag in agents:
        g.manual_seed(3)
        _fill(ag.trajectory, steps, extra, A, ns, g)
    p0, p1 = agents[0].policy, agents[1].policy
    tr = agents[0].trajectory
    assert tr.capacity == rc.SMALL_STEPS_CAP * A and tr.n_rt == steps * A + extra and p0.small_update_ok()
    assert (p0.update_loops, p0.batch_size) == (1, rc.SMALL_BU)
    p0._sample_seed, p0._sample_off = seed, off
    p0.update_small_rng(tr)
    slots = orng.sample_slots(seed, off, rc.SMALL_BU, len(tr), tr.n_rt, tr.capacity, tr.stride)
    p1.update_small(agents[1].trajectory, slots.reshape(3, 1, rc.SMALL_BU))
    torch.cuda.synchronize()
    assert p0._sample_off == off + (rc.SMALL_BU + 3) // 4
    fresh = pkg.create_agent(setup=setup, B=1, rng=np.random.default_rng(5), trajectory_length=rc.SMALL_STEPS_CAP * A).policy
    assert not np.array_equal(fresh.behavior_critic.model.params()[0], p1.behavior_critic.model.params()[0])      # it did update
    for n in ("behavior_actor", "behavior_critic", "target_actor", "target_critic"):
        for x, y in zip(getattr(p0, n).model.params(), getattr(p1, n).model.params()):
            assert np.array_equal(x, y), (n, state)
    assert p0.losses() == p1.losses()


@pytest.mark.parametrize("lap", list(rc.GLUE_LAPS))
@pytest.mark.parametrize("case", rc.GLUE_CASES)
def test_step_glue_at_the_seams_equals_the_model(pkg, case, lap):
    """pdec_step_glue with the rings filled so that one launch writes the last A rows of a ring and the next starts at row 0 --
    both rings in the same launch on the first lap, one launch apart on the second -- against the MODEL: traces, halt flag,
    n_sa, n_rt and the noise offset.  The second launch is the one the case is about."""
    runmod, L = import_module(pkg.__name__ + ".run"), pkg._lib
    setup = pkg.KSSetup.KS22()
    ns, A = setup.state_shape
    pre, launches = rc.GLUE_LAPS[lap]
    agent = pkg.create_agent(setup=setup, B=1, rng=np.random.default_rng(5), trajectory_length=rc.GLUE_CAP)
    pol, tr = agent.policy, agent.trajectory
    assert (tr.capacity, tr.stride, A) == (rc.GLUE_CAP, 8, 8)
    m = ref.Replay(ns, 1)
    g = torch.Generator().manual_seed(11)
    for k in range(pre + 1):                       # `pre` full steps and the (s, a) of the step whose reward the first launch pushes
        s, a = torch.randn(A, ns, generator=g), torch.rand(A, 1, generator=g) * 2 - 1
        tr.push_sa(s.cuda(), a.cuda())
        m.push_sa(s.numpy(), a.numpy())
        if k < pre:
            r, f = -torch.rand(A, generator=g), torch.zeros(1, dtype=torch.int32)
            tr.push_rt_flags(r.cuda(), f.cuda(), A, False)
            m.push_rt(r.numpy(), f.numpy(), A, 0)
    first_rt, first_sa = tr.n_rt % tr.capacity, tr.n_sa % (tr.capacity + tr.stride)
    assert first_rt == tr.capacity - 2 * A              # launch 2 fills the last A rows of the reward ring
    assert first_sa == (tr.capacity + tr.stride - (2 if lap == "first_lap" else 3) * A)
    dt = torch.float64
    T = launches + 2
    logs = SimpleNamespace(state=torch.randn(T, A, ns, generator=g).to(dt).cuda(), action=torch.full((T + 1, A, 1), 7.0, dtype=dt).cuda(),
                           reward=-torch.rand(T, 1, A, generator=g).to(dt).cuda(), done=torch.zeros(T, dtype=torch.int32).cuda())
    halt = torch.zeros(1, dtype=torch.int32).cuda()
    if case == "episode_ends_here":
        logs.done[1] = 1                            # the step whose reward launch 2 pushes
    if case == "episode_ended_before":
        halt[0] = 1
    m.set_halt(int(halt.item()))
    pol._noise_seed, pol._noise_off = 99, 5
    acting = case != "zero_policy"
    lib = pol.behavior_actor.model.lib
    torch.cuda.synchronize()
    L.check(lib.pdec_set_episode_halt(tr._h, L.ptr(halt)))
    try:
        pol._glue_off = False
        for t in range(1, launches + 1):
            assert runmod._step_glue(lib, pol, tr, SimpleNamespace(dtype=dt), logs, t, A, A, acting, True)
    finally:
        torch.cuda.synchronize()
        L.check(lib.pdec_set_episode_halt(tr._h, None))
    acts, states = logs.action.cpu().numpy(), logs.state.cpu().numpy()
    rew, done = logs.reward.cpu().numpy(), logs.done.cpu().numpy()
    for t in range(1, launches + 1):
        m.push_rt(rew[t - 1].reshape(-1), done[t - 1:t], A, 0)
        if acting:
            m.push_sa(states[t], acts[t + 1])
        else:
            assert np.all(acts[t + 1] == 0)
            m.push_sa(states[t], np.zeros((A, 1)))
    if acting and case != "episode_ended_before":
        assert all(0 < np.abs(acts[t + 1]).max() <= pol.act_limit and not np.any(acts[t + 1] == 7.0) for t in range(1, launches + 1))
    want = m.image(tr.capacity, tr.stride)
    for k in TRACES:
        assert np.array_equal(getattr(tr, k).cpu().numpy(), want[k]), (case, lap, k)
    assert int(halt.item()) == m.halt == (1 if case.startswith("episode_end") else 0)
    assert (tr.n_sa, tr.n_rt) == (m.n_sa, m.n_rt)
    assert pol._noise_off == 5 + (launches * ((A + 3) // 4) if acting else 0)
    # the launches did reach the seams: the model's pushes start where the docstring says
    if case in ("mid_episode", "zero_policy"):
        cap, cap1 = tr.capacity, tr.capacity + tr.stride
        rt_rows = [f % cap for f, _ in m.pushes["rt"][-launches:]]
        sa_rows = [f % cap1 for f, _ in m.pushes["sa"][-launches:]]
        assert rt_rows[:3] == [cap - 2 * A, cap - A, 0]
        assert sa_rows == ([cap1 - 2 * A, cap1 - A, 0] if lap == "first_lap" else [cap1 - 3 * A, cap1 - 2 * A, cap1 - A, 0])


# --------------------------------------------------------------------------------------------------------------------
def _plant(reward):
    """NaN, +Inf, -Inf and a finite value into every row of a [B, len] reward array, rotating (len 1: one kind per row)"""
    kinds = [np.nan, np.inf, -np.inf, None]
    B, n = reward.shape
    for b in range(B):
        for j in range(min(n, 4)):
            v = kinds[(b + j) % 4]
            if v is not None:
                reward[b, j] = v
    return reward


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("B", rc.RESET_B)
@pytest.mark.parametrize("geometry", rc.RESET_GEOMETRIES)
def test_same_step_reset_touches_done_rows_only(pkg, geometry, B, prec):
    """pdec_env_autoreset called directly: done rows of y / state / action bit-equal to their images, every other row bit-equal
    to what it held (its NaN / Inf rewards included), in done rows non-finite rewards 0 and finite ones untouched, buffers
    passed as NULL untouched -- for done patterns none / all / one in the middle / first with last, with and without the
    state and action pairs"""
    import ks_geometry_cases as kc
    from oracle import ks
    case = kc.CASES[geometry]
    setup, _ = kc.build(pkg, ks, geometry)
    dt = torch.float64 if prec == "f64" else torch.float32
    env = pkg.PDEenv(setup, B=B, dtype=dt, autoreset=False)
    L, lib, P = pkg._lib, env.lib, pkg._lib.ptr
    A, S = kc.n_actuators(case), len(case.sensor_positions)
    nsx = S if case.mono else case.window_size * case.temporal_steps
    cols = 1 if case.mono else A
    # the buffers are as large as the kernel's rows (pdec_env_autoreset: N | mono ? S : A ns | A na | mono ? 1 : A)
    assert env.y[0].numel() == case.nx and env.state[0].numel() == (S if case.mono else A * nsx)
    assert env.action[0].numel() == A and env.reward[0].numel() == cols
    rng = np.random.default_rng([B, case.nx, int(prec == "f64")])
    npdt = np.float64 if prec == "f64" else np.float32
    draw = lambda t: rng.standard_normal(tuple(t.shape)).astype(npdt)
    for done in rc.done_patterns(B):
        for with_state in (True, False):
            for with_action in (True, False):
                h = {k: draw(t) for k, t in (("y", env.y), ("y0", env.y), ("state", env.state), ("state0", env.state),
                                             ("action", env.action), ("action0", env.action))}
                h["reward"] = _plant(draw(env.reward))
                d = {k: dev(v) for k, v in h.items()}
                flags = dev(np.array(done, dtype=np.int32))
                torch.cuda.synchronize()
                L.check(lib.pdec_env_autoreset(env.handle, P(flags), P(d["y"]), P(d["y0"]), P(d["state"]) if with_state else None,
                                               P(d["state0"]) if with_state else None, P(d["action"]) if with_action else None,
                                               P(d["action0"]) if with_action else None, P(d["reward"])))
                torch.cuda.synchronize()
                got = {k: v.cpu().numpy() for k, v in d.items()}
                tag = (geometry, B, prec, done, with_state, with_action)
                for k in ("y0", "state0", "action0"):
                    assert same_bits(got[k], h[k]), tag + (k,)
                for b in range(B):
                    for k, on in (("y", True), ("state", with_state), ("action", with_action)):
                        want = h[k + "0"][b] if (done[b] and on) else h[k][b]
                        assert same_bits(got[k][b], want), tag + (k, b)
                    r0, r1 = h["reward"][b], got["reward"][b]
                    if done[b]:
                        fin = np.isfinite(r0)
                        assert np.all(r1[~fin] == 0) and not np.any(np.signbit(r1[~fin])) and same_bits(r1[fin], r0[fin]), tag + (b,)
                    else:
                        assert same_bits(r1, r0), tag + ("reward", b)
    # reward == NULL: the three pairs as before, the reward array untouched
    h = {k: draw(t) for k, t in (("y", env.y), ("y0", env.y))}
    d = {k: dev(v) for k, v in h.items()}
    flags = dev(np.ones(B, dtype=np.int32))
    torch.cuda.synchronize()
    L.check(lib.pdec_env_autoreset(env.handle, P(flags), P(d["y"]), P(d["y0"]), None, None, None, None, None))
    torch.cuda.synchronize()
    assert same_bits(d["y"].cpu().numpy(), h["y0"])
