"""The deferred actor finish (include/pdeconv.h, pdec_ddpg_defer_actor_finish; pipeline.py): with frozen targets the finish
launch of the actor half of update k -- slab reduction, ADAM, image refresh -- is issued as extra blocks of the critic's finish
launch of update k + 1.  Pure scheduling: every buffer the four-launch sequence leaves must be left byte for byte.

Native: two net pairs (critic tiles 9 / actor tiles 2, and 2 / 1) at the batch sizes that give 1, 2, 16, 17, 256 and 257 gradient
slabs of 128 columns -- one slab with dead columns, both sides of the 16 slab groups of the reduction and of its unrolled round of
256 slabs.  Pipeline: KS bench_C2(256) with B = 2 and 3 (128 and 192 columns) and episodes of four steps, run(5); run(6)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NETS = {"9x2": ([3, 16, 16, 1], [4, 140, 140, 1]), "2x1": ([1, 5, 5, 1], [2, 16, 16, 1])}
BATCHES = [1, 129, 2048, 2049, 32768, 32769]          # ceil(Bu / 128) = 1, 2, 16, 17, 256, 257 slabs
UPDATES = 4


def _nets(pkg, which, Bu):
    """behaviour actor, behaviour critic, target actor, target critic from one seed"""
    da, dc = NETS[which]
    rng = np.random.default_rng(5)
    out = []
    for dims, last in ((da, "tanh"), (dc, None), (da, "tanh"), (dc, None)):
        P = []
        for i, o in zip(dims[:-1], dims[1:]):
            P += [rng.uniform(-1, 1, (o, i)) * np.sqrt(6.0 / (i + o)), rng.standard_normal(o) * 0.1]
        out.append(pkg.HipMLP(dims, ["relu", "relu", last], P, dtype=torch.float32, max_cols=Bu))
    return out


def _batch(which, Bu):
    ns = NETS[which][0][0]
    g = torch.Generator().manual_seed(100 + Bu)
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32).to("cuda:0")
    t = (torch.rand(Bu, generator=g) < 0.1).to(torch.float32).to("cuda:0")
    return rnd(Bu, ns), torch.tanh(rnd(Bu, 1)), rnd(Bu), t, rnd(Bu, ns)


def _debug(pkg, net, which=0, image=False):
    """(image or None, pub, pending, paired) of pdec_debug_fused_image"""
    n, pub, pending, paired = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    refs = (C.byref(n), C.byref(pub), C.byref(pending), C.byref(paired))
    pkg._lib.check(net.lib.pdec_debug_fused_image(net.handle, which, None, *refs))
    img = None
    if image:
        img = np.empty(n.value, dtype=np.float32)
        pkg._lib.check(net.lib.pdec_debug_fused_image(net.handle, which, img.ctypes.data_as(C.c_void_p), *refs))
    return img, pub.value, pending.value, paired.value


def _state(pkg, nets, losses):
    """everything the update leaves, as bytes"""
    torch.cuda.synchronize()
    out = {"losses": losses.cpu().numpy().tobytes()}
    for name, net in zip(("A", "C", "At", "Ct"), nets):
        out[name + ".params"] = b"".join(np.ascontiguousarray(p).tobytes() for p in net.params())
    for name, net in zip(("A", "C"), nets[:2]):
        m, v, bp = pkg.checkpoint._adam_state(net)
        out[name + ".adam"] = m.tobytes() + v.tobytes() + bp.tobytes()
        ptr, n = net.grad_buffer()
        out[name + ".grads"] = torch.as_tensor(pkg.distributed._DevArray(ptr, n, "<f4"), device="cuda:0").cpu().numpy().tobytes()
        for w in range(3):
            out[f"{name}.image{w}"] = _debug(pkg, net, w, image=True)[0].tobytes()
        out[name + ".pub"] = _debug(pkg, net)[1]
    return out


def _updates(pkg, which, Bu, arm, rho):
    """UPDATES critic / actor halves, armed or not -> (state, armed as reported, paired launches, nets, losses)"""
    L, P_ = pkg._lib, pkg._lib.ptr
    nets = A, Cn, At, Ct = _nets(pkg, which, Bu)
    s, a, r, t, sn = _batch(which, Bu)
    losses = torch.zeros(2, dtype=torch.float32, device="cuda:0")
    lp = C.c_void_p(losses.data_ptr())
    armed = C.c_int(-1)
    if arm:
        L.check(A.lib.pdec_ddpg_defer_actor_finish(A.handle, 1, rho, C.byref(armed)))
    for u in range(UPDATES):
        L.check(A.lib.pdec_ddpg_update_critic_async(A.handle, Cn.handle, At.handle, Ct.handle, P_(s), P_(a), P_(r), P_(t), P_(sn), Bu,
                                                    0.99, rho, 1, 1e-3, lp))
        assert _debug(pkg, A)[2] == 0                     # the critic's finish launch took a pending finish along
        L.check(A.lib.pdec_ddpg_update_actor_async(A.handle, Cn.handle, At.handle, Ct.handle, P_(s), Bu, rho, 5e-4, lp))
        assert _debug(pkg, A)[2] == (1 if arm and armed.value == 1 else 0)
    if arm and armed.value == 1:
        # what a pending finish has yet to write is not handed out: acting is refused, by name
        out = torch.zeros(4, dtype=torch.float32, device="cuda:0")
        with pytest.raises(pkg.PdecError, match="pending"):
            L.check(A.lib.pdec_policy_act_rng(A.handle, P_(s), 1, 0.1, 1.0, 1, 7, 0, P_(out)))
    L.check(A.lib.pdec_ddpg_flush_actor_finish(A.handle))
    assert _debug(pkg, A)[2] == 0
    return _state(pkg, nets, losses), armed.value, _debug(pkg, A)[3], nets, losses


def _assert_same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], (what, k)


@pytest.mark.parametrize("Bu", BATCHES)
@pytest.mark.parametrize("which", list(NETS))
def test_armed_updates_leave_the_bytes_of_the_four_launch_sequence(pkg, which, Bu):
    want, _, paired0, _, _ = _updates(pkg, which, Bu, False, 1.0)
    got, armed, paired, nets, losses = _updates(pkg, which, Bu, True, 1.0)
    assert armed == 1 and paired0 == 0 and paired == UPDATES - 1       # updates 2 .. 4 carried the finish of the one before
    assert np.isfinite(np.frombuffer(want["losses"], dtype=np.float32)).all()
    fresh = b"".join(np.ascontiguousarray(p).tobytes() for p in _nets(pkg, which, Bu)[0].params())
    assert len(fresh) == len(want["A.params"]) and fresh != want["A.params"]               # (the updates moved the actor)
    _assert_same(got, want, "armed")
    # nothing is pending: a second flush, and switching the deferral off, change nothing
    A = nets[0]
    pkg._lib.check(A.lib.pdec_ddpg_flush_actor_finish(A.handle))
    pkg._lib.check(A.lib.pdec_ddpg_flush_actor_finish(A.handle))
    off = C.c_int(-1)
    pkg._lib.check(A.lib.pdec_ddpg_defer_actor_finish(A.handle, 0, 1.0, C.byref(off)))
    assert off.value == 0
    _assert_same(_state(pkg, nets, losses), want, "flushed twice and disarmed")


@pytest.mark.parametrize("which", list(NETS))
def test_moving_targets_decline_the_deferral(pkg, which):
    """rho = 0.995: the critic pass reads the target actor that the actor's finish writes -- not armed, the plain sequence"""
    Bu = 129
    want, _, _, _, _ = _updates(pkg, which, Bu, False, 0.995)
    got, armed, paired, _, _ = _updates(pkg, which, Bu, True, 0.995)
    assert armed == 0 and paired == 0
    _assert_same(got, want, "rho = 0.995")
    assert want["At.params"] != _updates(pkg, which, Bu, False, 1.0)[0]["At.params"]       # (and the targets do move there)


# ------------------------------------------------------------------ the training pipeline
def _pipe(pkg, B):
    setup = pkg.KSSetup.bench_C2(256)
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    y0 = setup.generate_random_init(np.random.default_rng(0), B) * 0.15
    env = pkg.PDEenv(setup, B=B, dtype=torch.float32, y0=y0, stream=s_env, autoreset=False)
    agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                             noise_seed=7, trajectory_length=1)
    agent.policy.act_noise = 0.3
    torch.cuda.synchronize()
    return pkg.TrainPipeline(env, agent, lag=2, episode_steps=4, stream_env=s_env, stream_upd=s_upd, use_graphs=False,
                             noise_seed=99)


def _pipe_state(pkg, p):
    p.sync()
    torch.cuda.synchronize()
    out = {"y": p.y, "state": p.state, "losses": p.policy.losses()}
    for ring in ("aring", "rring", "tring"):
        for i, x in enumerate(getattr(p, ring)):
            out[f"{ring}{i}"] = x
    out = {k: (v.cpu().numpy().tobytes() if torch.is_tensor(v) else v) for k, v in out.items()}
    for nm in ("behavior_actor", "behavior_critic", "target_actor", "target_critic"):
        out[nm] = b"".join(np.ascontiguousarray(x).tobytes() for x in getattr(p.policy, nm).model.params())
    return out


@pytest.mark.parametrize("B", [2, 3])
def test_pipeline_with_the_deferred_finish_is_the_four_launch_pipeline(pkg, monkeypatch, B):
    monkeypatch.setenv("PDEC_DEFER_ACTOR_FINISH", "0")
    plain = _pipe(pkg, B)
    monkeypatch.delenv("PDEC_DEFER_ACTOR_FINISH")
    deferred, drained = _pipe(pkg, B), _pipe(pkg, B)
    assert not plain.defer_actor_finish and deferred.defer_actor_finish and drained.defer_actor_finish
    drained.drain_between = True                  # the device drained behind every act and every env step: no timing left
    states = []
    for p in (plain, deferred, drained):
        p.run(5)
        p.run(6)
        assert not p._pending and not p._armed       # outside run() nothing is pending
        states.append(_pipe_state(pkg, p))
    A = lambda p: p.policy.behavior_actor.model
    # updates at steps 2 .. 10; the first of each run() finds nothing pending, the other seven pair
    assert _debug(pkg, A(plain))[3] == 0 and _debug(pkg, A(deferred))[3] == 7 == _debug(pkg, A(drained))[3]
    assert deferred._progs and not drained._progs
    assert np.isfinite(np.frombuffer(states[0]["y"], dtype=np.float32)).all() and all(np.isfinite(states[0]["losses"]))
    _assert_same(states[1], states[0], "deferred")
    _assert_same(states[2], states[0], "deferred, drained")
    for p in (plain, deferred, drained):
        p.close()
