"""Reward groups (include/pdeconv.h, pdec_ddpg_set_reward_groups): the reference's reward broadcast per group of g columns
instead of over the whole update batch.  Critic gradients and losses of every critic path against the fp64 restatement
tests/reward_group_ref.py; the routing identities (g = 1 is the diagonal target, g L >= Bu the whole-batch broadcast, bit
for bit); the refused shapes; the small update's route; what the gradient does when rewards move within and across groups;
and the training pipeline with groups, graphs against eager.

Tolerances as tests/test_gpu_grads.py: fp32 gradients <= 1e-4 of each parameter array's largest entry, the norms to 1e-4,
the loss to 2e-5 relative."""
import ctypes as C

import numpy as np
import pytest

from reward_group_ref import critic_grad_of_dq, group_index, group_members, grouped_losses_and_grads
from test_gpu_grads import TOL, _away_from_relu_kinks, _inputs, assert_arrays_close, flat_of, read_grads
from test_gpu_mlp import make_net
from util import to_dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# path -> (actor (ns, scale, drop), critic (scale, drop), dtype): the four critic paths
PATHS = {
    "fused3": ((3, 1.6, False), (7.0, False), torch.float32),      # 4->140->140->1: ddpg_critic_fused_kernel
    "fused2": ((9, 1.8, True), (17.0, True), torch.float32),       # 10->340->1: ddpg2 passes (fluid shape)
    "generic32": ((3, 1.6, False), (7.0, True), torch.float32),    # 3-layer actor + 2-layer critic: no fused pair
    "generic64": ((3, 1.6, False), (7.0, False), torch.float64),   # fp64 environments
}
G32 = np.float64(np.float32(0.99))


class Problem:
    def __init__(self, pkg, path, Bu, seed):
        from oracle import nn
        (ns, sa, drop_a), (sc, drop_c), dtype = PATHS[path]
        rng = np.random.default_rng(seed)
        da, self.aa = nn.layer_sizes(ns, 1, sa, True, drop_a)
        dc, self.ac = nn.layer_sizes(ns, 1, sc, False, drop_c)
        self.dtype, self.Bu, self.ns, self.pkg = dtype, Bu, ns, pkg
        self.A, PA = make_net(pkg, rng, da, self.aa, dtype, Bu)
        self.C, PC = make_net(pkg, rng, dc, self.ac, dtype, Bu)
        self.At, PAt = make_net(pkg, rng, da, self.aa, dtype, Bu)
        self.Ct, PCt = make_net(pkg, rng, dc, self.ac, dtype, Bu)
        s, a, r, t, sn = _inputs(rng, ns, Bu)
        if dtype == torch.float32:
            s, a, r, t, sn, _ = _away_from_relu_kinks(nn, PA, PC, self.aa, self.ac, s, a, r, t, sn)
        self.host = (s, a, r, t, sn)
        f64 = lambda P: [p.astype(np.float64) for p in P]
        self.P64 = (f64(PA), f64(PC), f64(PAt), f64(PCt))
        self.dev = [to_dev(s.T, dtype), to_dev(a.T, dtype), to_dev(r, dtype), to_dev(t, dtype), to_dev(sn.T, dtype)]
        self.losses = torch.zeros(2, dtype=dtype, device="cuda:0")

    def set_groups(self, g, L=1):
        self.pkg._lib.check(self.C.lib.pdec_ddpg_set_reward_groups(self.C.handle, g, L))

    def set_reward(self, r):
        self.dev[2] = to_dev(np.asarray(r, dtype=np.float32), self.dtype)

    def critic_grads(self, quirk=1, grad_scale=1.0):
        """-> (flat critic gradient fp64, critic loss)"""
        L = self.pkg._lib
        ds, da, dr, dt, dsn = self.dev
        L.check(self.A.lib.pdec_ddpg_critic_grads(self.A.handle, self.C.handle, self.At.handle, self.Ct.handle, L.ptr(ds), L.ptr(da),
                                                  L.ptr(dr), L.ptr(dt), L.ptr(dsn), self.Bu, 0.99, quirk, grad_scale,
                                                  C.c_void_p(self.losses.data_ptr())))
        if self.dtype == torch.float32:
            g = read_grads(self.pkg, self.C)
        else:                                   # (read_grads reads fp32 buffers)
            ptr, n = self.C.grad_buffer()
            torch.cuda.synchronize()
            g = torch.as_tensor(self.pkg.distributed._DevArray(ptr, n, "<f8"), device="cuda:0").cpu().numpy()
        return g, float(self.losses[0].cpu())

    def reference(self, g, L, r=None):
        s, a, r0, t, sn = (x.astype(np.float64) for x in self.host)
        r = r0 if r is None else np.asarray(r, dtype=np.float64)
        A, Cn, At, Ct = self.P64
        return grouped_losses_and_grads(A, Cn, At, Ct, self.aa, self.ac, s, a, r, t, sn, G32, g, L)


# (path, Bu, g, L): g in {2, 3, 8}, L in {1, A}; Bu from a few hundred to 32 768 (C2: 510 x 64 columns for g = 3)
CASES = [("fused3", 384, 3, 1), ("fused3", 32640, 3, 64), ("fused3", 4096, 8, 64), ("fused3", 1024, 2, 1), ("fused3", 32768, 2, 64),
         ("fused2", 300, 3, 1), ("fused2", 4096, 2, 16), ("fused2", 2048, 8, 1), ("fused2", 9216, 3, 64),
         ("generic32", 960, 3, 8), ("generic32", 512, 2, 1), ("generic32", 768, 8, 1),
         ("generic64", 600, 3, 4), ("generic64", 512, 8, 8), ("generic64", 256, 2, 1)]


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("path,Bu,g,L", CASES)
def test_grouped_critic_gradient_matches_the_restatement(pkg, path, Bu, g, L, grad_scale):
    pb = Problem(pkg, path, Bu, 300 + Bu % 89 + g + L)
    pb.set_groups(g, L)
    got, loss = pb.critic_grads(1, grad_scale)
    want = pb.reference(g, L)
    assert np.isfinite(got).all()
    assert_arrays_close(got, [grad_scale * x for x in want["gC"]], f"critic gradient {path} Bu={Bu} g={g} L={L}")
    assert abs(np.linalg.norm(got) / np.linalg.norm(grad_scale * flat_of(want["gC"])) - 1.0) <= TOL
    assert abs(loss - want["critic_loss"]) <= 2e-5 * max(1.0, abs(want["critic_loss"]))
    # the update entry point (critic half, fused with ADAM where the path has it) reports the same loss
    lu = torch.zeros(2, dtype=pb.dtype, device="cuda:0")
    P_ = pkg._lib.ptr
    ds, da, dr, dt, dsn = pb.dev
    pkg._lib.check(pb.A.lib.pdec_ddpg_update_critic_async(pb.A.handle, pb.C.handle, pb.At.handle, pb.Ct.handle, P_(ds), P_(da), P_(dr),
                                                          P_(dt), P_(dsn), Bu, 0.99, 1.0, 1, 0.0, C.c_void_p(lu.data_ptr())))
    assert abs(float(lu[0].cpu()) - want["critic_loss"]) <= 2e-5 * max(1.0, abs(want["critic_loss"]))


@pytest.mark.parametrize("path", list(PATHS))
def test_routing_identities_are_bit_exact(pkg, path):
    """g = 1 runs the diagonal pass and g L >= Bu the whole-batch pass, unchanged; switching the groups off restores the
    whole-batch broadcast"""
    Bu = 768
    pb = Problem(pkg, path, Bu, 11)
    diag, l_diag = pb.critic_grads(quirk=0)
    whole, l_whole = pb.critic_grads(quirk=1)
    assert not np.array_equal(diag, whole)
    pb.set_groups(1, 1)
    g1, l1 = pb.critic_grads(quirk=1)
    assert np.array_equal(g1, diag) and l1 == l_diag
    pb.set_groups(1, 64)
    g1, l1 = pb.critic_grads(quirk=1)
    assert np.array_equal(g1, diag) and l1 == l_diag
    for g, L in ((Bu, 1), (3, Bu // 3), (2, 1000), (Bu + 5, 1)):        # one group spans the batch (or more than it)
        pb.set_groups(g, L)
        gw, lw = pb.critic_grads(quirk=1)
        assert np.array_equal(gw, whole) and lw == l_whole, (g, L)
    pb.set_groups(3, 1)
    gg, _ = pb.critic_grads(quirk=1)
    assert not np.array_equal(gg, whole) and not np.array_equal(gg, diag)
    gq0, lq0 = pb.critic_grads(quirk=0)                 # the groups refine the broadcast only: the diagonal target ignores them
    assert np.array_equal(gq0, diag) and lq0 == l_diag
    pb.set_groups(0, 1)
    g0, l0 = pb.critic_grads(quirk=1)
    assert np.array_equal(g0, whole) and l0 == l_whole


def test_shapes_the_groups_do_not_tile_are_refused(pkg):
    pb = Problem(pkg, "fused3", 384, 3)
    for g, L in ((5, 1), (3, 7), (7, 8)):
        pb.set_groups(g, L)
        with pytest.raises(pkg.PdecError, match="reward groups"):
            pb.critic_grads(quirk=1)
    with pytest.raises(pkg.PdecError):
        pkg._lib.check(pb.C.lib.pdec_ddpg_set_reward_groups(pb.C.handle, -1, 1))
    with pytest.raises(pkg.PdecError):
        pkg._lib.check(pb.C.lib.pdec_ddpg_set_reward_groups(pb.C.handle, 3, 0))
    setup = pkg.KSSetup.bench_C2(256)
    with pytest.raises(ValueError):
        pkg.create_agent(setup=setup, B=3, device="cuda:0", quirk_target_broadcast=False, target_broadcast_group=3)
    with pytest.raises(ValueError):
        pkg.create_agent(setup=setup, B=3, device="cuda:0", target_broadcast_group="batch")
    ag = pkg.create_agent(setup=setup, B=3, device="cuda:0", target_broadcast_group="setup")
    assert ag.policy.reward_group == setup.batch_size


def test_small_update_route_reports_the_batched_fallback(pkg):
    """KS22 shapes, minibatch 3 from the replay (L = 1): groups that split the minibatch have no small kernel -- the query
    names the batched path, the small call refuses, the agent takes the batched update; g >= 3 keeps the kernel as it is
    and g = 1 is the diagonal target, bit for bit"""
    from test_gpu_small_update import S2F, Rig
    L = pkg._lib

    def rig_with(g):
        rg = Rig(pkg, "ks22_frozen")
        L.check(rg.nets[1].lib.pdec_ddpg_set_reward_groups(rg.nets[1].handle, g, 1))
        return rg

    for g in (0, 1, 3, 8):
        rg = rig_with(g)
        assert rg.kernel(2)[0] == S2F, g
        rg.close()
    rg = rig_with(2)
    assert rg.kernel(2) == ("generic_path/reward_groups", 0) and rg.kernel(2, True) == ("generic_path/reward_groups", 0)
    with pytest.raises(pkg.PdecError, match="reward groups"):
        rg.launch(rg.slots(2), 1)
    rg.launch(rg.slots(2), 0)                    # the diagonal target does not read the groups: served
    rg.close()
    ra, rb = rig_with(1), rig_with(0)
    sl = ra.slots(2)
    ra.launch(sl, 1)
    rb.launch(sl, 0)
    torch.cuda.synchronize()
    for x, y in zip(ra.nets, rb.nets):
        for p, q in zip(x.params(), y.params()):
            assert np.array_equal(p, q)
    assert torch.equal(ra.losses, rb.losses)
    ra.close(); rb.close()
    setup = pkg.KSSetup.KS22()
    assert not pkg.create_agent(setup=setup, B=1, device="cuda:0", target_broadcast_group=2).policy.small_update_ok()
    for g in (1, 3, None):
        assert pkg.create_agent(setup=setup, B=1, device="cuda:0", target_broadcast_group=g).policy.small_update_ok()


@pytest.mark.parametrize("path,L", [("fused3", 1), ("fused3", 64), ("fused2", 16), ("generic64", 8)])
def test_rewards_act_through_their_own_group_only(pkg, path, L):
    """permuting rewards inside every group leaves the gradient as it was (to rounding); moving one reward into another
    group changes it by exactly -(2 / Bu) (change of the group means) pushed through the critic; in the whole-batch mode
    neither changes anything beyond rounding"""
    g, Bu = 3, 1536
    pb = Problem(pkg, path, Bu, 21 + L)
    s, a, r, t, sn = pb.host
    r = r.astype(np.float64)
    r[5 * L] = -40.0                                 # one large reward (column 5 L), to be moved within and across groups
    pb.set_reward(r)
    pb.set_groups(g, L)
    base, _ = pb.critic_grads()
    scale = np.abs(base).max()
    rng = np.random.default_rng(5)
    perm = np.arange(Bu)
    for cols in group_members(Bu, g, L):
        perm[cols] = cols[rng.permutation(g)]
    pb.set_reward(r[perm])
    within, _ = pb.critic_grads()
    assert np.abs(within - base).max() <= 1e-5 * scale
    # move the large reward across: swap it with a column of another group
    i = 5 * L
    j = i + g * L if (i // (g * L)) == 0 else i - g * L
    j = j + 1 if group_index(Bu, g, L)[j] == group_index(Bu, g, L)[i] else j
    assert group_index(Bu, g, L)[j] != group_index(Bu, g, L)[i]
    r2 = r.copy()
    r2[i], r2[j] = r[j], r[i]
    pb.set_reward(r2)
    moved, _ = pb.critic_grads()
    ref0, ref1 = pb.reference(g, L, r), pb.reference(g, L, r2)
    s64, a64 = s.astype(np.float64), a.astype(np.float64)
    delta = flat_of(critic_grad_of_dq(pb.P64[1], pb.ac, s64, a64, ref1["dq"] - ref0["dq"]))
    assert np.abs(delta).max() >= 1e-3 * scale      # a visible change
    assert np.abs((moved - base) - delta).max() <= 2e-3 * np.abs(delta).max()
    # whole batch: the same two moves change nothing beyond rounding
    pb.set_groups(0, 1)
    pb.set_reward(r)
    w0, _ = pb.critic_grads()
    pb.set_reward(r[perm])
    w1, _ = pb.critic_grads()
    pb.set_reward(r2)
    w2, _ = pb.critic_grads()
    sw = np.abs(w0).max()
    assert np.abs(w1 - w0).max() <= 1e-5 * sw and np.abs(w2 - w0).max() <= 1e-5 * sw


def _pipeline(pkg, use_graphs, group, B=63, E=17):
    setup = pkg.KSSetup.bench_C2(256)
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    y0 = setup.generate_random_init(np.random.default_rng(0), B) * 0.15
    env = pkg.PDEenv(setup, B=B, dtype=torch.float32, y0=y0, stream=s_env, autoreset=False)
    agent = pkg.create_agent(setup=setup, B=B, rng=np.random.default_rng(1), dtype=torch.float32, stream=s_upd, start_steps=-1,
                             noise_seed=7, trajectory_length=1, target_broadcast_group=group)
    agent.policy.act_noise = 0.3
    torch.cuda.synchronize()
    return pkg.TrainPipeline(env, agent, lag=2, episode_steps=E, stream_env=s_env, stream_upd=s_upd, use_graphs=use_graphs,
                             chunks=(6, 1), noise_seed=99)


def test_grouped_pipeline_graphs_are_bit_identical_to_eager(pkg):
    """TrainPipeline with g = 3 (L = A: actuator a of three consecutive trajectories): captured graphs against the eager
    pipeline over 60 steps of 17-step episodes -- identical fields, actions and networks; the whole-batch hand-overs are
    off and the critics differ from the whole-batch pipeline's"""
    pe = _pipeline(pkg, False, 3)
    pg = _pipeline(pkg, True, 3)
    assert not pe.pre_rbar and pe.rpart is None and pe.reward_interleave == 64
    pg.run(5)
    pg.capture()
    n0 = pg.tick
    pe.run(n0)
    for n in (1, 7, 20, 32):
        pe.run(n)
        pg.run(n)
    pe.sync(); pg.sync()
    assert pe.tick == pg.tick >= 60 and pg.n_graph_launches > 0
    assert torch.equal(pe.y, pg.y) and torch.equal(pe.state, pg.state) and bool(torch.isfinite(pg.y).all())
    for k in range(3):
        assert torch.equal(pe.aring[k], pg.aring[k]) and torch.equal(pe.rring[k], pg.rring[k])
    for n in ("behavior_actor", "behavior_critic", "target_actor", "target_critic"):
        for x, y in zip(getattr(pe.policy, n).model.params(), getattr(pg.policy, n).model.params()):
            assert np.array_equal(x, y), n
    assert pe.policy.losses() == pg.policy.losses()
    pw = _pipeline(pkg, False, None)
    pw.run(pe.tick)
    pw.sync()
    assert pw.pre_rbar
    diff = max(np.abs(x - y).max() for x, y in zip(pw.policy.behavior_critic.model.params(), pe.policy.behavior_critic.model.params()))
    assert diff > 0
    for p in (pe, pg, pw):
        p.close()
