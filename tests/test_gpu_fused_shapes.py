"""Every instantiation of the fused MFMA DDPG passes at its width, row and batch edges, against the fp64 oracle.

The passes are templates over padded tile counts (csrc/mlp_mfma.hip with fused3_*.hpp, csrc/mlp_mfma2.hip with fused2_*.hpp); a shape inside a tile is served by
zero padding, and the lines that pad are only exercised where a shape sits ON a tile edge.  The rows of fused_shape_cases.CASES
sit on those edges; each names the instantiation it must reach, asserted through pdec_debug_batched_update_route BEFORE anything is
launched, and together they reach every name the dispatch can produce (test_fused_shape_table.py, on the CPU).  Per row and target
form (quirk 1 | 0):
  1. gradients     pdec_ddpg_critic_grads / pdec_ddpg_actor_grads: every gradient array, both losses and the norm ratio against
                   the fp64 oracle -- the assertions and tolerances of test_gpu_grads.py (1e-4 of each array's largest entry)
  2. three updates pdec_ddpg_update_async == the split sequence, bit for bit, and both within 2e-4 of oracle.nn.ddpg_update
  3. acting        pdec_policy_act_rng after the updates against the fp64 forward of the parameters READ BACK from the actor
                   (1e-5: the update's own error stays out), and far from the actions of the initial parameters
  4. pad hygiene   the gradients behind an update on a LARGER batch (stale slabs, scratch and staging images) are bit-identical to
                   those of fresh handles
The rows one step outside each predicate must report "generic" and pass 1 - 2 all the same."""
import ctypes as C
import zlib

import numpy as np
import pytest

import fused_shape_cases as fc
from test_gpu_grads import TOL, _away_from_relu_kinks, _inputs, assert_arrays_close, flat_of, read_grads
from test_gpu_mlp import make_net, relerr
from util import to_dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GAMMA, RHO, ETA_A, ETA_C = 0.99, 0.995, 5e-4, 1e-3
CRITIC_GRADS, ACTOR_GRADS, UPDATE_CRITIC, UPDATE_ACTOR, ACT = range(5)
f64 = lambda P: [p.astype(np.float64) for p in P]


def rows(names):
    """parametrize arguments; the rows of 32 768 columns and more (about 20 s of fp64 oracle together) carry the slow mark"""
    return [pytest.param(c, marks=pytest.mark.slow) if fc.CASES[c][4] >= 32768 else c for c in names]


class Rig:
    """the four networks of a row (one or more identical sets of handles) and the library around them"""

    def __init__(self, pkg, case, quirk, sets=1, max_cols=None):
        from oracle import nn
        self.pkg, self.L, self.nn, self.case, self.quirk = pkg, pkg._lib, nn, case, quirk
        layers, self.ns, _, _, self.Bu, self.scale, _, _ = fc.CASES[case]
        self.da, self.dc = fc.dims_of(case)
        self.aa = [nn.RELU] * (layers - 1) + [nn.TANH]
        self.ac = [nn.RELU] * (layers - 1) + [nn.IDENT]
        self.seed = self._live_seed(zlib.crc32(case.encode()) % 100000 + quirk)
        self.sets = []
        for _ in range(sets):
            r = np.random.default_rng(self.seed)
            self.sets.append([make_net(pkg, r, d, a, torch.float32, max_cols or self.Bu)
                              for d, a in ((self.da, self.aa), (self.dc, self.ac), (self.da, self.aa), (self.dc, self.ac))])
        self.P = [p for _, p in self.sets[0]]                       # initial fp32 parameters: A, C, At, Ct
        self.rng = np.random.default_rng(self.seed + 7)
        self.lib = self.sets[0][0][0].lib

    def _live_seed(self, seed):
        """An actor of ONE hidden unit per layer is dead on every column for about every other initialisation, and its gradient
        arrays are then exactly zero -- nothing to compare.  The parameters make_net draws from a seed are looked at in the oracle
        alone (no handle is made) and the first seed with a gradient in every actor array on 64 random columns is taken."""
        import types
        dry = types.SimpleNamespace(HipMLP=lambda *a, **k: None)
        for seed in range(seed, seed + 64 * 100003, 100003):
            r = np.random.default_rng(seed)
            PA = make_net(dry, r, self.da, self.aa, torch.float32, 1)[1]
            PC = make_net(dry, r, self.dc, self.ac, torch.float32, 1)[1]
            s = np.random.default_rng(seed + 1).standard_normal((self.ns, 64))
            if all(np.abs(g).max() > 0 for g in self.nn.actor_grads(f64(PA), f64(PC), self.aa, self.ac, s)["gA"]):
                return seed
        raise AssertionError(f"{self.case}: no initialisation with a live actor")

    def nets(self, i=0):
        return [n for n, _ in self.sets[i]]

    def route(self, which, Bu=None):
        A, Cn, At, Ct = self.nets()
        buf, lds = C.create_string_buffer(128), C.c_int64(-1)
        self.L.check(self.L.load().pdec_debug_batched_update_route(A.handle, Cn.handle, At.handle, Ct.handle, Bu or self.Bu, which, buf,
                                                                   128, C.byref(lds)))
        return buf.value.decode(), lds.value

    def assert_routes(self):
        """the passes and the acting kernel this row must reach, and for a 2-layer row the dynamic LDS bytes of
        fused_shape_cases.lds2_rule -- nothing is launched"""
        crit, actor, acting = fc.kernel_names(self.case)
        layers, ns, ha, hc = fc.CASES[self.case][:4]
        lds2 = fc.lds2_rule(ns, ha, hc, fc.read_constants()) if layers == 2 else None
        apart = "/adam_apart" if crit and layers == 2 and self.Bu < 64 else ""
        want = {CRITIC_GRADS: crit or "generic", ACTOR_GRADS: actor or "generic", UPDATE_CRITIC: (crit or "generic") + apart,
                UPDATE_ACTOR: (actor or "generic") + apart}
        for which, name in want.items():
            got, lds = self.route(which)
            assert got == name, (self.case, which, got, name)
            assert (0 < lds <= 160 * 1024) if name != "generic" else lds == 0, (self.case, which, lds)
            if lds2 and name != "generic":
                assert lds == lds2[which in (ACTOR_GRADS, UPDATE_ACTOR)], (self.case, which, lds, lds2)
        got, lds = self.route(ACT, fc.ACT_COLS)
        if acting:
            assert got == acting and 0 < lds <= 64 * 1024, (self.case, got, acting, lds)
            if lds2:
                assert lds == lds2[2], (self.case, lds, lds2)
        else:
            assert got in ("generic", "small_act_kernel") and lds == 0, (self.case, got)

    def batch(self, Bu, safe):
        """fp32 inputs of one minibatch; safe: no column with a ReLU pre-activation within 2e-5 of zero (the gradient checks)"""
        nn, (PA, PC) = self.nn, self.P[:2]
        if not safe:
            return _inputs(self.rng, self.ns, Bu)
        if Bu >= 256:
            return _away_from_relu_kinks(nn, PA, PC, self.aa, self.ac, *_inputs(self.rng, self.ns, Bu))[:5]
        # Few columns: replacing a column by a copy can run out of safe ones (Bu < 16), and the helper's own cap -- at most 10 % of
        # the columns replaced -- is a statement about a rate: a 143-wide 3-layer critic on a 2-row input has a pre-activation
        # within the margin in about 6 % of the columns, which is 7 of 64 columns one time in ten.  So the columns are drawn by
        # rejection from a pool of 1024, on which the helper (and its cap) runs: those it left alone are the safe ones.  None of
        # the chosen columns may be dropped afterwards.
        s, a, r, t, sn = _inputs(self.rng, self.ns, 1024)
        s2, a2, _, _, sn2, _ = _away_from_relu_kinks(nn, PA, PC, self.aa, self.ac, s, a, r, t, sn)
        keep = np.flatnonzero((s2 == s).all(axis=0) & (a2 == a).all(axis=0) & (sn2 == sn).all(axis=0))[:Bu]
        assert keep.size == Bu
        out = (s[:, keep], a[:, keep], r[keep], t[keep], sn[:, keep])
        assert _away_from_relu_kinks(nn, PA, PC, self.aa, self.ac, *out)[5] == 0
        return out

    def dev(self, batch):
        s, a, r, t, sn = batch
        dt = torch.float32
        return to_dev(s.T, dt), to_dev(a.T, dt), to_dev(r, dt), to_dev(t, dt), to_dev(sn.T, dt)

    def grads(self, dv, Bu, i=0):
        """critic_grads then actor_grads on handle set i -> (gC, gA, losses)"""
        L, (A, Cn, At, Ct) = self.L, self.nets(i)
        ds, da_, dr, dt_, dsn = dv
        losses = torch.zeros(2, dtype=torch.float32, device="cuda:0")
        L.check(self.lib.pdec_ddpg_critic_grads(A.handle, Cn.handle, At.handle, Ct.handle, L.ptr(ds), L.ptr(da_), L.ptr(dr), L.ptr(dt_),
                                                L.ptr(dsn), Bu, GAMMA, self.quirk, self.scale, C.c_void_p(losses.data_ptr())))
        gC = read_grads(self.pkg, Cn)
        L.check(self.lib.pdec_ddpg_actor_grads(A.handle, Cn.handle, L.ptr(ds), Bu, self.scale, C.c_void_p(losses.data_ptr() + 4)))
        gA = read_grads(self.pkg, A)
        return gC, gA, losses.cpu().numpy()

    def update_async(self, dv, Bu, i=0, eta_a=ETA_A, eta_c=ETA_C, rho=RHO, losses=None):
        L, (A, Cn, At, Ct) = self.L, self.nets(i)
        ds, da_, dr, dt_, dsn = dv
        L.check(self.lib.pdec_ddpg_update_async(A.handle, Cn.handle, At.handle, Ct.handle, L.ptr(ds), L.ptr(da_), L.ptr(dr), L.ptr(dt_),
                                                L.ptr(dsn), Bu, GAMMA, rho, self.quirk, eta_a, eta_c,
                                                L.ptr(losses) if losses is not None else None))

    def update_split(self, dv, Bu, i, losses):
        L, (A, Cn, At, Ct) = self.L, self.nets(i)
        ds, da_, dr, dt_, dsn = dv
        L.check(self.lib.pdec_ddpg_critic_grads(A.handle, Cn.handle, At.handle, Ct.handle, L.ptr(ds), L.ptr(da_), L.ptr(dr), L.ptr(dt_),
                                                L.ptr(dsn), Bu, GAMMA, self.quirk, 1.0, C.c_void_p(losses.data_ptr())))
        L.check(self.lib.pdec_adam_polyak_step(Cn.handle, Ct.handle, ETA_C, 0.9, 0.999, 1e-8, RHO))
        L.check(self.lib.pdec_ddpg_actor_grads(A.handle, Cn.handle, L.ptr(ds), Bu, 1.0, C.c_void_p(losses.data_ptr() + 4)))
        L.check(self.lib.pdec_adam_polyak_step(A.handle, At.handle, ETA_A, 0.9, 0.999, 1e-8, RHO))

    def act(self, dstate, cols, i=0):
        L, A = self.L, self.nets(i)[0]
        out = torch.empty((cols, 1), dtype=torch.float32, device="cuda:0")
        L.check(self.lib.pdec_policy_act_rng(A.handle, L.ptr(dstate), cols, 0.7, 1.0, 0, 4321, 17, L.ptr(out)))
        return out.cpu().numpy().T.astype(np.float64)


@pytest.mark.parametrize("case", list(fc.CASES))
def test_route_is_the_instantiation_the_row_names(pkg, case):
    """the debug entry reports, from the dispatching host code itself, the kernels the row claims (nothing is launched)"""
    Rig(pkg, case, 1).assert_routes()


def test_route_entry_refuses_what_the_calls_refuse(pkg):
    rig = Rig(pkg, "l3_ns3_a16_c128_bu15", 1)
    A, Cn, At, Ct = rig.nets()
    buf, lds = C.create_string_buffer(128), C.c_int64(-1)
    lib = pkg._lib.load()
    assert lib.pdec_debug_batched_update_route(A.handle, Cn.handle, Cn.handle, Ct.handle, 15, CRITIC_GRADS, buf, 128, C.byref(lds)) != 0
    assert b"target networks" in lib.pdec_last_error()
    assert lib.pdec_debug_batched_update_route(A.handle, Cn.handle, At.handle, Ct.handle, 15, 5, buf, 128, C.byref(lds)) != 0
    # the actor pass of pdec_ddpg_actor_grads and the acting kernel look at no target network
    assert lib.pdec_debug_batched_update_route(A.handle, Cn.handle, 0, 0, 15, ACTOR_GRADS, buf, 128, C.byref(lds)) == 0
    assert buf.value.decode() == "ddpg_actor_fused_kernel<9,2>"
    assert lib.pdec_debug_batched_update_route(A.handle, 0, 0, 0, 300, ACT, buf, 128, C.byref(lds)) == 0
    assert buf.value.decode() == "policy_act_fused_kernel<2>"


def _check_gradients(rig, gC, gA, lv, batch):
    nn, (PA, PC, PAt, PCt) = rig.nn, rig.P
    s, a, r, t, sn = (x.astype(np.float64) for x in batch)
    out = nn.ddpg_losses_and_grads(f64(PA), f64(PC), f64(PAt), f64(PCt), rig.aa, rig.ac, s, a, r, t, sn,
                                   np.float64(np.float32(GAMMA)), bool(rig.quirk))
    out2 = nn.actor_grads(f64(PA), f64(PC), rig.aa, rig.ac, s)
    sc, what = rig.scale, f"{rig.case} quirk={rig.quirk} scale={rig.scale}"
    assert np.isfinite(gC).all() and np.isfinite(gA).all()
    wc = assert_arrays_close(gC, [sc * g for g in out["gC"]], f"critic gradient {what}")
    wa = assert_arrays_close(gA, [sc * g for g in out2["gA"]], f"actor gradient {what}")
    print(f"{what}: worst critic array {wc:.2e}, worst actor array {wa:.2e} of the array's largest entry")
    assert abs(np.linalg.norm(gC) / np.linalg.norm(sc * flat_of(out["gC"])) - 1.0) <= TOL
    assert abs(np.linalg.norm(gA) / np.linalg.norm(sc * flat_of(out2["gA"])) - 1.0) <= TOL
    assert abs(lv[0] - out["critic_loss"]) <= 2e-5 * max(1.0, abs(out["critic_loss"]))
    assert abs(lv[1] - out2["actor_loss"]) <= 2e-5 * max(1.0, abs(out2["actor_loss"]))


@pytest.mark.parametrize("quirk", [1, 0])
@pytest.mark.parametrize("case", rows(fc.CASES))
def test_gradients_match_the_oracle(pkg, case, quirk):
    """check 1: every gradient array of one update, both losses and the norm ratio (src/PDEagent.jl:385-409)"""
    rig = Rig(pkg, case, quirk)
    rig.assert_routes()
    batch = rig.batch(rig.Bu, safe=True)
    gC, gA, lv = rig.grads(rig.dev(batch), rig.Bu)
    _check_gradients(rig, gC, gA, lv, batch)


@pytest.mark.parametrize("quirk", [1, 0])
@pytest.mark.parametrize("case", rows(fc.FUSED))
def test_stale_buffers_of_a_larger_batch_do_not_leak(pkg, case, quirk):
    """check 4: an update on a larger batch leaves slabs, scratch and staging images full beyond the extent of the next call.  The
    update runs at eta = 0 with frozen targets (rho = 1), so it moves no parameter (asserted) and the gradients behind it must
    be those of fresh handles, bit for bit"""
    Bu = fc.CASES[case][4]
    big = 2 * Bu + 333 if Bu < 4096 else Bu + 4099
    rig = Rig(pkg, case, quirk, sets=2, max_cols=big)
    rig.assert_routes()
    dv = rig.dev(rig.batch(Bu, safe=True))
    rig.update_async(rig.dev(rig.batch(big, safe=False)), big, 0, eta_a=0.0, eta_c=0.0, rho=1.0)
    for net, p0 in zip(rig.nets(0), rig.P):
        assert all(np.array_equal(x, y) for x, y in zip(net.params(), p0))
    gC, gA, lv = rig.grads(dv, Bu, 0)
    gC1, gA1, lv1 = rig.grads(dv, Bu, 1)      # (fresh handles on this very batch are what test_gradients_match_the_oracle checks)
    assert np.array_equal(gC, gC1) and np.array_equal(gA, gA1) and np.array_equal(lv, lv1)


@pytest.mark.parametrize("quirk", [1, 0])
@pytest.mark.parametrize("case", rows(fc.CASES))
def test_three_updates_then_acting(pkg, case, quirk):
    """checks 2 and 3: the finish kernels read slabs of MT tiles back into flat [H][K0] arrays and re-stage the padded images after
    ADAM; the acting kernel then reads the image the last update published"""
    from oracle import nn
    rig = Rig(pkg, case, quirk, sets=2)
    rig.assert_routes()
    Bu, npdt = rig.Bu, np.float32
    PA, PC, PAt, PCt = ([p.copy() for p in P] for P in rig.P)
    optA, optC = nn.Adam(PA, ETA_A), nn.Adam(PC, ETA_C)
    losses = torch.zeros(2, dtype=torch.float32, device="cuda:0")
    losses2 = torch.zeros(2, dtype=torch.float32, device="cuda:0")
    state = rig.rng.standard_normal((rig.ns, fc.ACT_COLS)).astype(npdt)
    dstate = to_dev(state.T, torch.float32)
    fused_act = fc.kernel_names(case)[2] is not None
    if fused_act:
        act0 = rig.act(dstate, fc.ACT_COLS)             # stages (3-layer: publishes) the image of the initial parameters
        assert np.abs(act0 - nn.policy_act(f64(rig.P[0]), rig.aa, state.astype(np.float64), None, 0.0, 1.0, learning=False)).max() <= 1e-5
    for it in range(3):
        batch = rig.batch(Bu, safe=False)
        s, a, r, t, sn = batch
        out = nn.ddpg_update(PA, PC, PAt, PCt, optA, optC, rig.aa, rig.ac, s, a, r, t, sn, npdt(np.float32(GAMMA)), np.float32(RHO),
                             bool(quirk))
        dv = rig.dev(batch)
        rig.update_async(dv, Bu, 0, losses=losses)
        rig.update_split(dv, Bu, 1, losses2)
        assert torch.equal(losses, losses2), (it, losses, losses2)
        lv = losses.cpu().numpy()
        assert abs(lv[0] - out["critic_loss"]) <= 2e-4 * max(1.0, abs(out["critic_loss"]))
        assert abs(lv[1] - out["actor_loss"]) <= 2e-4 * max(1.0, abs(out["actor_loss"]))
        for i, (P, who) in enumerate(zip((PA, PC, PAt, PCt), ("actor", "critic", "target actor", "target critic"))):
            for j, (x, y, z) in enumerate(zip(rig.nets(0)[i].params(), rig.nets(1)[i].params(), P)):
                assert np.array_equal(x, y), f"{case}: update {it}, {who} array {j}: update_async and the split sequence differ"
                assert relerr(x, z) <= 2e-4, f"{case}: update {it}, {who} array {j} off by {relerr(x, z):.3e}"
    if not fused_act:
        return
    for i in range(2):
        got = rig.act(dstate, fc.ACT_COLS, i)
        back = rig.nets(i)[0].params()                  # what the library's actor holds now
        ref = nn.policy_act(f64(back), rig.aa, state.astype(np.float64), None, 0.0, 1.0, learning=False)
        assert np.abs(got - ref).max() <= 1e-5, f"{case}: acting after the updates off by {np.abs(got - ref).max():.3e} (handle set {i})"
        # a stale image would give the actions of the initial parameters: the updates moved them by far more than the tolerance
        assert np.abs(got - act0).max() >= 1e-4, np.abs(got - act0).max()
