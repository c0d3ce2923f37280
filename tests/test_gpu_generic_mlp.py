"""The GENERIC path of the weight-shared MLPs (csrc/mlp.hip) at its tile, split-K and dtype edges, against the fp64 oracle.

gemm_kernel<T> is ONE template behind forward, dW and dX of every fp64 network and of every fp32 network outside the fused
tables, so an indexing slip at a tile edge breaks both types alike.  The rows of generic_mlp_cases.py put layer widths and column
counts ON the edges of its 64 x 64 x 16 tile and of the 512-column split of dW, run 1- to 8-layer nets with every activation as
hidden and as output layer, and run a second, smaller column count on the handle the first left behind
(test_generic_mlp_table.py holds the table against these claims on the CPU).
  a. forward / backward   every network row x {f32, f64} x each column count: y, dX and every gradient array
  b. ADAM by itself       adam_kernel<T> on a written gradient buffer: p, m, v and the beta powers against oracle.nn.Adam
  c. Polyak and copy      polyak_kernel<double> (rho rounded to Float32 first), the frozen case rho = 1, cast_copy_kernel both ways
  d. generic DDPG passes  critic_grads_t / actor_grads_t (fp64, and fp32 with na = 2, tanh hidden layers, 4 layers): gradients,
                          losses, then two whole updates of the fp64 rows and the async entry bit for bit
Tolerances: fp32 forward <= 1e-5, fp32 dX / gradients <= 1e-4, fp64 <= 1e-11 / 1e-10, each of the array's largest
entry; nothing is measured against the kernel under test."""
import ctypes as C

import numpy as np
import pytest

import generic_mlp_cases as gc
from test_gpu_grads import _away_from_relu_kinks, assert_arrays_close
from test_gpu_mlp import make_net, relerr
from util import to_dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TDT = {"f32": torch.float32, "f64": torch.float64}


def arrays_close(got_list, want_list, tol, what):
    """every array within tol of ITS largest reference entry -> the worst ratio"""
    worst = 0.0
    assert len(got_list) == len(want_list)
    for i, (g, w) in enumerate(zip(got_list, want_list)):
        w = np.asarray(w, dtype=np.float64)
        scale = np.abs(w).max()
        assert scale > 0, (what, i)
        err = np.abs(np.asarray(g, dtype=np.float64).reshape(w.shape) - w).max() / scale
        worst = max(worst, err)
        assert err <= tol, f"{what}: array {i} {w.shape} off by {err:.3e} of its largest entry {scale:.3e} (tolerance {tol:.0e})"
    return worst


def split_flat(flat, shapes_like):
    """the library's flat order -- per layer [W row-major [out][in] | b] -- cut into arrays shaped like shapes_like"""
    out, o = [], 0
    for w in shapes_like:
        out.append(np.asarray(flat[o:o + w.size]).reshape(w.shape))
        o += w.size
    assert o == len(flat)
    return out


def grad_view(pkg, net):
    """the network's flat gradient buffer as a device tensor of the network's type (a view: writable)"""
    ptr, n = net.grad_buffer()
    assert n == net.num_params
    return torch.as_tensor(pkg.distributed._DevArray(ptr, n, "<f8" if net.dtype == torch.float64 else "<f4"), device=net.device)


def read_flat_grads(pkg, net):
    torch.cuda.synchronize()
    return grad_view(pkg, net).cpu().numpy().astype(np.float64)


def net_of(pkg, name, prec, max_cols, dims_acts=None):
    """a handle with the row's parameters, drawn by make_net from the row's seed -- the very values the table draws"""
    dims, acts = dims_acts or gc.NETS[name][:2]
    net, P = make_net(pkg, np.random.default_rng(gc.seed_of(name, 0)), dims, acts, TDT[prec], max_cols)
    want = gc.draw_params(np.random.default_rng(gc.seed_of(name, 0)), dims, prec)
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(P, want))
    return net, P


# ------------------------------------------------------------------ a. forward / backward
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("name", list(gc.NETS))
def test_forward_backward_at_the_tile_edges(pkg, name, prec):
    dims, acts, col_counts = gc.NETS[name]
    dtype, tol = TDT[prec], gc.TOL[prec]
    net, P = net_of(pkg, name, prec, max(col_counts))
    for cols in col_counts:                 # in the table's order, on the one handle: a later count runs over stale buffers
        x, dy, _ = gc.net_data(name, cols, prec, P)
        y, g, dx = gc.net_reference(P, acts, x, dy)
        xd, dyd = to_dev(x.T, dtype), to_dev(dy.T, dtype)
        yd = net(xd).cpu().numpy().T
        gg, dxd = net.backward(xd, dyd)
        dxd = dxd.cpu().numpy().T
        what = f"{name} {prec} cols={cols}"
        ef, ex = relerr(yd, y), relerr(dxd, dx)
        eg = [relerr(a, b) for a, b in zip(gg, g)]
        print(f"{what}: forward {ef:.2e} (tol {tol['forward']:.0e}), dX {ex:.2e}, worst gradient array {max(eg):.2e} (tol {tol['grad']:.0e})")
        assert yd.shape == y.shape and np.isfinite(yd).all()
        assert ef <= tol["forward"], what
        assert ex <= tol["grad"], what
        arrays_close(gg, g, tol["grad"], f"gradient {what}")
        # without dX the weight gradients are the same bits; a repeated call repeats them (the slab reduction is deterministic)
        g_nodx, none = net.backward(xd, dyd, want_dx=False)
        assert none is None and all(np.array_equal(a, b) for a, b in zip(g_nodx, gg)), what
        gg2, dxd2 = net.backward(xd, dyd)
        assert all(np.array_equal(a, b) for a, b in zip(gg2, gg)) and np.array_equal(dxd2.cpu().numpy().T, dxd), what
        assert np.array_equal(net(xd).cpu().numpy().T, yd), what
    over = max(col_counts) + 1
    with pytest.raises(pkg.PdecError, match="max_cols"):
        net(torch.zeros((over, dims[0]), dtype=dtype, device="cuda:0"))
    for a, b in zip(net.params(), P):       # checkpoint / copyto!: the bits that went in
        assert a.dtype == b.dtype and np.array_equal(a, b)


# ------------------------------------------------------------------ b. ADAM by itself
ADAM_NET = "l5_bottleneck"
ADAM_ETA, ADAM_B1, ADAM_B2, ADAM_EPS = 5e-4, 0.9, 0.999, 1e-8


def adam_gradients(n, steps=3):
    """flat gradients whose entries mix exact zeros, +-1e-12, +-1e-6, O(1) and +-1e3 (no nonzero |g| below 1e-15: g^2 stays a normal
    Float32); entry i keeps its class over the steps with another value, and every eighth entry is zero in EVERY step"""
    rng = np.random.default_rng([gc.seed_of(ADAM_NET, 0)[0], 77])
    mags = np.array([0.0, 1e-12, 1e-6, 1.0, 1e3, 1.0, 1e-6, 0.0])
    cls = np.arange(n) % 8
    cls[1::16] = rng.integers(1, 7, cls[1::16].size)        # some entries change class from step to step below
    out = []
    for k in range(steps):
        c = cls.copy()
        c[1::16] = (c[1::16] + k) % 7
        g = mags[c] * rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)
        g[::8] = 0.0
        assert ((g == 0) | (np.abs(g) >= 1e-15)).all()
        out.append(g)
    return out


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_adam_by_itself(pkg, prec):
    """adam_kernel<T> (Flux.Optimise.ADAM: arithmetic in Float64, stored in T) on gradients written into the flat buffer, three steps"""
    from oracle import nn
    dims, acts, _ = gc.NETS[ADAM_NET]
    npdt = gc.np_dtype(prec)
    net, P0 = net_of(pkg, ADAM_NET, prec, 16)
    P = [p.copy() for p in P0]
    opt = nn.Adam(P, ADAM_ETA, (ADAM_B1, ADAM_B2), ADAM_EPS)
    view = grad_view(pkg, net)
    bp = np.array([ADAM_B1, ADAM_B2])
    grads = adam_gradients(net.num_params)
    for g in grads:
        g = g.astype(npdt)
        view.copy_(torch.as_tensor(g, device=net.device))
        torch.cuda.synchronize()
        pkg._lib.check(net.lib.pdec_adam_step(net.handle, ADAM_ETA, ADAM_B1, ADAM_B2, ADAM_EPS))
        P = opt.step(P, split_flat(g, P))
        bp = bp * np.array([ADAM_B1, ADAM_B2])
    m = np.empty(net.num_params, dtype=npdt)
    v = np.empty_like(m)
    bpd = (C.c_double * 2)()
    pkg._lib.check(net.lib.pdec_adam_get_state(net.handle, m.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), bpd))
    got = {"p": net.params(), "m": net._unflatten(m), "v": net._unflatten(v)}
    tol = 2e-5 if prec == "f32" else 1e-12
    for key, want in (("p", P), ("m", opt.m), ("v", opt.v)):
        assert all(a.dtype == npdt for a in got[key])
        worst = arrays_close(got[key], want, tol, f"adam {prec} {key}")
        print(f"adam {prec} {key}: worst array {worst:.2e} of its largest entry (tol {tol:.0e})")
    # the beta powers are Float64 whatever the network's type: the iterated binary64 products, bit for bit
    assert (bpd[0], bpd[1]) == (bp[0], bp[1]) and bp[0] == ADAM_B1 * ADAM_B1 * ADAM_B1 * ADAM_B1
    # an entry whose gradient was zero in every step never moved, and holds no moment
    still = split_flat(np.arange(net.num_params) % 8 == 0, P0)
    assert sum(int(z.sum()) for z in still) == -(-net.num_params // 8)
    for p_new, p_old, m_, v_, z in zip(got["p"], P0, got["m"], got["v"], still):
        assert np.array_equal(p_new[z], p_old[z]) and not m_[z].any() and not v_[z].any()


# ------------------------------------------------------------------ c. Polyak and copy
def two_nets(pkg, prec):
    dims, acts, _ = gc.NETS[ADAM_NET]
    rng = np.random.default_rng(gc.seed_of(ADAM_NET, 1))
    return make_net(pkg, rng, dims, acts, TDT[prec], 16), make_net(pkg, rng, dims, acts, TDT[prec], 16)


def test_polyak_f64_rounds_rho_to_float32_first(pkg):
    """pdec_polyak on fp64 networks: dest = rho32 dest + (1 - rho32) src with rho32 = Float32(rho) and 1 - rho32 formed in Float32,
    then widened (the reference holds p = 0.995f0)"""
    (dst, PD), (src, PS) = two_nets(pkg, "f64")
    pkg._lib.check(dst.lib.pdec_polyak(dst.handle, src.handle, 0.995))
    rho32 = np.float32(0.995)
    omr = np.float64(np.float32(1.0) - rho32)
    assert np.float64(rho32) != 0.995       # (1 - rho32 is exact in Float32 -- Sterbenz --, so only the rounding of rho shows)
    want = [np.float64(rho32) * d + omr * s for d, s in zip(PD, PS)]
    worst = arrays_close(dst.params(), want, 1e-15, "polyak f64")
    print(f"polyak f64: worst array {worst:.2e} of its largest entry (tol 1e-15)")
    # the rounding is visible at this tolerance: rho taken as a double is 5e-9 away
    assert relerr(np.concatenate([a.ravel() for a in want]),
                  np.concatenate([(0.995 * d + (1 - 0.995) * s).ravel() for d, s in zip(PD, PS)])) > 1e-10
    for a, b in zip(src.params(), PS):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_polyak_rho_one_leaves_the_target_untouched(pkg, prec):
    """rho = 1 is the reference as it runs (frozen targets): the target keeps its bits, also where 0 * src would be NaN"""
    (dst, PD), (src, PS) = two_nets(pkg, prec)
    bad = [p.copy() for p in PS]
    bad[0].flat[0], bad[0].flat[-1], bad[1].flat[0], bad[-1].flat[-1] = np.inf, np.nan, -np.inf, np.nan
    src.set_params(bad)
    assert not all(np.isfinite(a).all() for a in src.params())
    pkg._lib.check(dst.lib.pdec_polyak(dst.handle, src.handle, 1.0))
    for a, b in zip(dst.params(), PD):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_clone_casts_exactly_up_and_by_rounding_down(pkg):
    """HipMLP.clone(dtype=...): cast_copy_kernel<double, float> is exact, <float, double> rounds as astype(float32) does"""
    (n32, P32), (n64, P64) = two_nets(pkg, "f32")[0], two_nets(pkg, "f64")[1]
    up = n32.clone(dtype=torch.float64)
    for a, b in zip(up.params(), P32):
        assert a.dtype == np.float64 and np.array_equal(a, b.astype(np.float64))
    down = n64.clone(dtype=torch.float32)
    inexact = 0
    for a, b in zip(down.params(), P64):
        assert a.dtype == np.float32 and np.array_equal(a, b.astype(np.float32))
        inexact += int((b.astype(np.float32).astype(np.float64) != b).sum())
    assert inexact > 0                               # the fp64 source did hold more than 24 bits
    same = n64.clone()
    for a, b in zip(same.params(), P64):
        assert a.dtype == np.float64 and np.array_equal(a, b)


# ------------------------------------------------------------------ d. generic DDPG passes
class Pair:
    """the four networks of a DDPG row -- A, C, At, Ct, drawn in this order from the row's seed -- and its batches"""

    def __init__(self, pkg, name, quirk):
        self.pkg, self.L, self.name, self.quirk = pkg, pkg._lib, name, quirk
        self.da, self.aa, self.dc, self.ac, self.prec, self.Bu = gc.DDPG[name]
        self.dtype, self.ts = TDT[self.prec], 8 if self.prec == "f64" else 4
        self.case = gc.ddpg_case(name, quirk)

    def handles(self):
        rng = np.random.default_rng(self.case["seed"])
        made = [make_net(self.pkg, rng, d, a, self.dtype, self.Bu) for d, a in ((self.da, self.aa), (self.dc, self.ac)) * 2]
        for (_, P), want in zip(made, self.case["P"]):
            assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(P, want))
        return [n for n, _ in made]

    def dev(self, batch):
        s, a, r, t, sn = batch
        dt = self.dtype
        return [to_dev(s.T, dt), to_dev(a.T, dt), to_dev(r, dt), to_dev(t, dt), to_dev(sn.T, dt)]

    def assert_generic(self, nets):
        A, Cn, At, Ct = nets
        for which in range(4):
            buf, lds = C.create_string_buffer(128), C.c_int64(-1)
            self.L.check(self.L.load().pdec_debug_batched_update_route(A.handle, Cn.handle, At.handle, Ct.handle, self.Bu, which, buf,
                                                                       128, C.byref(lds)))
            assert buf.value.decode() == "generic" and lds.value == 0, (self.name, which, buf.value)


@pytest.mark.parametrize("quirk", gc.QUIRKS)
@pytest.mark.parametrize("name", list(gc.DDPG))
def test_generic_ddpg_gradients_match_the_oracle(pkg, name, quirk):
    """steps 1 - 3: the route, then the critic gradient (src/PDEagent.jl:385-400) and the actor gradient through the critic
    (:402-409) read from the flat buffers, every array and both losses, at grad_scale 1 and 0.5"""
    from oracle import nn
    pair = Pair(pkg, name, quirk)
    L, Bu, prec, tol = pair.L, pair.Bu, pair.prec, gc.TOL[pair.prec]
    nets = pair.handles()
    A, Cn, At, Ct = nets
    pair.assert_generic(nets)
    # the table's kink replacement is the project's: _away_from_relu_kinks finds nothing left to replace
    PA, PC = pair.case["P"][:2]
    assert _away_from_relu_kinks(nn, PA, PC, pair.aa, pair.ac, *pair.case["batch"])[5] == 0
    out, out2 = gc.ddpg_reference(name, quirk, pair.case)
    ds, da_, dr, dt_, dsn = pair.dev(pair.case["batch"])
    for scale in (1.0, 0.5):
        losses = torch.zeros(2, dtype=pair.dtype, device="cuda:0")
        L.check(A.lib.pdec_ddpg_critic_grads(A.handle, Cn.handle, At.handle, Ct.handle, L.ptr(ds), L.ptr(da_), L.ptr(dr), L.ptr(dt_),
                                             L.ptr(dsn), Bu, gc.GAMMA, quirk, scale, C.c_void_p(losses.data_ptr())))
        gC = read_flat_grads(pkg, Cn)
        L.check(A.lib.pdec_ddpg_actor_grads(A.handle, Cn.handle, L.ptr(ds), Bu, scale, C.c_void_p(losses.data_ptr() + pair.ts)))
        gA = read_flat_grads(pkg, A)
        assert np.isfinite(gC).all() and np.isfinite(gA).all()
        what = f"{name} quirk={quirk} scale={scale}"
        wantC, wantA = [scale * g for g in out["gC"]], [scale * g for g in out2["gA"]]
        if prec == "f32":                   # the comparison of test_fused_pass_gradients_match_the_oracle itself (1e-4)
            wc = assert_arrays_close(gC, wantC, f"critic gradient {what}")
            wa = assert_arrays_close(gA, wantA, f"actor gradient {what}")
        else:
            wc = arrays_close(split_flat(gC, wantC), wantC, tol["grad"], f"critic gradient {what}")
            wa = arrays_close(split_flat(gA, wantA), wantA, tol["grad"], f"actor gradient {what}")
        lv = losses.cpu().numpy().astype(np.float64)
        el = [abs(lv[0] - out["critic_loss"]) / max(1.0, abs(out["critic_loss"])),
              abs(lv[1] - out2["actor_loss"]) / max(1.0, abs(out2["actor_loss"]))]
        print(f"{what}: worst critic array {wc:.2e}, worst actor array {wa:.2e} (tol {tol['grad']:.0e}), losses {el[0]:.2e} {el[1]:.2e} "
              f"(tol {tol['loss']:.0e})")
        assert max(el) <= tol["loss"], what


@pytest.mark.parametrize("quirk", gc.QUIRKS)
@pytest.mark.parametrize("name", gc.F64_DDPG)
def test_generic_f64_updates_match_the_oracle_and_the_async_entry(pkg, name, quirk):
    """steps 4 - 6: two consecutive pdec_ddpg_update calls (rho = 0.995) against oracle.nn.ddpg_update -- all four networks, both
    losses -- and the same updates through pdec_ddpg_update_async on fresh handles, bit for bit"""
    pair = Pair(pkg, name, quirk)
    L, Bu = pair.L, pair.Bu
    nets, fresh = pair.handles(), pair.handles()
    pair.assert_generic(nets)
    want_P, want_losses, masks = gc.ddpg_reference_updates(name, quirk, pair.case)
    tol = gc.TOL_UPDATE_F64
    async_losses = torch.zeros(2, dtype=pair.dtype, device="cuda:0")
    for it, batch in enumerate(pair.case["batches"]):
        dv = pair.dev(batch)
        al, cl = C.c_double(), C.c_double()
        L.check(nets[0].lib.pdec_ddpg_update(*[n.handle for n in nets], *[L.ptr(x) for x in dv], Bu, gc.GAMMA, gc.RHO, quirk,
                                             gc.ETA_A, gc.ETA_C, C.byref(al), C.byref(cl)))
        L.check(nets[0].lib.pdec_ddpg_update_async(*[n.handle for n in fresh], *[L.ptr(x) for x in dv], Bu, gc.GAMMA, gc.RHO, quirk,
                                                   gc.ETA_A, gc.ETA_C, L.ptr(async_losses)))
        torch.cuda.synchronize()
        wc, wa = want_losses[it]
        el = [abs(cl.value - wc) / max(1.0, abs(wc)), abs(al.value - wa) / max(1.0, abs(wa))]
        print(f"{name} quirk={quirk} update {it}: losses off by {el[0]:.2e} {el[1]:.2e} (tol {tol:.0e})")
        assert max(el) <= tol
        assert async_losses.cpu().numpy().tolist() == [cl.value, al.value]
    for net, other, want, mask, who in zip(nets, fresh, want_P, masks, ("actor", "critic", "target actor", "target critic")):
        got = net.params()
        for j, (x, y, z, m) in enumerate(zip(got, other.params(), want, mask)):
            assert np.array_equal(x, y), f"{name}: {who} array {j}: pdec_ddpg_update and pdec_ddpg_update_async differ"
            # ADAM's first step is ill-conditioned at an almost-zero gradient: such entries (at most 0.1 % of an array) are left out
            assert int(m.sum()) <= int(gc.SMALL_GRAD_CAP * m.size), (who, j, int(m.sum()))
            keep = ~m
            err = np.abs(x[keep] - z[keep]).max() / np.abs(z).max()
            assert err <= tol, f"{name} quirk={quirk}: {who} array {j} off by {err:.3e} (tolerance {tol:.0e})"
        print(f"{name} quirk={quirk} {who}: worst array {max(relerr(x, z) for x, z in zip(got, want)):.2e} (tol {tol:.0e})")
