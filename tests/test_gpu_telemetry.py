"""GPU tests of the telemetry object alone (csrc/telemetry.hip: pdec_telemetry_create / _step / _update / _read / _reset), without
an environment: synthetic rows and small HipMLPs, every row held to the NumPy model of tests/telemetry_ref.py -- counts, minima,
maxima, losses and the sentinel exactly, sums to the model's derived bound -- in fp32 and fp64, at the sizes where the launches take
another path: one lane, a full wave +- 1, one workgroup's chunk +- 1 (1024 row elements, 4096 parameters), several workgroups."""
import ctypes as C

import numpy as np
import pytest
import torch

from telemetry_ref import STEP_COLUMNS, UPDATE_COLUMNS, mismatches, ring, step_nonfinite, step_row, update_nonfinite, update_row

pytestmark = pytest.mark.gpu

DT = {"f32": (torch.float32, np.float32), "f64": (torch.float64, np.float64)}
LIMIT = 0.5


class _Obj:
    def __init__(self, pkg, cap, B, cols, ns, na, tdt, actor, critic, stream):
        self.L = L = pkg._lib
        self.lib = L.init(0)
        self.h = L.Handle()
        self.cap = cap
        L.check(self.lib.pdec_telemetry_create(C.byref(self.h), cap, B, cols, ns, na, L.dtype_code(tdt), actor.handle, critic.handle))
        L.check(self.lib.pdec_set_stream(self.h, C.c_void_p(stream.cuda_stream)))

    def step(self, s, a, r, t, f, limit=LIMIT):
        p = self.L.ptr
        self.L.check(self.lib.pdec_telemetry_step(self.h, p(s), p(a), p(r), p(t), p(f), float(limit)))

    def update(self, A, Cn, At, Ct, losses):
        self.L.check(self.lib.pdec_telemetry_update(self.h, A.handle, Cn.handle, At.handle, Ct.handle, self.L.ptr(losses)))

    def read(self):
        """(step rows, update rows: lists of name -> value, oldest first; dropped counts; the sentinel pair)"""
        srows, urows = np.full((self.cap, len(STEP_COLUMNS)), -7.0), np.full((self.cap, len(UPDATE_COLUMNS)), -7.0)
        ns, nu, sent = C.c_int64(), C.c_int64(), np.zeros(2, dtype=np.int64)
        p = self.L.ptr
        self.L.check(self.lib.pdec_telemetry_read(self.h, p(srows), C.byref(ns), p(urows), C.byref(nu), p(sent)))
        out = []
        for rows, n, names in ((srows, ns.value, STEP_COLUMNS), (urows, nu.value, UPDATE_COLUMNS)):
            kept, dropped = ring(range(n), self.cap)
            out += [[dict(zip(names, rows[c % self.cap])) for c in kept], dropped]
        return out[0], out[1], out[2], out[3], (int(sent[0]), int(sent[1])), (srows, urows)

    def reset(self):
        self.L.check(self.lib.pdec_telemetry_reset(self.h))

    def close(self):
        self.lib.pdec_destroy(self.h)


def _tiny_nets(pkg, tdt, stream, dims_a=(1, 1), dims_c=(2, 1)):
    mk = lambda d: pkg.nna.HipMLP(list(d), ["identity"] * (len(d) - 1), None, tdt, "cuda:0", 1, stream)
    return mk(dims_a), mk(dims_c)


def _step_inputs(rng, case, B, cols, ns, na, npdt):
    """host arrays of one step call.  planted: NaN / +Inf / -Inf in rewards and states, actions exactly at +-LIMIT and one ulp
    inside it; all_bad: no finite reward; clean: nothing planted"""
    lim = npdt(LIMIT)
    s = rng.normal(size=(cols, ns)).astype(npdt)
    a = (0.4 * rng.normal(size=(cols, na))).astype(npdt)
    a[:, 1:] = 9.0                                         # memory rows: never looked at
    r = (3.0 * rng.normal(size=cols)).astype(npdt)
    t = (rng.random(cols) < 0.3).astype(npdt)
    f = (rng.random(B) < 0.4).astype(np.int32) * rng.integers(1, 5, B).astype(np.int32)
    if case == "planted":
        edge = [lim, -lim, np.nextafter(lim, npdt(0)), -np.nextafter(lim, npdt(0)), np.nextafter(lim, npdt(1))]
        for i, v in enumerate(edge[:cols]):
            a[(i * 7) % cols, 0] = v
        for i, v in enumerate([np.nan, np.inf, -np.inf][:max(1, cols // 2)]):
            r[(i * 5 + cols - 1) % cols] = v
        flat = s.reshape(-1)
        for i, v in enumerate([np.nan, np.inf, -np.inf, np.nan][:max(1, flat.size // 2)]):
            flat[(i * 11 + flat.size - 1) % flat.size] = v
    elif case == "all_bad":
        r[:] = np.array([np.nan, np.inf, -np.inf], dtype=npdt)[np.arange(cols) % 3]
    return s, a, r, t, f


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_step_rows(pkg, dt):
    tdt, npdt = DT[dt]
    st = torch.cuda.Stream()
    A, Cn = _tiny_nets(pkg, torch.float32, st)
    rng = np.random.default_rng(5)
    bad, seen_blocks = [], set()
    for cols in (1, 63, 64, 65, 257, 1025):
        for ns in (1, 9):
            for na in (1, 3):
                for B in sorted({1, max(1, cols // 8), cols}):
                    o = _Obj(pkg, 8, B, cols, ns, na, tdt, A, Cn, st)
                    seen_blocks.add((cols * ns + 1023) // 1024)
                    want = []
                    for k, case in enumerate(("planted", "clean", "all_bad", "clean")):
                        host = _step_inputs(rng, case, B, cols, ns, na, npdt)
                        with torch.cuda.stream(st):
                            dev = [torch.as_tensor(x).to("cuda:0", non_blocking=False) for x in host]
                            o.step(*dev)
                        st.synchronize()
                        want.append(step_row(*host, LIMIT, step=k))
                    rows, dropped, _u, _du, sent, _raw = o.read()
                    where = f"[{dt} cols {cols} ns {ns} na {na} B {B}] "
                    if dropped != 0 or len(rows) != 4 or len(_u) != 0:
                        bad.append(where + "row counts")
                    for k, (g, (w, tol)) in enumerate(zip(rows, want)):
                        bad += mismatches(g, w, tol, STEP_COLUMNS, where + f"call {k} ")
                    w2 = want[2][0]
                    if not (np.isnan(w2["reward_mean"]) and w2["reward_nonfinite"] == cols):
                        bad.append(where + "the model of the all-non-finite call")
                    first = next(k for k, (w, _t) in enumerate(want) if step_nonfinite(w))
                    if sent != (first, -1):
                        bad.append(where + f"sentinel {sent}, want ({first}, -1)")
                    o.close()
    assert {1, 2, 3, 10} <= seen_blocks                    # one workgroup, a partial last one, several
    assert bad == [], bad[:10]


def _params(rng, net, scale=1.0):
    return [(scale * rng.normal(size=np.shape(p))).astype(net.np_dtype) for p in net._unflatten(np.zeros(net.num_params))]


# flat sizes: 2; 255 / 256 / 257 (a workgroup's 256 threads +- 1); 4095 / 4096 / 4097 (one workgroup's chunk +- 1); 8221 (three)
NETS = {2: (1, 1), 255: (2, 85), 256: (1, 128), 257: (256, 1), 4095: (64, 63), 4096: (63, 64), 4097: (16, 241), 8221: (20, 100, 60, 1)}


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_update_rows(pkg, dt):
    """actor and critic of different sizes, targets equal to and different from the behaviour nets, a planted NaN parameter, and
    step2 across three calls with host-side parameter writes in between: 0, then exact to the bound"""
    tdt, npdt = DT[dt]
    st = torch.cuda.Stream()
    rng = np.random.default_rng(11)
    mk = lambda d: pkg.nna.HipMLP(list(d), ["identity"] * (len(d) - 1), None, tdt, "cuda:0", 1, st)
    sizes = list(NETS)
    bad = []
    for i, na_ in enumerate(sizes):
        nc_ = sizes[(i + 3) % len(sizes)]
        A, Cn, At, Ct = mk(NETS[na_]), mk(NETS[nc_]), mk(NETS[na_]), mk(NETS[nc_])
        assert A.num_params == na_ and Cn.num_params == nc_
        o = _Obj(pkg, 8, 1, 1, 1, 1, torch.float32, A, Cn, st)
        losses = torch.zeros(2, dtype=tdt, device="cuda:0")
        want, prev = [], (None, None)
        for k in range(3):
            pa, pc = _params(rng, A), _params(rng, Cn, 3.0)
            pat, pct = (pa, pc) if k == 0 else (_params(rng, A), _params(rng, Cn))      # call 0: the targets equal the nets
            if k == 1:
                pa[0].reshape(-1)[pa[0].size // 2] = np.nan                             # one NaN parameter
                pct[-1].reshape(-1)[0] = np.inf                                         # ... and a non-finite target entry
            for net, p in ((A, pa), (Cn, pc), (At, pat), (Ct, pct)):
                net.set_params(p)
            lv = np.array([0.1 * (k + 1), -1.0 / 3.0 - k], dtype=npdt)
            with torch.cuda.stream(st):
                losses.copy_(torch.as_tensor(lv))
                o.update(A, Cn, At, Ct, losses)
            st.synchronize()
            want.append(update_row(lv, pa, pc, pat, pct, prev[0], prev[1], update=k))
            prev = (pa, pc)
        _s, _ds, rows, dropped, sent, _raw = o.read()
        where = f"[{dt} actor {na_} critic {nc_}] "
        if dropped != 0 or len(rows) != 3 or len(_s) != 0:
            bad.append(where + "row counts")
        for k, (g, (w, tol)) in enumerate(zip(rows, want)):
            bad += mismatches(g, w, tol, UPDATE_COLUMNS, where + f"call {k} ")
        w0, w1, w2 = (w for w, _t in want)
        if not (w0["actor_step2"] == 0 == w0["critic_step2"] and w0["actor_target_dist2"] == 0 and w1["actor_nonfinite"] == 1
                and w2["actor_step2"] > 0 and w2["critic_step2"] > 0 and update_nonfinite(w1) and not update_nonfinite(w0)):
            bad.append(where + "the model's own rows")
        if sent != (-1, 1):
            bad.append(where + f"sentinel {sent}, want (-1, 1)")
        o.close()
    assert bad == [], bad[:10]


def _sequence(pkg, st, o, nets, calls, seed):
    """`calls` step and update calls on fixed-seed data; the raw rings"""
    rng = np.random.default_rng(seed)
    A, Cn = nets
    losses = torch.zeros(2, dtype=torch.float32, device="cuda:0")
    for k in range(calls):
        host = _step_inputs(rng, "planted" if k == 2 else "clean", 3, 257, 9, 1, np.float32)
        A.set_params(_params(rng, A))
        with torch.cuda.stream(st):
            dev = [torch.as_tensor(x).to("cuda:0") for x in host]
            o.step(*dev)
            losses.copy_(torch.as_tensor(np.array([np.inf if k == 4 else k, -k], dtype=np.float32)))
            o.update(A, Cn, A, Cn, losses)
        st.synchronize()
    return o.read()


def test_ring_wrap_sticky_sentinel_reset_and_repeatability(pkg):
    st = torch.cuda.Stream()
    mk = lambda d: pkg.nna.HipMLP(list(d), ["identity"] * (len(d) - 1), None, torch.float32, "cuda:0", 1, st)
    nets = (mk(NETS[8221]), mk(NETS[4097]))
    o = _Obj(pkg, 4, 3, 257, 9, 1, torch.float32, nets[0], nets[1], st)
    srows, ds, urows, du, sent, raw1 = _sequence(pkg, st, o, nets, 11, seed=3)
    # capacity 4, 11 calls: rows 7 .. 10, 7 dropped
    assert ds == du == 7
    assert [r["step"] for r in srows] == [7, 8, 9, 10] == [r["update"] for r in urows]
    # call 2 planted non-finite rewards / states and call 4 an infinite loss: both long overwritten by clean rows, both remembered
    assert sent == (2, 4)
    assert all(r["reward_nonfinite"] == 0 == r["state_nonfinite"] for r in srows)
    assert all(np.isfinite(r["critic_loss"]) and r["actor_nonfinite"] == 0 for r in urows)
    # reset: rings, counters, sentinel and theta_prev as at creation -- the same sequence again gives the same bits
    o.reset()
    e = o.read()
    assert e[0] == [] and e[2] == [] and e[1] == e[3] == 0 and e[4] == (-1, -1) and not e[5][0].any() and not e[5][1].any()
    again = _sequence(pkg, st, o, nets, 11, seed=3)
    assert again[4] == (2, 4) and again[2][0]["update"] == 7
    for a, b in zip(raw1, again[5]):
        assert a.tobytes() == b.tobytes()
    # ... and so does a fresh object
    o2 = _Obj(pkg, 4, 3, 257, 9, 1, torch.float32, nets[0], nets[1], st)
    fresh = _sequence(pkg, st, o2, nets, 11, seed=3)
    for a, b in zip(raw1, fresh[5]):
        assert a.tobytes() == b.tobytes()
    # the first update row of a sequence has step2 = 0, the later ones do not (the actor is rewritten before every call)
    o.reset()
    first = _sequence(pkg, st, o, nets, 2, seed=3)[2]
    assert first[0]["actor_step2"] == 0 and first[1]["actor_step2"] > 0 and first[1]["critic_step2"] == 0
    o.close()
    o2.close()


def test_mismatched_networks_are_refused(pkg):
    st = torch.cuda.Stream()
    A, Cn = _tiny_nets(pkg, torch.float32, st)
    o = _Obj(pkg, 2, 1, 1, 1, 1, torch.float32, A, Cn, st)
    losses = torch.zeros(2, dtype=torch.float32, device="cuda:0")
    with pytest.raises(pkg.PdecError, match="differs in dtype or size"):
        o.update(Cn, Cn, A, Cn, losses)
    A64, _ = _tiny_nets(pkg, torch.float64, st)
    with pytest.raises(pkg.PdecError, match="one dtype"):
        _Obj(pkg, 2, 1, 1, 1, 1, torch.float32, A64, Cn, st)
    with pytest.raises(pkg.PdecError, match="capacity 0 < 1"):
        _Obj(pkg, 0, 1, 1, 1, 1, torch.float32, A, Cn, st)
    o.close()
