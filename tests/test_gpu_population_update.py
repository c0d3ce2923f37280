"""The members' update launch (pdec_population_update: sm_member_begin + every kernel of the small-update dispatch on a grid of
M workgroups, csrc/mlp_small.hip) driven through the C ABI on raw networks, traces and a row table the test writes -- no
environment, no Population object.  Cases and member roles: population_update_cases.py (claims: test_population_update_table.py).

Per case and target form, ONE launch of M = 6 workgroups, then a second one on the rows the first left:
  * a member that updates equals, bit for bit, its solo twin (the same seeds) called through pdec_ddpg_update_small_rng with the
    arguments Agent.update_small_rng passes for the member's counters -- the same kernel function, so no tolerance;
  * and it is right against fp64: the launch makes LOOPS = 2 updates at real step sizes, and small_update_ref.check_launch
    judges one update at a time (its closed forms: one update, or any number at eta = 0), so a third rig from the same seeds
    (the stepper) makes the launch's updates as LOOPS solo launches of one minibatch each on the slots of
    oracle.rng.sample_slots, every one of them checked by check_launch with its own tolerances, and must end bit for bit
    where the member ends (one launch of L loops == L launches of one, in-kernel slots == host slots: both pinned for the
    solo call by test_gpu_small_update.py);
  * its row: POP_SAMPLE + ceil(LOOPS Bu / 4), POP_BPA / POP_BPC flipped, the 13 other slots as they were;
  * a member that does not update keeps parameters, moments, BOTH beta-power slots of both networks, losses and its row byte for byte;
  * nobody's traces change.
Without per-member hyper-parameters slots 11..14 of every row hold NaN bit patterns: the launch must not read them.
With them (the kernels small_serves_member_hyper accepts) the updating members differ in gamma, rho (moving targets), eta_a and
eta_c; one of them has both step sizes 0 and keeps its behaviour parameters while m and v move.  The four bounded instantiations
refuse pdec_population_set_member_hyper by name."""
import ctypes as C_

import numpy as np
import pytest

import population_update_cases as pc
from small_update_ref import check_launch, minibatches
from test_gpu_small_update import Rig, _reach, _same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _solo_rng(rig, mb, offset, quirk, gamma, rho, eta_a, eta_c):
    """the solo call of Agent.update_small_rng for member mb's counters: n_valid = len(trajectory) = min(n_rt, cap)"""
    A, C, At, Ct = rig.nets
    L = rig.L
    torch.cuda.synchronize()
    L.check(A.lib.pdec_ddpg_update_small_rng(A.handle, C.handle, At.handle, Ct.handle, *(L.ptr(x) for x in rig.dev), pc.LOOPS, rig.Bu,
                                             mb.seed, offset, pc.n_valid(mb), mb.n_rt, pc.CAP, pc.STRIDE, gamma, rho, quirk, eta_a, eta_c,
                                             L.ptr(rig.losses)))


def _solo_slots(rig, slots, quirk, gamma, rho, eta_a, eta_c):
    """pdec_ddpg_update_small on host slots [3, loops, Bu] (Rig.launch with the member's own gamma and rho)"""
    A, C, At, Ct = rig.nets
    L = rig.L
    d = torch.as_tensor(np.ascontiguousarray(slots, dtype=np.int32), device="cuda:0")
    torch.cuda.synchronize()
    rig._keep.append(d)
    L.check(A.lib.pdec_ddpg_update_small(A.handle, C.handle, At.handle, Ct.handle, *(L.ptr(x) for x in rig.dev),
                                         C_.c_void_p(d[0].data_ptr()), C_.c_void_p(d[1].data_ptr()), C_.c_void_p(d[2].data_ptr()),
                                         int(slots.shape[1]), rig.Bu, gamma, rho, quirk, eta_a, eta_c, L.ptr(rig.losses)))


def _identical(a, b):
    """byte equality of two snapshots (NaN losses of a learner that never updated included): the first field that differs"""
    for f in ("A", "C", "At", "Ct", "mA", "vA", "mC", "vC"):
        for x, y in zip(getattr(a, f), getattr(b, f)):
            if x.shape != y.shape or x.tobytes() != y.tobytes():
                return f
    if a.bpA.tobytes() != b.bpA.tobytes() or a.bpC.tobytes() != b.bpC.tobytes():
        return "beta powers"
    if np.array(a.losses, np.float32).tobytes() != np.array(b.losses, np.float32).tobytes():
        return "losses"
    return None


class Members:
    """M member rigs joined in a population, their solo twins and, for the members that update, their steppers"""

    def __init__(self, pkg, case, quirk, hyper):
        self.case, self.quirk, self.L = case, quirk, pkg._lib
        self.mbs = pc.members(case)
        self.h = None
        self.rigs, self.twins, self.steppers = [], [], {}
        mk = lambda m: Rig(pkg, case, seed=10 + m, n=pc.CAP, stride=pc.STRIDE)      # noqa: E731
        for m, mb in enumerate(self.mbs):
            self.rigs.append(mk(m))
            self.twins.append(mk(m))
            if mb.updates:
                self.steppers[m] = mk(m)
        self.rho = self.rigs[0].rho
        # launch-wide values, or each member's own
        self.hyper = pc.hyper(case) if hyper else np.tile([pc.GAMMA0, self.rho, pc.ETA_A0, pc.ETA_C0], (pc.M, 1))
        for m, mb in enumerate(self.mbs):       # the aged members: three solo launches before the population exists
            if mb.aged:
                for r in (self.rigs[m], self.twins[m], self.steppers[m]):
                    for _ in range(3):
                        r.launch(r.slots(pc.LOOPS), quirk)
        lib = self.lib = self.rigs[0].nets[0].lib
        A0 = self.rigs[0].nets[0]
        served = C_.c_int(0)
        f64 = self.L.dtype_code(torch.float64)
        self.L.check(lib.pdec_step_glue_served(A0.handle, A0.handle, f64, 1, pc.COLS, pc.COLS, C_.byref(served)))
        assert served.value == 1                # what pdec_population_create requires of member 0's actor
        H = self.L.Handle * pc.M
        hs = [H(*[int(getattr(r.nets[k].handle, "value", r.nets[k].handle)) for r in self.rigs]) for k in range(4)]
        traces = (C_.c_void_p * (4 * pc.M))(*[t.data_ptr() for r in self.rigs for t in r.dev])
        seeds = (C_.c_uint64 * (2 * pc.M))(*[s for m, mb in enumerate(self.mbs) for s in (900 + m, mb.seed)])
        losses = (C_.c_void_p * pc.M)(*[r.losses.data_ptr() for r in self.rigs])
        self.rows_dev = torch.zeros((pc.M, pc.ROW), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        h = self.L.Handle()
        g0, r0, ea0, ec0 = self.hyper[0]
        self.L.check(lib.pdec_population_create(C_.byref(h), pc.M, hs[0], hs[1], hs[2], hs[3], traces, seeds, losses, f64, pc.COLS, pc.CAP,
                                                pc.STRIDE, pc.LOOPS, self.rigs[0].Bu, g0, r0, quirk, ea0, ec0, pc.AFTER_ROWS, pc.FREQ,
                                                pc.START_STEPS, self.L.ptr(self.rows_dev)))
        self.h = h
        self.rows = pc.rows(case, hyper)
        self._bp_sel(self.rows, 0)              # as population.py does before it uploads an episode's rows
        for m, mb in enumerate(self.mbs):
            assert self.rows[m, [pc.BPA, pc.BPC]].tolist() == ([1, 1] if mb.aged else [0, 0]), m

    def _bp_sel(self, rows_host, set_):
        assert rows_host.dtype == np.int64 and rows_host.flags.c_contiguous
        self.L.check(self.lib.pdec_population_bp_sel(self.h, rows_host.ctypes.data_as(C_.c_void_p), set_))

    def upload(self):
        self.rows_dev.copy_(torch.from_numpy(self.rows))
        torch.cuda.synchronize()

    def launch(self):
        """one pdec_population_update, settled as population.py settles an episode: rows read back, slots adopted"""
        torch.cuda.synchronize()
        self.L.check(self.lib.pdec_population_update(self.h))
        torch.cuda.synchronize()
        self.rows = self.rows_dev.cpu().numpy().copy()
        self._bp_sel(self.rows, 1)
        return self.rows

    def beta_powers(self):
        """bytes [M][actor, critic][slot 0, slot 1] of every member's double-buffered beta powers: the current slot through
        pdec_adam_get_state, the other one with the slots flipped on the host and put back"""
        def cur():
            out = []
            for r in self.rigs:
                pair = []
                for net in (r.nets[0], r.nets[1]):
                    bp = (C_.c_double * 2)()
                    self.L.check(net.lib.pdec_adam_get_state(net.handle, None, None, bp))
                    pair.append(bytes(bp))
                out.append(pair)
            return out
        torch.cuda.synchronize()
        here = cur()
        flipped = self.rows.copy()
        flipped[:, [pc.BPA, pc.BPC]] ^= 1
        self._bp_sel(flipped, 1)
        there = cur()
        self._bp_sel(self.rows, 1)
        out = []
        for m in range(pc.M):
            pair = []
            for k, slot in enumerate((pc.BPA, pc.BPC)):
                two = [None, None]
                two[int(self.rows[m, slot])], two[int(self.rows[m, slot]) ^ 1] = here[m][k], there[m][k]
                pair.append(two)
            out.append(pair)
        return out

    def traces(self):
        torch.cuda.synchronize()
        return [[t.cpu().numpy().tobytes() for t in r.dev] for r in self.rigs]

    def snaps(self):
        return [r.snap() for r in self.rigs]

    def twin_launch(self, m, launch):
        g, rho, ea, ec = self.hyper[m]
        _solo_rng(self.twins[m], self.mbs[m], self.mbs[m].offset + launch * pc.dsample(self.case), self.quirk, g, rho, ea, ec)

    def stepper_launch(self, m, launch):
        """the launch's updates one at a time on the oracle's slots, each judged against fp64"""
        st, (g, rho, ea, ec) = self.steppers[m], self.hyper[m]
        s = pc.slots(self.case, self.mbs[m], launch)
        for k in range(pc.LOOPS):
            before = st.snap()
            _solo_slots(st, s[:, k:k + 1], self.quirk, g, rho, ea, ec)
            errs = check_launch(before, st.snap(), minibatches(st.S, st.Aa, st.R, st.T, s[:, k:k + 1]), st.aa, st.ac, g, rho,
                                self.quirk, ea, ec)
            assert not errs, (self.mbs[m].role, "update", k, errs)

    def close(self):
        torch.cuda.synchronize()
        if self.h is not None:
            self.lib.pdec_destroy(self.h)
        for r in self.rigs + self.twins + list(self.steppers.values()):
            r.close()


def _check_launch_of_members(P, launch, rows_before, snaps0, bp0, traces0):
    """everything one population launch must have done, `launch` = 0, 1: the launches so far; *0: the state before the first"""
    case, mbs = P.case, P.mbs
    bp_before = P.beta_powers()
    rows = P.launch()
    want = pc.rows_after(case, rows_before)
    for m, mb in enumerate(mbs):
        changed = np.flatnonzero(rows[m] != rows_before[m]).tolist()
        assert changed == (sorted(pc.MOVES) if mb.updates else []), (m, mb.role, changed)
        assert np.array_equal(rows[m], want[m]), (m, mb.role, rows[m], want[m])
    assert P.traces() == traces0
    bp = P.beta_powers()
    for m, mb in enumerate(mbs):
        got = P.rigs[m].snap()
        if not mb.updates:
            diff = _identical(got, snaps0[m])
            assert diff is None, (m, mb.role, diff)
            assert bp[m] == bp0[m], (m, mb.role)
            continue
        P.twin_launch(m, launch)
        diff = _same(got, P.twins[m].snap())
        assert diff is None, (m, mb.role, "solo twin", diff)
        # the slot the launch read stays; the one it wrote is the twin's current one, whose value the comparison above and the
        # stepper's check_launch pin -- the inequality below is a sanity check only (the slot was written at all)
        for k, slot in enumerate((pc.BPA, pc.BPC)):
            was = int(rows_before[m, slot])
            assert bp[m][k][was] == bp_before[m][k][was], (m, mb.role, k)
            assert bp[m][k][was ^ 1] != bp_before[m][k][was], (m, mb.role, k)
    return rows


@pytest.mark.parametrize("case", list(pc.CASES))
@pytest.mark.parametrize("quirk", [1, 0])
def test_member_launch_equals_solo_twins_and_fp64(pkg, case, quirk):
    P = Members(pkg, case, quirk, hyper=False)
    try:
        _reach(P.rigs[0], pc.LOOPS, sampling=True)
        P.upload()
        rows0, snaps0, bp0, traces0 = P.rows.copy(), P.snaps(), P.beta_powers(), P.traces()
        assert np.isnan(rows0[:, pc.GAMMA:pc.ETA_C + 1].view(np.float64)).all()
        rows1 = _check_launch_of_members(P, 0, rows0, snaps0, bp0, traces0)
        for m, mb in enumerate(P.mbs):
            if mb.updates:
                P.stepper_launch(m, 0)
                diff = _same(P.rigs[m].snap(), P.steppers[m].snap())
                assert diff is None, (m, mb.role, "stepper", diff)
                assert _identical(P.rigs[m].snap(), snaps0[m]) is not None      # it did update
        # the second launch, on the rows the first left on the device: the same members fire again (ustep has not moved) at
        # the advanced offset and the flipped slots
        rows2 = _check_launch_of_members(P, 1, rows1, snaps0, bp0, traces0)
        assert np.array_equal(rows2, pc.rows_after(case, rows0, 2))
    finally:
        P.close()


HYPER_CASES = [c for c in pc.CASES if pc.serves_member_hyper(c)]
BOUNDED_CASES = [c for c in pc.CASES if not pc.serves_member_hyper(c)]


@pytest.mark.parametrize("case", HYPER_CASES)
@pytest.mark.parametrize("quirk", [1, 0])
def test_member_hyper_parameters_are_each_member_s_own(pkg, case, quirk):
    P = Members(pkg, case, quirk, hyper=True)
    try:
        _reach(P.rigs[0], pc.LOOPS, sampling=True)
        assert P.lib.pdec_population_set_member_hyper(P.h, 1) == 0, P.lib.pdec_last_error().decode()
        P.upload()
        rows0, snaps0, bp0, traces0 = P.rows.copy(), P.snaps(), P.beta_powers(), P.traces()
        assert np.array_equal(rows0[:, pc.GAMMA:pc.ETA_C + 1].view(np.float64), pc.hyper(case))
        _check_launch_of_members(P, 0, rows0, snaps0, bp0, traces0)
        for m, mb in enumerate(P.mbs):
            if not mb.updates:
                continue
            P.stepper_launch(m, 0)              # check_launch with the member's own gamma, rho, eta_a, eta_c
            got = P.rigs[m].snap()
            diff = _same(got, P.steppers[m].snap())
            assert diff is None, (m, mb.role, "stepper", diff)
            if P.hyper[m, 2] == 0.0 and P.hyper[m, 3] == 0.0:       # no step: behaviour parameters stay, the moments move
                for f in ("A", "C"):
                    assert all(np.array_equal(x, y) for x, y in zip(getattr(got, f), getattr(snaps0[m], f))), (m, f)
                for f in ("mA", "vA", "mC", "vC"):
                    assert any(not np.array_equal(x, y) for x, y in zip(getattr(got, f), getattr(snaps0[m], f))), (m, f)
            else:
                assert any(not np.array_equal(x, y) for x, y in zip(got.A, snaps0[m].A)), m
                assert any(not np.array_equal(x, y) for x, y in zip(got.C, snaps0[m].C)), m
    finally:
        P.close()


@pytest.mark.parametrize("case", BOUNDED_CASES)
def test_bounded_kernels_refuse_member_hyper_by_name(pkg, case):
    """(their launch-wide result under NaN bit patterns in slots 11..14 is test_member_launch_equals_solo_twins_and_fp64's)"""
    P = Members(pkg, case, 0, hyper=False)
    try:
        _reach(P.rigs[0], pc.LOOPS, sampling=True)
        assert pc.kernel_of(case) in pc.BOUNDED
        assert P.lib.pdec_population_set_member_hyper(P.h, 1) != 0
        assert pc.kernel_of(case) in P.lib.pdec_last_error().decode()
        assert P.lib.pdec_population_set_member_hyper(P.h, 0) == 0
    finally:
        P.close()
