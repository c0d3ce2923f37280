"""The fp64 checks of the small DDPG update (tests/small_update_ref.py) tell a right launch from a wrong one: they accept
an fp32 NumPy run of the oracle's update and reject each of a list of plausible kernel bugs, built by perturbing that
run.  Host only (no GPU)."""
import numpy as np
import pytest

from oracle import nn
from small_update_ref import B1, B2, EPS, check_launch, fresh_snap, minibatches

GAMMA, RHO = 0.99, 0.995


def _adam32(P, m, v, bp, g, eta):
    """one Flux ADAM step in fp32 (oracle.nn.Adam's arithmetic); bp = the beta powers of this step"""
    f = np.float32
    m[:] = [f(B1) * mi + f(1 - B1) * gi for mi, gi in zip(m, g)]
    v[:] = [f(B2) * vi + f(1 - B2) * gi * gi for vi, gi in zip(v, g)]
    P[:] = [(p - mi / f(1 - bp[0]) / (np.sqrt(vi / f(1 - bp[1])) + f(EPS)) * f(eta)).astype(np.float32)
            for p, mi, vi in zip(P, m, v)]


def fp32_launch(before, mbs, acts_a, acts_c, rho, quirk, eta_a, eta_c, fault=None):
    """the launch as the oracle runs it in fp32 (one ddpg_update per minibatch), optionally with one bug built in"""
    st = before.copy()
    for k, (s, a, r, t, sn) in enumerate(mbs):
        if fault == "s_next_from_s_slot":
            sn = s
        if fault == "no_terminal_mask":
            t = np.zeros_like(t)
        q = (not quirk) if fault == "quirk_inverted" else quirk
        out = nn.ddpg_losses_and_grads(st.A, st.C, st.At, st.Ct, acts_a, acts_c, s, a, r, t, sn, np.float32(GAMMA), q)
        gC = out["gC"]
        if fault == "minibatch_dropped" and k == 1:
            gC = [np.zeros_like(g) for g in gC]
        if fault == "hidden_bias_grad_zeroed":
            gC[1] = gC[1].copy()
            gC[1][np.argmax(np.abs(gC[1]))] = 0
        C_old = [p.copy() for p in st.C]
        advance = not (fault == "beta_powers_once_per_launch" and k > 0)
        bpC = st.bpC.copy()
        _adam32(st.C, st.mC, st.vC, bpC, gC, eta_c)
        out2 = nn.actor_grads(st.A, C_old if fault == "actor_through_pre_update_critic" else st.C, acts_a, acts_c, s)
        bpA = st.bpA.copy()
        _adam32(st.A, st.mA, st.vA, bpA, out2["gA"], eta_a)
        if advance:
            st.bpC, st.bpA = st.bpC * np.array([B1, B2]), st.bpA * np.array([B1, B2])
        r_eff = RHO if fault == "polyak_at_rho_1" else rho
        st.At, st.Ct = nn.polyak(st.At, st.A, np.float32(r_eff)), nn.polyak(st.Ct, st.C, np.float32(r_eff))
        st.losses = (out["critic_loss"], out2["actor_loss"])
    return st


def _setup(ns=2, na=1, ha=12, hc=40, Bu=3, loops=1, seed=0):
    rng = np.random.default_rng(seed)
    da, aa = [ns, ha, na], [nn.RELU, nn.TANH]
    dc, ac = [ns + na, hc, 1], [nn.RELU, nn.IDENT]

    def net(d):
        P = nn.glorot_uniform(rng, d, np.float32)
        return [p if i % 2 == 0 else (rng.standard_normal(p.shape) * 0.1).astype(np.float32) for i, p in enumerate(P)]
    A, C = net(da), net(dc)
    At, Ct = [p + np.float32(0.01) for p in A], [p - np.float32(0.01) for p in C]
    n = 64
    S = rng.standard_normal((n, ns)).astype(np.float32)
    Aa = rng.uniform(-1, 1, (n, na)).astype(np.float32)
    R = -rng.uniform(0, 1, n).astype(np.float32)
    T = np.zeros(n, np.float32)
    slots = np.stack([rng.permutation(n)[:loops * Bu] for _ in range(3)]).reshape(3, loops, Bu)
    T[slots[1, :, ::2]] = 1                     # terminal flags in the drawn slots
    return fresh_snap(A, C, At, Ct), minibatches(S, Aa, R, T, slots), aa, ac


# (fault, launch): "one" = one update at real learning rates, "eta0" = three updates at eta = 0
FAULTS = [
    ("minibatch_dropped", "eta0"),
    ("no_terminal_mask", "one"),
    ("quirk_inverted", "one"),
    ("actor_through_pre_update_critic", "one"),
    ("s_next_from_s_slot", "one"),
    ("hidden_bias_grad_zeroed", "one"),
    ("polyak_at_rho_1", "one"),
    ("beta_powers_once_per_launch", "eta0"),
]


def _launch(kind, rho, quirk, fault=None):
    loops, eta = (1, (5e-4, 1e-3)) if kind == "one" else (3, (0.0, 0.0))
    st, mbs, aa, ac = _setup(loops=loops)
    if kind == "one":                          # a continuation: nonzero moments and advanced beta powers
        st = fp32_launch(st, _setup(loops=4, seed=1)[1], aa, ac, rho, quirk, *eta)
    after = fp32_launch(st, mbs, aa, ac, rho, quirk, *eta, fault=fault)
    return check_launch(st, after, mbs, aa, ac, GAMMA, rho, quirk, *eta)


@pytest.mark.parametrize("kind", ["one", "eta0"])
@pytest.mark.parametrize("rho", [1.0, RHO])
@pytest.mark.parametrize("quirk", [True, False])
def test_checks_accept_the_fp32_oracle(kind, rho, quirk):
    assert _launch(kind, rho, quirk) == []


@pytest.mark.parametrize("fault,kind", FAULTS)
def test_checks_reject_a_faulty_update(fault, kind):
    rho = 1.0 if fault == "polyak_at_rho_1" else RHO
    errs = _launch(kind, rho, True, fault)
    assert errs, fault
