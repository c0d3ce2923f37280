"""Population sweeps (population.py): members with their own hyper-parameters, the one-launch clone of a member's learner into
others, and exploit / explore on an evaluation's ranking.  Every member must stay bit for bit where a solo run of the same
agent would be -- through a clone, where load_agent of the source's save_agent file would put it."""
import copy
import ctypes as C
import warnings

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from population_sweep_ref import (SWEEP, Solo, adam_moments, assert_learner_equal, assert_member_equals_solo, beta_powers,  # noqa: E402
                                  filled_rows, flat_params, halve_learning_rates, make_member)

SEEDS = [3, 11, 29, 41]


def _population(pkg, setup, hypers, frozen=None, seeds=SEEDS, **kw):
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    members = [make_member(pkg, setup, s, s_upd, h, frozen, **kw) for s, h in zip(seeds, hypers)]
    return pkg.Population(setup, [a for a, _ in members], [h for _, h in members], stream_env=s_env, dtype=torch.float64)


def _stops(pkg, n, episodes=1):
    return [pkg.StopAfterEpisode(episodes) for _ in range(n)]


def _population_module(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + ".population")


def _kernel_name(pop):
    pol = pop.agents[0].policy
    name, lds = C.create_string_buffer(128), C.c_int64()
    hs = [getattr(pol, n).model.handle for n in ("behavior_actor", "behavior_critic", "target_actor", "target_critic")]
    assert pop.lib.pdec_debug_small_update_kernel(*hs, int(pol.update_loops), int(pol.batch_size), float(pol.rho_effective), 1,
                                                  name, 128, C.byref(lds)) == 0
    return name.value.decode()


# ---- 1. members with their own hyper-parameters equal their solo runs

@pytest.mark.parametrize("which", ["ks22_frozen", "ks22_moving", "ks22_three_layer", "keller_segel"])
def test_members_with_own_hyper_parameters_equal_solo_runs(pkg, which):
    setup, frozen, kernel = {
        "ks22_frozen": (lambda: pkg.KSSetup.KS22(), None, "ddpg_small2f_kernel"),
        "ks22_moving": (lambda: pkg.KSSetup.KS22(), False, "ddpg_small2_kernel<2,1,3,1>"),
        "ks22_three_layer": (lambda: pkg.KSSetup.KS22(drop_middle_layer=False), None, "ddpg_small_kernel"),
        "keller_segel": (lambda: pkg.KellerSegelSetup(), None, "ddpg_small2_kernel<13,12,3,1,5>"),
    }[which]
    setup = setup()
    hypers, seeds = SWEEP[:3], SEEDS[:3]
    pop = _population(pkg, setup, hypers, frozen)
    assert _kernel_name(pop).startswith(kernel), _kernel_name(pop)
    table = pop.hyper()
    assert table["gamma"].tolist() == [0.99, 0.95, 0.9] and table["act_limit"].tolist() == [1.0, 0.8, 1.0]
    assert table["rho"].tolist() == [0.995, 0.99, 0.98] and table["act_noise"].tolist() == [1.2, 0.9, 0.6]
    moving = which in ("ks22_moving", "keller_segel")
    assert table["rho_effective"].tolist() == (table["rho"].tolist() if moving else [1.0, 1.0, 1.0])
    assert np.array_equal(table["actor_lr"], setup.learning_rate * np.array([1.0, 0.5, 2.0]))
    assert np.array_equal(table["critic_lr"], setup.learning_rate_critic * np.array([1.0, 2.0, 0.5]))
    pop.run(_stops(pkg, 3))
    pop.set_hyper(1, actor_lr=table["actor_lr"][1] * 0.5, critic_lr=table["critic_lr"][1] * 0.5)
    pop.run(_stops(pkg, 3))
    torch.cuda.synchronize()
    for m, (s, h) in enumerate(zip(seeds, hypers)):
        solo = Solo(pkg, setup, s, h, frozen).run(pkg.StopAfterEpisode(1))
        if m == 1:
            halve_learning_rates(solo.agent)
        solo.run(pkg.StopAfterEpisode(1))
        assert solo.agent.policy._sample_off > 0                     # (updates ran)
        assert_member_equals_solo(pop, m, solo)
    # the sweep is a sweep: the members' learners differ from one another
    assert not np.array_equal(flat_params(pop.agents[0].policy.behavior_critic), flat_params(pop.agents[1].policy.behavior_critic))


# ---- 2. the ABI's default: launch-wide hyper-parameters, slots 11-14 not read

def test_member_hyper_off_ignores_the_slots(pkg):
    setup = pkg.KSSetup.KS22()
    pop = _population(pkg, setup, [None, None], seeds=SEEDS[:2])
    assert pop.lib.pdec_population_set_member_hyper(pop._h, 0) == 0
    garbage = np.full((2, 6), np.nan)
    garbage[:, 2:4] = 1e300
    pop._hyper_rows = lambda: garbage           # what the episode's row table takes slots 11-14 from
    pop.run(_stops(pkg, 2))
    torch.cuda.synchronize()
    for m in range(2):
        assert_member_equals_solo(pop, m, Solo(pkg, setup, SEEDS[m]).run(pkg.StopAfterEpisode(1)))


# ---- 3. refusals

def test_sweep_refusals(pkg):
    ks = pkg.KSSetup.KS22()
    with pytest.raises(pkg.PdecError, match=r"member 1.*quirk_frozen_targets"):
        s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
        mem = [make_member(pkg, ks, s, s_upd, None, fr) for s, fr in zip(SEEDS[:2], (True, False))]
        pkg.Population(ks, [a for a, _ in mem], [h for _, h in mem], stream_env=s_env)
    with pytest.raises(pkg.PdecError, match=r"member 2.*rho may differ between members only"):
        _population(pkg, ks, [SWEEP[0], SWEEP[1], dict(SWEEP[2], rho=1.0)], frozen=False)
    # ... also when it comes about between two runs
    pop = _population(pkg, ks, SWEEP[:2], frozen=False, seeds=SEEDS[:2])
    with pytest.raises(pkg.PdecError, match=r"member 1.*rho may differ between members only"):
        pop.set_hyper(1, rho=1.0)
    with pytest.raises(pkg.PdecError, match=r"member 1.*rho may differ between members only"):
        pop.run(_stops(pkg, 2))
    with pytest.raises(pkg.PdecError, match="update_loops"):
        s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
        mem = [make_member(pkg, ks, s, s_upd, h) for s, h in zip(SEEDS[:2], SWEEP[:2])]
        mem[1][0].policy.update_loops += 1
        pkg.Population(ks, [a for a, _ in mem], [h for _, h in mem], stream_env=s_env)


# ---- 4. clone == the checkpoint round-trip

def _take_over_by_checkpoint(pkg, path, src, dst, replay):
    """what Population.clone promises: load_agent(dst) of save_agent(src), dst keeping its own counters, streams and rng"""
    p = dst.agent.policy
    keep = (p.update_step, p.act_noise, p._noise_seed, p._noise_off, p._sample_seed, p._sample_off,
            copy.deepcopy(p.rng.bit_generator.state))
    pkg.checkpoint.save_agent(path, src.agent, with_trajectory=(replay == "copy"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", pkg.agent.TargetNetworkWarning)
        pkg.checkpoint.load_agent(path, dst.agent)
    p.update_step, p.act_noise, p._noise_seed, p._noise_off, p._sample_seed, p._sample_off = keep[:6]
    p.rng.bit_generator.state = keep[6]
    torch.cuda.synchronize()


@pytest.mark.parametrize("frozen,replay,length", [(True, "copy", None), (True, "keep", None), (False, "copy", None),
                                                  (False, "keep", None), (False, "copy", 320)])
def test_clone_equals_checkpoint_round_trip(pkg, tmp_path, frozen, replay, length):
    setup = pkg.KSSetup.KS22()
    kw = {} if length is None else dict(trajectory_length=length)
    pop = _population(pkg, setup, SWEEP, frozen, **kw)
    pop.run(_stops(pkg, 4, 2))
    torch.cuda.synchronize()
    tr0 = pop.agents[0].trajectory
    assert (tr0.n_rt > tr0.capacity) == (length is not None)          # the ring has wrapped, or not
    assert pop.clone({3: 0, 2: 0}, replay=replay) == [(2, 0), (3, 0)]
    before = pop.hyper()
    pop.run(_stops(pkg, 4, 2))
    torch.cuda.synchronize()
    assert all(np.array_equal(before[k], v) for k, v in pop.hyper().items())      # hyper-parameters stay the destination's
    twins = [Solo(pkg, setup, s, h, frozen, **kw).run(pkg.StopAfterEpisode(2)) for s, h in zip(SEEDS, SWEEP)]
    path = str(tmp_path / "member0.npz")
    for k in (2, 3):
        _take_over_by_checkpoint(pkg, path, twins[0], twins[k], replay)
    for m, tw in enumerate(twins):
        tw.run(pkg.StopAfterEpisode(2))
        assert_member_equals_solo(pop, m, tw, prefix_only=True)


# ---- 5. the clone kernel's edges

@pytest.mark.parametrize("three_layer", [False, True])
def test_clone_kernel_edges(pkg, three_layer):
    setup = pkg.KSSetup.KS22(drop_middle_layer=not three_layer)
    pop = _population(pkg, setup, SWEEP[:2], seeds=SEEDS[:2])
    pop.run([pkg.StopAfterEpisode(2), pkg.StopAfterEpisode(1)])      # 51 more update launches on the source: an odd number
    torch.cuda.synchronize()
    P = _population_module(pkg)
    rows = np.zeros((2, P.ROW), dtype=np.int64)
    assert pop.lib.pdec_population_bp_sel(pop._h, rows.ctypes.data_as(C.c_void_p), 0) == 0
    assert rows[0, P.BPA] != rows[1, P.BPA] and rows[0, P.BPC] != rows[1, P.BPC], rows[:, P.BPA:P.BPC + 1]
    src, dst = pop.agents[0], pop.agents[1]
    for n in ("behavior_actor", "behavior_critic"):
        assert getattr(src.policy, n).model.num_params % 4 != 0
    sentinel = -777.0
    for name in ("state", "action", "reward", "terminal"):
        getattr(dst.trajectory, name).fill_(sentinel)
    torch.cuda.synchronize()
    n_sa, n_rt = filled_rows(src.trajectory)
    rows_sa, rows_rt = np.array([0, 77], dtype=np.int64), np.array([0, 51], dtype=np.int64)
    assert rows_sa[1] < n_sa and rows_rt[1] < n_rt
    who = np.array([0, 0], dtype=np.int32)
    assert pop.lib.pdec_population_clone(pop._h, who.ctypes.data_as(C.c_void_p), rows_sa.ctypes.data_as(C.c_void_p),
                                         rows_rt.ctypes.data_as(C.c_void_p)) == 0
    torch.cuda.synchronize()
    assert_learner_equal(dst.policy, src.policy, "clone")
    for n in ("behavior_actor", "behavior_critic"):                  # (moments that are not all zero)
        assert all(x.any() for x in adam_moments(getattr(dst.policy, n)))
        assert np.all(beta_powers(getattr(dst.policy, n)) > 0)
    for name, k in (("state", 77), ("action", 77), ("reward", 51), ("terminal", 51)):
        d, s = getattr(dst.trajectory, name), getattr(src.trajectory, name)
        assert torch.equal(d[:k], s[:k]), name
        assert bool((d[k:] == sentinel).all()), name


# ---- 6. clone refusals

def test_clone_refusals(pkg):
    pop = _population(pkg, pkg.KSSetup.KS22(), SWEEP[:3], seeds=SEEDS[:3])
    with pytest.raises(pkg.PdecError, match="member 0 is both a source and a destination"):
        pop.clone({1: 0, 0: 2})
    with pytest.raises(pkg.PdecError, match="source 7 is not one of the 3 members"):
        pop.clone({1: 7})
    with pytest.raises(pkg.PdecError, match="source -1 is not one of the 3 members"):
        pop.clone({1: -1}, replay="keep")
    with pytest.raises(pkg.PdecError, match="destination 5"):
        pop.clone({5: 0})
    assert pop.clone({2: 2}) == []                                    # src[d] == d: keep


# ---- 7. exploit end to end

def test_exploit_end_to_end(pkg):
    setup = pkg.KSSetup.KS22()
    pop = _population(pkg, setup, SWEEP)
    pop.run(_stops(pkg, 4))
    res = pop.evaluate(n_inits=2)
    before = pop.hyper()
    with pytest.raises(pkg.PdecError, match="needs rng"):
        pop.exploit(res, frac=0.25, perturb=(0.8, 1.25))
    out = pop.exploit(res, frac=0.25, perturb=(0.8, 1.25), rng=np.random.default_rng(0))
    plan = pkg.plan_exploit(res["score"], res["order"], 0.25)
    assert len(plan) >= 1 and [(o["dst"], o["src"]) for o in out] == plan
    after = pop.hyper()
    touched = {d for d, _ in plan}
    for d, s in plan:
        for k in ("gamma", "rho", "act_limit"):
            assert after[k][d] == before[k][s], (d, s, k)
        for k in ("actor_lr", "critic_lr", "act_noise"):
            assert after[k][d] in (before[k][s] * 0.8, before[k][s] * 1.25), (d, s, k)
        assert out[[o["dst"] for o in out].index(d)]["hyper"] == {k: after[k][d] for k in out[0]["hyper"]}
        assert_learner_equal(pop.agents[d].policy, pop.agents[s].policy, (d, s))
    for m in set(range(4)) - touched:
        assert all(after[k][m] == before[k][m] for k in before), m
    pop.run(_stops(pkg, 4))
    torch.cuda.synchronize()
    for m, hk in enumerate(pop.hooks):
        assert len(hk.rewards) == 2 and np.isfinite(hk.rewards[-1]), (m, hk.rewards)
