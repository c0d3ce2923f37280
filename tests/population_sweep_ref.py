"""What the population-sweep tests share: members with their own hyper-parameters, their solo twins, and the statement that a
member of a Population ended bit for bit where a solo agent ended (the comparison of tests/test_gpu_population.py, restated
here so that no test file imports another)."""
import ctypes as C
import warnings

import numpy as np
import torch

NETS = ("behavior_actor", "behavior_critic", "target_actor", "target_critic")

# member k of a sweep: gamma, Polyak rho, factors on the setup's two learning rates, act_noise, act_limit
SWEEP = [dict(gamma=0.99, rho=0.995, lr=1.0, lr_critic=1.0, act_noise=1.2, act_limit=1.0),
         dict(gamma=0.95, rho=0.99, lr=0.5, lr_critic=2.0, act_noise=0.9, act_limit=0.8),
         dict(gamma=0.9, rho=0.98, lr=2.0, lr_critic=0.5, act_noise=0.6, act_limit=1.0),
         dict(gamma=0.97, rho=0.97, lr=1.5, lr_critic=1.5, act_noise=1.0, act_limit=0.9)]


def make_member(pkg, setup, seed, s_upd, hyper=None, frozen=None, random_init=True, **kw):
    """an agent and its hook as the existing population tests make them, with `hyper` (an entry of SWEEP) instead of the setup's
    values; frozen: quirk_frozen_targets (None: the setup's regime)"""
    if hyper is not None:
        kw.update(gamma=hyper["gamma"], rho=hyper["rho"], learning_rate=setup.learning_rate * hyper["lr"],
                  learning_rate_critic=setup.learning_rate_critic * hyper["lr_critic"], act_limit=hyper["act_limit"])
    if frozen is not None:
        kw["quirk_frozen_targets"] = frozen
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", pkg.agent.TargetNetworkWarning)
        agent = pkg.create_agent(setup=setup, B=1, rng=np.random.default_rng(seed), noise_seed=seed, stream=s_upd, **kw)
    hook = pkg.PDEhook(min_best_episode=1, use_random_init=random_init, init_seed=seed)
    agent.policy.act_noise = hyper["act_noise"] if hyper is not None else setup.act_noise
    return agent, hook


class Solo:
    """a solo twin: its own environment and streams"""

    def __init__(self, pkg, setup, seed, hyper=None, frozen=None, **kw):
        self.pkg = pkg
        self.s_env, self.s_upd = torch.cuda.Stream(), torch.cuda.Stream()
        self.env = pkg.PDEenv(setup, B=1, dtype=torch.float64, stream=self.s_env)
        self.agent, self.hook = make_member(pkg, setup, seed, self.s_upd, hyper, frozen, **kw)

    def run(self, stop):
        self.pkg.run(self.agent, self.env, stop, self.hook)
        torch.cuda.synchronize()
        return self


def halve_learning_rates(agent):
    for n in ("behavior_actor", "behavior_critic"):
        getattr(agent.policy, n).optimizer.eta *= 0.5


def beta_powers(nna):
    bp = (C.c_double * 2)()
    m = nna.model
    assert m.lib.pdec_adam_get_state(m.handle, None, None, bp) == 0
    return np.array([bp[0], bp[1]])


def adam_moments(nna):
    m = nna.model
    k = m.num_params
    a, b = (C.c_float * k)(), (C.c_float * k)()
    assert m.lib.pdec_adam_get_state(m.handle, a, b, None) == 0
    return np.frombuffer(bytes(a), dtype=np.uint32), np.frombuffer(bytes(b), dtype=np.uint32)


def flat_params(nna):
    return np.concatenate([np.asarray(x, dtype=np.float32).ravel() for x in nna.model.params()]).view(np.uint32)


def filled_rows(tr):
    """rows of the state / action and of the reward / terminal traces that have been written"""
    return min(tr.n_sa, tr.capacity + tr.stride), min(tr.n_rt, tr.capacity)


def assert_learner_equal(pd, ps, tag):
    """the four networks, beta powers (bit patterns) and ADAM moments of two policies"""
    for n in NETS:
        assert np.array_equal(flat_params(getattr(pd, n)), flat_params(getattr(ps, n))), (tag, n)
        assert np.array_equal(beta_powers(getattr(pd, n)).view(np.uint64), beta_powers(getattr(ps, n)).view(np.uint64)), (tag, n)
    for n in NETS[:2]:
        for x, y in zip(adam_moments(getattr(pd, n)), adam_moments(getattr(ps, n))):
            assert np.array_equal(x, y), (tag, n, "adam")


def assert_member_equals_solo(pop, m, solo, prefix_only=False):
    """member m of `pop` against the Solo twin: counters, the four traces (prefix_only: their filled prefix), the four networks,
    beta-power bit patterns, ADAM moments, environment row, hook rewards, best episode and best actor"""
    ad, hd, as_, hs = pop.agents[m], pop.hooks[m], solo.agent, solo.hook
    pd, ps, td, ts = ad.policy, as_.policy, ad.trajectory, as_.trajectory
    assert (td.n_sa, td.n_rt, pd.update_step, pd._noise_off, pd._sample_off) == \
        (ts.n_sa, ts.n_rt, ps.update_step, ps._noise_off, ps._sample_off), m
    n_sa, n_rt = filled_rows(td)
    for name in ("state", "action", "reward", "terminal"):
        x, y = getattr(td, name), getattr(ts, name)
        if prefix_only:
            k = n_sa if name in ("state", "action") else n_rt
            x, y = x[:k], y[:k]
        assert torch.equal(x, y), (m, name)
    assert_learner_equal(pd, ps, m)
    assert torch.equal(pop.env.y[m], solo.env.y[0]) and torch.equal(pop.env.state[m], solo.env.state[0]), m
    assert np.array_equal(np.asarray(hd.rewards), np.asarray(hs.rewards)), m
    assert (hd.bestepisode, hd.bestreward, len(hd.bestDF)) == (hs.bestepisode, hs.bestreward, len(hs.bestDF)), m
    for rd, rs in zip(hd.bestDF, hs.bestDF):
        assert rd["timestep"] == rs["timestep"]
        for k in ("action", "p", "y", "reward"):
            assert np.array_equal(rd[k], rs[k]), (m, k)
    for x, y in zip(hd.bestNNA.model.params(), hs.bestNNA.model.params()):
        assert np.array_equal(x, y), m
