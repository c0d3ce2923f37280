"""Populations of fluid learners (population.py with FluidSetup): M = 3 members with different seeds, act_noise and act_limit,
trained side by side, against their three solo `run()`s -- bit for bit, compared as integer views so that NaN rows compare too.

Setups: FluidSetup(nx=64 | 128, oversampling=8, te=0.2, start_steps=0, update_after=2): 11-step episodes (the step loop's sum of
ten 0.02 stays below 0.2), the generic kernels at 64 and the wave-register kernels of the reference's grid at 128, updates from
the third step of the first episode on; hooks from make_hook(), random initial fields on, every member's own init_rng.  The
replay is 8192 entries long (4 episodes fill 2816), which changes no number and keeps the comparisons of the traces quick.

The three kinds of episode.  The random fields themselves have neighbour differences of 9 to 45 (a Taylor vortex of radius
L / 20 on these grids, computed on the host: 18 to 45 at 64 x 64, 8.9 to 23 at 128 x 128), so whether an episode that ended
early counts as errored is decided by its initial field and by what the member's forcing leaves of it.  MEMBERS and MAX_VALUE
were found on an MI355X; the members' solo runs of four episodes there, at both grids:
  * (seed 3, act_noise 0.1, act_limit 1): all four episodes run to the time-out;
  * (seed 13, act_noise 100, act_limit 5): saturated actions of +-5; every episode ends at its second step on the action
    penalty (largest |reward| 0.29 to 0.38 > 0.25).  Largest neighbour difference of the final fields at 128 x 128: 17.68,
    20.55, 9.62, 13.84 -- episodes 1, 2 and 4 are errored, episode 3 ended early and is not; at 64 x 64: 34.66, 39.84, 18.95,
    26.76 -- all four errored;
  * (seed 29, act_noise 1e4, act_limit 1000): saturated actions of +-1000; every episode ends early and none is counted as
    errored, at both grids -- error_detection's answer for its final fields (a field that is no longer finite yields False;
    whether these are was not looked at).  (An act_limit of 1000 under the default noise of 1.2 clips nothing: such a member
    ran to the time-out like the tame one.)
So the counts (time-out, ended early and not errored, ended early and errored) over the three solo runs were (4, 4, 4) at
64 x 64 and (4, 5, 3) at 128 x 128, and the test asserts that every kind occurs before it compares anything."""
import copy
import ctypes as C
import warnings

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# (seed, act_noise, act_limit): tame; saturated small actions (ends early on the action penalty, hardly changes the field);
# act_limit of the order 1e3 with the noise to reach it (the forcing roughens the field within one step)
MEMBERS = [(3, 0.1, 1.0), (13, 100.0, 5.0), (29, 1.0e4, 1000.0)]
MAX_VALUE = 0.25
EPISODES = 4
_SETUPS, _SOLOS = {}, {}


def _setup(pkg, nx):
    if nx not in _SETUPS:
        _SETUPS[nx] = pkg.FluidSetup(nx=nx, oversampling=8, te=0.2, start_steps=0, update_after=2, max_value=MAX_VALUE)
    return _SETUPS[nx]


def _make(pkg, setup, k, s_upd):
    seed, noise, limit = MEMBERS[k]
    agent = pkg.create_agent(setup=setup, B=1, rng=np.random.default_rng(seed), noise_seed=seed, stream=s_upd, trajectory_length=8192)
    agent.policy.act_noise, agent.policy.act_limit = noise, limit
    hook = setup.make_hook(min_best_episode=1, use_random_init=True, init_seed=seed, init_rng=np.random.default_rng(seed))
    return agent, hook


class _Solo:
    def __init__(self, pkg, setup, k):
        self.s_env, self.s_upd = torch.cuda.Stream(), torch.cuda.Stream()
        self.env = pkg.PDEenv(setup, B=1, dtype=torch.float64, stream=self.s_env)
        self.agent, self.hook = _make(pkg, setup, k, self.s_upd)
        self.pkg = pkg

    def run(self, stop):
        self.pkg.run(self.agent, self.env, stop, self.hook)
        torch.cuda.synchronize()
        return self


def _solos(pkg, nx, key, stops):
    """the members' solo runs, made once per (grid, stop conditions) and left unchanged"""
    if (nx, key) not in _SOLOS:
        _SOLOS[nx, key] = [_Solo(pkg, _setup(pkg, nx), k).run(stops(k)) for k in range(len(MEMBERS))]
    return _SOLOS[nx, key]


def _population(pkg, setup, three_pipes=False, **kw):
    if three_pipes:               # env, update and the fluid step's part stream on three compute pipes
        s_env, s_upd, s_part = pkg.make_streams((-1, 0, -1))
        kw["part_streams"] = [s_part]
    else:
        s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    members = [_make(pkg, setup, k, s_upd) for k in range(len(MEMBERS))]
    return pkg.Population(setup, [a for a, _ in members], [h for _, h in members], stream_env=s_env, dtype=torch.float64, **kw)


def _raw(x):
    """the bytes of a tensor / array / list of floats (NaN-safe equality)"""
    if isinstance(x, torch.Tensor):
        return x.detach().contiguous().cpu().numpy().tobytes()
    return np.ascontiguousarray(np.asarray(x)).tobytes()


def _adam(nna):
    m = nna.model
    k = sum(int(np.asarray(x).size) for x in m.params())
    a, b, bp = (C.c_float * k)(), (C.c_float * k)(), (C.c_double * 2)()
    assert m.lib.pdec_adam_get_state(m.handle, a, b, bp) == 0
    return bytes(a), bytes(b), bytes(bp)


def _assert_member_equals_solo(pop, m, solo, next_draw=True):
    ad, hd, as_, hs = pop.agents[m], pop.hooks[m], solo.agent, solo.hook
    pd, ps, td, ts = ad.policy, as_.policy, ad.trajectory, as_.trajectory
    assert (td.n_sa, td.n_rt, pd.update_step, pd._noise_off, pd._sample_off) == \
        (ts.n_sa, ts.n_rt, ps.update_step, ps._noise_off, ps._sample_off), m
    for name in ("state", "action", "reward", "terminal"):
        assert _raw(getattr(td, name)) == _raw(getattr(ts, name)), (m, name)
    for n in ("behavior_actor", "behavior_critic", "target_actor", "target_critic"):
        for x, y in zip(getattr(pd, n).model.params(), getattr(ps, n).model.params()):
            assert _raw(x) == _raw(y), (m, n)
        assert _adam(getattr(pd, n)) == _adam(getattr(ps, n)), (m, n, "adam")
    assert _raw(pop.env.y[m]) == _raw(solo.env.y[0]) and _raw(pop.env.state[m]) == _raw(solo.env.state[0]), m
    assert _raw(hd.rewards) == _raw(hs.rewards) and _raw(hd.rewards_compare) == _raw(hs.rewards_compare), m
    assert (hd.ep, hd.bestepisode, hd._init_off) == (hs.ep, hs.bestepisode, hs._init_off), m
    assert _raw([hd.bestreward]) == _raw([hs.bestreward]), m
    assert hd.errored_episodes == hs.errored_episodes, (m, hd.errored_episodes, hs.errored_episodes)
    assert len(hd.bestDF) == len(hs.bestDF), m
    for rd, rs in zip(hd.bestDF, hs.bestDF):
        assert rd["timestep"] == rs["timestep"]
        for k in ("action", "p", "y", "reward"):
            assert _raw(rd[k]) == _raw(rs[k]), (m, k)
    for x, y in zip(hd.bestNNA.model.params(), hs.bestNNA.model.params()):
        assert _raw(x) == _raw(y), m
    assert hd.init_rng.bit_generator.state == hs.init_rng.bit_generator.state, m
    if next_draw:                # the next draw of the member's generator (on copies: the cached solo runs stay as they are)
        assert copy.deepcopy(hd.init_rng).random() == copy.deepcopy(hs.init_rng).random(), m


def _kinds(solos):
    """(time-outs, early ends that are not errored, early ends that are errored) over the solo runs"""
    full = sum(len(s.hook.rewards_compare) for s in solos)          # min_best_episode = 1: every episode that reached te
    errored = sum(len(s.hook.errored_episodes) for s in solos)
    early = sum(len(s.hook.rewards) for s in solos) - full
    return full, early - errored, errored


def _four(pkg):
    return lambda k: pkg.StopAfterEpisode(EPISODES)


@pytest.mark.parametrize("nx", [64, 128])
def test_members_equal_solo_runs(pkg, nx):
    setup = _setup(pkg, nx)
    solos = _solos(pkg, nx, "four", _four(pkg))
    kinds = _kinds(solos)
    print("nx", nx, "kinds (time-out, early, early and errored)", kinds,
          [(s.hook.errored_episodes, len(s.hook.rewards_compare)) for s in solos])
    assert min(kinds) >= 1, kinds
    pop = _population(pkg, setup, three_pipes=(nx == 128))
    print(f"part streams of the population's step (nx = {nx}): {pop.env.n_part_streams}")
    pop.run([pkg.StopAfterEpisode(EPISODES) for _ in MEMBERS])
    torch.cuda.synchronize()
    assert pop.timing["blocks"] == EPISODES
    T = pop._logs.T
    assert T == 11
    steps = np.array(pop.episode_steps)
    assert (steps == T).any() and ((steps > 0) & (steps < T)).any(), steps.tolist()
    for m, solo in enumerate(solos):
        _assert_member_equals_solo(pop, m, solo)
    ev = pop.evaluate(n_inits=2)
    assert ev["batched"] is True and ev["episode_reward"].shape == (len(MEMBERS), 2)
    h = pop.hyper()
    assert h["act_limit"].tolist() == [mb[2] for mb in MEMBERS] and h["act_noise"].tolist() == [mb[1] for mb in MEMBERS]
    pop.close()


def test_members_equal_solo_runs_with_the_batch_split_into_parts():
    """the same comparisons on the reference's grid, one episode per read-back and blocks of three, with the step's part-batch
    children forced on (PDEC_FLUID_SPLIT=2: the three members step as 1 + 2 trajectories, the second part on the caller's part
    stream; by default the fluid step splits from the padded 512-point grid and 8 trajectories on).  The blocks run
    pdec_fluid_error_detection on the split parent, which serves the whole batch from its own work arrays.  The switch is read
    once per process, hence the fresh one."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, PDEC_FLUID_SPLIT="2")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-s", "-p", "no:cacheprovider",
                        "-k", "(test_members_equal_solo_runs or test_blocks_of_three) and 128"], env=env, capture_output=True, text=True, timeout=300,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout, r.stdout[-2000:]
    assert "part streams of the population's step (nx = 128): 1" in r.stdout, r.stdout[-2000:]
    assert "part streams of the block population's step (nx = 128): 1" in r.stdout, r.stdout[-2000:]


def _mixed_stops(pkg):
    # the tame member stops at the first episode end behind 25 steps (its third episode), the wild one inside the first block
    return lambda k: [pkg.StopAfterEpisodeWithMinSteps(25), pkg.StopAfterEpisode(EPISODES), pkg.StopAfterEpisode(2)][k]


@pytest.mark.parametrize("nx", [64, 128])
def test_blocks_of_three_episodes_equal_solo_runs(pkg, nx):
    setup = _setup(pkg, nx)
    mk = _mixed_stops(pkg)
    solos = _solos(pkg, nx, "mixed", mk)
    assert [len(s.hook.rewards) for s in solos] == [3, EPISODES, 2]
    print("nx", nx, "mixed stops: errored", [s.hook.errored_episodes for s in solos])
    assert sum(len(s.hook.errored_episodes) for s in solos) >= 1
    pop = _population(pkg, setup, three_pipes=(nx == 128))
    print(f"part streams of the block population's step (nx = {nx}): {pop.env.n_part_streams}")
    stops = [mk(k) for k in range(len(MEMBERS))]
    pop.run(stops, episodes_per_sync=3)
    torch.cuda.synchronize()
    assert pop.timing["blocks"] == 2 and pop.timing["episodes"] == 4
    for m, solo in enumerate(solos):
        _assert_member_equals_solo(pop, m, solo)
    # ... and where the one-episode path ends, stop conditions included
    p1 = _population(pkg, setup)
    stops1 = [mk(k) for k in range(len(MEMBERS))]
    p1.run(stops1)
    torch.cuda.synchronize()
    assert [n.tolist() for n in pop.episode_steps] == [n.tolist() for n in p1.episode_steps]
    assert [s.cur for s in stops] == [s.cur for s in stops1]
    for m in range(len(MEMBERS)):
        assert pop.hooks[m].errored_episodes == p1.hooks[m].errored_episodes
        assert pop.hooks[m].init_rng.bit_generator.state == p1.hooks[m].init_rng.bit_generator.state
    pop.close()
    p1.close()


def _take_over_by_checkpoint(pkg, path, src, dst):
    """what Population.clone promises: load_agent(dst) of save_agent(src), dst keeping its own counters, seeds and rng"""
    p = dst.agent.policy
    keep = (p.update_step, p.act_noise, p.act_limit, p._noise_seed, p._noise_off, p._sample_seed, p._sample_off,
            copy.deepcopy(p.rng.bit_generator.state))
    pkg.checkpoint.save_agent(path, src.agent, with_trajectory=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", pkg.agent.TargetNetworkWarning)
        pkg.checkpoint.load_agent(path, dst.agent)
    p.update_step, p.act_noise, p.act_limit, p._noise_seed, p._noise_off, p._sample_seed, p._sample_off = keep[:7]
    p.rng.bit_generator.state = keep[7]
    torch.cuda.synchronize()


def test_clone_between_two_runs_equals_the_checkpoint_round_trip(pkg, tmp_path):
    setup = _setup(pkg, 64)
    pop = _population(pkg, setup)
    two = lambda: [pkg.StopAfterEpisode(2) for _ in MEMBERS]      # noqa: E731
    pop.run(two())
    torch.cuda.synchronize()
    assert pop.clone({2: 0}, replay="copy") == [(2, 0)]
    pop.run(two())
    torch.cuda.synchronize()
    twins = [_Solo(pkg, setup, k).run(pkg.StopAfterEpisode(2)) for k in range(len(MEMBERS))]
    _take_over_by_checkpoint(pkg, str(tmp_path / "member0.npz"), twins[0], twins[2])
    for m, tw in enumerate(twins):
        tw.run(pkg.StopAfterEpisode(2))
        _assert_member_equals_solo(pop, m, tw)
    pop.close()


def test_refusals_name_the_member_or_the_number(pkg):
    setup = _setup(pkg, 64)
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()

    def members(st, n=2, **kw):
        ags = [pkg.create_agent(setup=st, B=1, rng=np.random.default_rng(i), noise_seed=i, stream=s_upd, trajectory_length=4096, **kw)
               for i in range(n)]
        return ags, [st.make_hook(init_seed=i) if hasattr(st, "make_hook") else pkg.PDEhook(init_seed=i) for i in range(n)]

    big = pkg.FluidSetup.Fluid_32(te=0.2)
    with pytest.raises(pkg.PdecError, match=r"member 0: 1024 actuators.*Fluid_32"):
        pkg.Population(big, *members(big), stream_env=s_env)
    with pytest.raises(pkg.PdecError, match="fp64 environments only"):
        pkg.Population(setup, *members(setup), stream_env=s_env, dtype=torch.float32)
    ags, hks = members(setup)
    with pytest.raises(pkg.PdecError, match=r"max_log_bytes = 1048576; at most \d+ members fit"):
        pkg.Population(setup, ags, hks, stream_env=s_env, max_log_bytes=1 << 20)
    ks = pkg.KSSetup.KS22()
    with pytest.raises(pkg.PdecError, match=r"member 0: .*FluidSetup"):
        pkg.Population(setup, *members(ks), stream_env=s_env)
    with pytest.raises(pkg.PdecError, match="KellerSegel2DSetup"):
        pkg.Population(pkg.KellerSegel2DSetup(), *members(ks), stream_env=s_env)
    # a hook whose error_detection is not this population's setup's own stays with one episode per read-back
    other = pkg.FluidSetup(nx=64, oversampling=8, te=0.2)
    hks[1] = pkg.PDEhook(init_seed=1, error_detection=other.error_detection)
    pop = pkg.Population(setup, ags, hks, stream_env=s_env)
    with pytest.raises(pkg.PdecError, match="member 1: .*error_detection"):
        pop.run([pkg.StopAfterEpisode(1) for _ in ags], episodes_per_sync=2)
    pop.hooks[1] = pkg.PDEhook(init_seed=1, error_detection=lambda y: False)
    with pytest.raises(pkg.PdecError, match="member 1: .*error_detection"):
        pop.run([pkg.StopAfterEpisode(1) for _ in ags], episodes_per_sync=2)
    assert all(h.rewards == [] for h in pop.hooks)      # nothing ran
    pop.close()
