"""Population.run(stops, episodes_per_sync = E > 1): blocks of whole episodes per read-back, the episode boundary decided on
the device (csrc/pop_book.hip).  Every member must end bit for bit where episodes_per_sync = 1 leaves it."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import population_block_ref as ref
from test_gpu_population import _assert_member_equals_solo, _make, _solo

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _population(pkg, setup, seeds, stop_lists, decay, E, random_init=None):
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    members = [_make(pkg, setup, s, s_upd, True if random_init is None else random_init[i]) for i, s in enumerate(seeds)]
    pop = pkg.Population(setup, [a for a, _ in members], [h for _, h in members], stream_env=s_env, dtype=torch.float64)
    for k in range(len(stop_lists[0])):
        pop.run([sl[k] for sl in stop_lists], episodes_per_sync=E)
        for a in pop.agents:
            a.policy.act_noise *= decay
    torch.cuda.synchronize()
    return pop


def _bits(values):
    return np.asarray(values, dtype=np.float64).view(np.int64).tolist()


def _assert_populations_equal(pe, p1, stops_e, stops_1):
    """everything _assert_member_equals_solo compares, member by member, and what only a population's hooks and stops hold"""
    assert [n.tolist() for n in pe.episode_steps] == [n.tolist() for n in p1.episode_steps]
    for m in range(pe.M):
        one = SimpleNamespace(y=p1.env.y[m:m + 1], state=p1.env.state[m:m + 1])
        _assert_member_equals_solo(pe, m, (one, p1.agents[m], p1.hooks[m]))
        he, h1 = pe.hooks[m], p1.hooks[m]
        assert (he.ep, he.bestepisode, he._init_off, he.reward) == (h1.ep, h1.bestepisode, h1._init_off, h1.reward), m
        assert _bits([he.bestreward]) == _bits([h1.bestreward]) and _bits(he.rewards_compare) == _bits(h1.rewards_compare), m
        assert he.currentDF == [] and h1.currentDF == []
        for x, y in zip(he.currentNNA.model.params(), h1.currentNNA.model.params()):
            assert np.array_equal(x, y), m
        for se, s1 in zip(stops_e[m], stops_1[m]):
            assert se.cur == s1.cur, m


def test_close_launch_on_synthetic_tables(pkg):
    """pdec_population_episode_close, both phases, three consecutive episodes of M = 3, T = 4 against the NumPy restatement,
    bit for bit: book, rows, which, episode log, gathered y / state.  Flags: none, step 0, step T - 1 (the time-out), mid-episode;
    member 2 is idle and the bytes of its rows of env.y / env.state stay; member 1 stops inside the sequence."""
    setup = pkg.KSSetup.KS22()
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    members = [_make(pkg, setup, s, s_upd) for s in (1, 2, 3)]
    pop = pkg.Population(setup, [a for a, _ in members], [h for _, h in members], stream_env=s_env, dtype=torch.float64)
    M, T, ysz, ssz = 3, 4, 7, 5
    cols, stride = pop.cols, pop.agents[0].trajectory.stride
    rng = np.random.default_rng(0)
    rows = np.zeros((M, 16), dtype=np.int64)
    rows[:, [ref.USTEP, ref.NSA, ref.NRT, ref.NOISE, ref.SAMPLE]] = [[7, 40, 40, 3, 1], [9, 56, 48, 5, 2], [4, 16, 16, 0, 0]]
    rows[:, ref.ACTIVE], rows[:, ref.HALT] = [1, 1, 0], [0, 0, 1]
    rows[:, 7:16] = rng.integers(0, 2 ** 40, size=(M, 9))            # (slots the close must not touch)
    book = np.zeros((M, 16), dtype=np.int64)
    #              ep min nna has cmp            bestreward        bestep kind cur lim rnd seed off inc
    book[0, :14] = (1, 0, 1, 0, 0, ref.bits(-1000000.0), 0, 1, 1, 100, 1, 11, 6, 2)
    book[1, :14] = (3, 2, 1, 1, ref.bits(-0.5), ref.bits(-0.5), 2, 0, 0, 2, 0, 12, 0, 2)
    book[2, :14] = (5, 0, 0, 1, ref.bits(2.0), ref.bits(-1000000.0), 0, 0, 9, 3, 1, 13, 4, 2)
    flags = np.zeros((3, T, M), dtype=np.int32)
    flags[0, T - 1, 1] = 1            # member 1, episode 0: the time-out flag only
    flags[1, 0, 0] = 1                # member 0, episode 1: ends at its first step
    flags[1, 2, 0] = 1
    flags[2, 1, 0] = 1                # member 0, episode 2: ends mid-episode
    flags[2, T - 1, 0] = 1
    flags[:, 1, 2] = 1                # (the idle member's flags are not read)
    means = rng.standard_normal((3, M, T))
    means[0, 1] = np.abs(means[0, 1])
    means[1, 1] = means[0, 1]         # member 1: a tie above the earlier maximum, the later episode takes the best
    log_y, log_s = rng.standard_normal((3, T + 1, M, ysz)), rng.standard_normal((3, T + 1, M, ssz))
    env_y, env_s = rng.standard_normal((M, ysz)), rng.standard_normal((M, ssz))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    P = lambda t: C.c_void_p(t.data_ptr())                                # noqa: E731
    d_book, d_y, d_s = dev(book), dev(env_y), dev(env_s)
    d_elog = torch.full((M, 4), -1, dtype=torch.int64, device="cuda:0")
    d_which = torch.full((M,), -1, dtype=torch.int32, device="cuda:0")
    pop.rows.copy_(dev(rows))
    idle_y = env_y[2].copy()
    for e in range(3):
        d_flags, d_means, d_ly, d_ls = dev(flags[e]), dev(means[e]), dev(log_y[e]), dev(log_s[e])
        torch.cuda.synchronize()
        for phase in (0, 1):
            assert pop.lib.pdec_population_episode_close(pop._h, phase, P(d_book), P(d_elog), P(d_flags), P(d_means), T, P(d_ly), P(d_ls),
                                                         P(d_y), P(d_s), ysz, ssz, P(d_which), 1, int(e == 2)) == 0
        torch.cuda.synchronize()
        elog, which = ref.close_phase0(rows, book, flags[e], means[e], log_y[e], log_s[e], env_y, env_s)
        ref.close_phase1(rows, book, cols, stride, 1, int(e == 2))
        assert np.array_equal(d_elog.cpu().numpy(), elog), e
        assert np.array_equal(d_which.cpu().numpy(), which), e
        assert np.array_equal(d_book.cpu().numpy(), book), e
        assert np.array_equal(pop.rows.cpu().numpy(), rows), e
        assert np.array_equal(d_y.cpu().numpy().view(np.int64), env_y.view(np.int64)), e
        assert np.array_equal(d_s.cpu().numpy().view(np.int64), env_s.view(np.int64)), e
        assert d_y[2].cpu().numpy().tobytes() == idle_y.tobytes(), e
    # the restatement itself went where the cases say: executed steps, the tie, member 1 stopped inside the sequence
    assert rows[:, ref.ACTIVE].tolist() == [1, 0, 0] and int(book[1, ref.BESTEPISODE]) == 4 and int(book[1, ref.EP]) == 5
    assert int(book[0, ref.STOP_CUR]) == 1 + T + 1 + 2 and int(book[0, ref.INIT_OFF]) == 6 + 3 * 2 and int(book[2, ref.INIT_OFF]) == 4
    pop.close()


def _both(pkg, setup, seeds, make_stops, decay, E, random_init=None):
    stops_e, stops_1 = [make_stops(m) for m in range(len(seeds))], [make_stops(m) for m in range(len(seeds))]
    pe = _population(pkg, setup, seeds, stops_e, decay, E, random_init)
    p1 = _population(pkg, setup, seeds, stops_1, decay, 1, random_init)
    _assert_populations_equal(pe, p1, stops_e, stops_1)
    return pe, p1


def test_block_equals_the_one_episode_path(pkg):
    """members drop out inside the first block (episode counts 2, 5, 3 at E = 4) and the second block is shorter than E"""
    setup, seeds, eps = pkg.KSSetup.KS22(), [3, 11, 29], [2, 5, 3]
    pe, p1 = _both(pkg, setup, seeds, lambda m: [pkg.StopAfterEpisode(eps[m])], 1.0, 4)
    assert [len(h.rewards) for h in pe.hooks] == eps
    assert pe.timing["blocks"] == 2 and pe.timing["episodes"] == 5 and p1.timing["blocks"] == 5
    _assert_member_equals_solo(pe, 1, _solo(pkg, setup, seeds[1], [pkg.StopAfterEpisode(eps[1])], 1.0))


def test_early_ending_episodes_inside_a_block(pkg):
    setup, seeds = pkg.KSSetup.KS22(max_value=4.0), [3, 11, 29]
    pe, _ = _both(pkg, setup, seeds, lambda m: [pkg.StopAfterEpisodeWithMinSteps(200)], 1.0, 3)
    T = pe._logs.T
    assert pe.timing["blocks"] < pe.timing["episodes"]
    mixed = [n for n in pe.episode_steps if ((n > 0) & (n < T)).any() and (n == T).any()]
    assert mixed, [n.tolist() for n in pe.episode_steps]
    assert any(len(h.bestDF) for h in pe.hooks)


def test_keller_segel_with_and_without_random_inits(pkg):
    """the temporal-stack featurize of the episode opening under the device mask"""
    pe, _ = _both(pkg, pkg.KellerSegelSetup(), [2, 8, 13], lambda m: [pkg.StopAfterEpisode(2)], 1.0, 2, [True, False, True])
    assert pe.timing["blocks"] == 1


def test_act_noise_decay_between_two_block_runs(pkg):
    _both(pkg, pkg.KSSetup.KS22(), [5, 6], lambda m: [pkg.StopAfterEpisode(3), pkg.StopAfterEpisode(3)], 0.2, 3)


def test_refusals_name_their_member(pkg):
    setup = pkg.KSSetup.KS22()
    s_env, s_upd = torch.cuda.Stream(), torch.cuda.Stream()
    ags = [pkg.create_agent(setup=setup, B=1, rng=np.random.default_rng(i), noise_seed=i, stream=s_upd) for i in range(3)]
    stops = lambda: [pkg.StopAfterEpisode(1) for _ in range(3)]      # noqa: E731
    hks = [pkg.PDEhook(init_seed=0), pkg.PDEhook(init_seed=1, collect_history=True), pkg.PDEhook(init_seed=2)]
    pop = pkg.Population(setup, ags, hks, stream_env=s_env)
    with pytest.raises(pkg.PdecError, match="member 1: collect_history"):
        pop.run(stops(), episodes_per_sync=2)
    hks[1].collect_history = False
    hks[2] = pop.hooks[2] = pkg.PDEhook(init_seed=2, error_detection=lambda y: False)
    with pytest.raises(pkg.PdecError, match="member 2: .*error_detection"):
        pop.run(stops(), episodes_per_sync=2)
    for bad in (0, -3, 1.5):
        with pytest.raises(pkg.PdecError, match="episodes_per_sync.*members 0..2"):
            pop.run(stops(), episodes_per_sync=bad)
    assert all(h.rewards == [] for h in pop.hooks)      # nothing ran
    pop.close()
