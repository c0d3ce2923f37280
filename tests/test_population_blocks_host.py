"""Host rules of Population.run(stops, episodes_per_sync > 1), no GPU: the NumPy restatement of the device's episode close
(tests/population_block_ref.py) against the real PDEhook, stop conditions and Agent; the block-length function against stepping
the stop classes; the book's slot names against the header."""
import importlib
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import population_block_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, COLS, STRIDE, INC = 5, 3, 3, 2


def _mods(pkg):
    return [importlib.import_module(pkg.__name__ + "." + n) for n in ("run", "agent", "population")]


class _Traj:
    """the counters of CircularArraySARTTrajectory that the boundary moves"""
    stride = STRIDE

    def __init__(self):
        self.n_sa = self.n_rt = 0

    def __len__(self):
        return self.n_rt

    def pop_sa(self, n):
        self.n_sa -= n


class _Member:
    """one member on the host, moved by the real classes exactly as Population._episode / run._run_device_episodes move it"""

    def __init__(self, pkg, stop, reset_post=True, **hook_kw):
        self.run, self.ag, _ = _mods(pkg)
        self.hook = pkg.PDEhook(collect_bestDF=False, **hook_kw)
        self.stop = stop
        pol = SimpleNamespace(reset_stage=self.ag.POST_EPISODE_STAGE if reset_post else self.ag.POST_EXPERIMENT_STAGE, update_step=0)
        self.agent = self.ag.Agent(pol, _Traj())
        self.env = SimpleNamespace(dt=0.1, te=0.45, y=None, is_fluid=False)
        assert self.run._episode_steps(self.env) == T
        self.active = True

    def episode(self, flags_m, means_m):
        """returns (reward, n, new_best, which); the member's objects are behind the boundary afterwards"""
        pol, tr, hk = self.agent.policy, self.agent.trajectory, self.hook
        self.agent._stage(self.ag.PRE_EPISODE_STAGE, self.env, ())
        if hk.use_random_init:
            hk._init_off += INC
        n = self.run._executed_steps(flags_m, T)
        pol.update_step += n
        tr.n_sa += n * COLS
        tr.n_rt += n * COLS
        self.run._add_episode_reward(hk, means_m[:n], np.float64)
        reward = hk.reward
        fired = self.run._stop_fired(self.stop, self.agent, n)
        self.agent.end_episode(np.zeros((COLS, 1)), pushed=True)
        self.env.time = self.run._episode_time(self.env.dt, n)
        new_best = hk.end_episode(self.env)
        if fired:
            self.active = False
        return reward, n, int(new_best), (1 if new_best else 0) | (2 if hk.collect_NNA else 0)


def _tables(pkg, members):
    """rows and book as Population._block uploads them (after the host's PRE_EPISODE of the block's first episode)"""
    _, ag_mod, pop = _mods(pkg)
    M = len(members)
    rows, book = np.zeros((M, 16), dtype=np.int64), np.zeros((M, 16), dtype=np.int64)
    for m, mb in enumerate(members):
        hk, st, tr = mb.hook, mb.stop, mb.agent.trajectory
        if mb.active:
            mb.agent._stage(ag_mod.PRE_EPISODE_STAGE, mb.env, ())
        rows[m, [ref.USTEP, ref.NSA, ref.NRT]] = (mb.agent.policy.update_step, tr.n_sa, tr.n_rt)
        rows[m, ref.HALT], rows[m, ref.ACTIVE] = (0, 1) if mb.active else (1, 0)
        has, cmp = pop.python_max_state(hk.rewards_compare)
        kind, lim = (0, st.episode) if type(st) is pkg.StopAfterEpisode else (1, st.step)
        book[m, :ref.FIRED] = (hk.ep, hk.min_best_episode, int(hk.collect_NNA), has, ref.bits(cmp), ref.bits(hk.bestreward), hk.bestepisode,
                               kind, st.cur, lim, int(hk.use_random_init), hk.init_seed, hk._init_off, INC)
    return rows, book


def _same_double(a, b):
    return ref.bits(a) == ref.bits(b) or (np.isnan(a) and np.isnan(b))


def _run_block(pkg, members, flags_seq, means_seq, reset_post=True):
    """a block of len(flags_seq) episodes through the restatement, and the same episodes through the real classes"""
    _, _, pop = _mods(pkg)
    rows, book = _tables(pkg, members)
    M, L = len(members), len(flags_seq)
    dummy = np.zeros((T + 1, M, 1)), np.zeros((T + 1, M, 1)), np.zeros((M, 1)), np.zeros((M, 1))
    for e in range(L):
        was = [mb.active for mb in members]
        for m in np.flatnonzero(was):      # the kernels of the episode's steps count them into the rows
            n = ref.executed_steps(flags_seq[e][:, m], T)
            rows[m, [ref.USTEP, ref.NSA, ref.NRT]] += (n, n * COLS, n * COLS)
        elog, which = ref.close_phase0(rows, book, flags_seq[e], means_seq[e], *dummy)
        ref.close_phase1(rows, book, COLS, STRIDE, int(reset_post), int(e == L - 1))
        for m, mb in enumerate(members):
            if not was[m]:
                assert elog[m].tolist() == [0, 0, 0, 0] and which[m] == 0
                continue
            n = int(elog[m, ref.STEPS])
            reward, n_h, nb, wh = mb.episode(flags_seq[e][:, m], means_seq[e][m])
            assert (n, int(elog[m, ref.NEW_BEST]), int(which[m]), int(elog[m, ref.RAN])) == (n_h, nb, wh, 1), (e, m)
            assert _same_double(ref.dbl(elog[m, ref.REWARD]), reward), (e, m)
            hk, tr = mb.hook, mb.agent.trajectory
            assert bool(rows[m, ref.ACTIVE]) == mb.active and bool(rows[m, ref.HALT]) == (not mb.active), (e, m)
            assert int(book[m, ref.EP]) == hk.ep and int(book[m, ref.STOP_CUR]) == mb.stop.cur, (e, m)
            assert int(book[m, ref.BESTEPISODE]) == hk.bestepisode and _same_double(ref.dbl(book[m, ref.BESTREWARD]), hk.bestreward)
            has, cmp = pop.python_max_state(hk.rewards_compare)
            assert int(book[m, ref.CMP_HAS]) == has and (not has or _same_double(ref.dbl(book[m, ref.CMP]), cmp)), (e, m)
            if has:     # the carried state IS Python's max()
                assert _same_double(cmp, max(hk.rewards_compare))
            assert int(book[m, ref.INIT_OFF]) == hk._init_off, (e, m)
            # the host's PRE_EPISODE of a member that goes on comes with its next episode (or the next block's upload)
            n_sa = tr.n_sa - (STRIDE if mb.active and e + 1 < L and tr.n_sa > tr.n_rt else 0)
            assert (int(rows[m, ref.USTEP]), int(rows[m, ref.NSA]), int(rows[m, ref.NRT])) == (mb.agent.policy.update_step, n_sa, tr.n_rt)
    return rows, book


def _episodes(rng, M, L, p_flag=0.3, special=None):
    """L episodes of flags [T, M] and means [M, T]; special[(e, m)] = ("nan" | "tie", ...) shapes single episodes"""
    flags_seq, means_seq = [], []
    for e in range(L):
        fl = np.zeros((T, M), dtype=np.int32)
        for m in range(M):
            if rng.random() < p_flag:
                fl[rng.integers(0, T), m] = 1            # (a flag at T - 1 is the time-out: the episode counts as whole)
                if rng.random() < 0.3:
                    fl[rng.integers(0, T), m] = 1
        mu = rng.standard_normal((M, T))
        for (ee, m), what in (special or {}).items():
            if ee == e:
                fl[:, m] = 0
                if what == "nan":
                    mu[m, rng.integers(0, T)] = np.nan
                elif what == "tie":
                    means_seq[e - 1][m] += 5.0           # (the earlier of the two is a best when it comes)
                    mu[m] = means_seq[e - 1][m]
                    flags_seq[e - 1][:, m] = 0
        flags_seq.append(fl)
        means_seq.append(mu)
    return flags_seq, means_seq


@pytest.mark.parametrize("seed", range(6))
def test_close_rule_equals_the_real_classes_on_random_sequences(pkg, seed):
    rng = np.random.default_rng(seed)
    stops = [pkg.StopAfterEpisode(4), pkg.StopAfterEpisodeWithMinSteps(17), pkg.StopAfterEpisode(12), pkg.StopAfterEpisodeWithMinSteps(40),
             pkg.StopAfterEpisode(2)]
    kw = [dict(min_best_episode=0), dict(min_best_episode=3, use_random_init=True, init_seed=5), dict(collect_NNA=False),
          dict(min_best_episode=1, use_random_init=True), dict(min_best_episode=2)]
    members = [_Member(pkg, s, reset_post=bool(seed % 2 == 0), **k) for s, k in zip(stops, kw)]
    # two blocks of the same members: the second starts from what the first left in the real objects
    for L in (4, 5):
        fs, ms = _episodes(rng, len(members), L)
        _run_block(pkg, members, fs, ms, reset_post=bool(seed % 2 == 0))
    assert not members[0].active and not members[4].active      # members stopped mid-sequence and stayed idle
    assert any(mb.active for mb in members)


def test_nan_rewards_ties_and_min_best_episode(pkg):
    rng = np.random.default_rng(11)
    members = [_Member(pkg, pkg.StopAfterEpisode(6), min_best_episode=0),     # NaN is its first eligible episode
               _Member(pkg, pkg.StopAfterEpisode(6), min_best_episode=0),     # NaN comes later
               _Member(pkg, pkg.StopAfterEpisode(6), min_best_episode=0),     # a tie: >= keeps the later episode
               _Member(pkg, pkg.StopAfterEpisode(6), min_best_episode=4)]     # its first three episodes are not eligible
    special = {(0, 0): "nan", (1, 0): "whole", (2, 1): "nan", (0, 1): "whole", (3, 1): "whole", (2, 2): "tie", (4, 3): "whole"}
    fs, ms = _episodes(rng, 4, 6, p_flag=0.2, special=special)
    _run_block(pkg, members, fs, ms)
    h0, h1, h2, h3 = (mb.hook for mb in members)
    assert np.isnan(h0.rewards_compare[0]) and h0.bestepisode == 0 and h0.bestreward == -1000000.0     # nothing is >= NaN
    assert any(np.isnan(v) for v in h1.rewards_compare[1:]) and h1.bestepisode >= 1 and not np.isnan(h1.bestreward)
    assert h2.rewards[1] == h2.rewards[2] and h2.bestepisode == 3      # (episodes count from 1: the tie is episodes 2 and 3)
    assert h3.bestepisode >= 4 and len(h3.rewards_compare) <= 3


def test_python_max_state_is_pythons_max(pkg):
    _, _, pop = _mods(pkg)
    nan = float("nan")
    for vals in ([], [1.0], [nan], [nan, 2.0], [2.0, nan], [1.0, 3.0, 3.0, 2.0], [-0.0, 0.0], [0.0, -0.0], [2.0, nan, 5.0]):
        has, cmp = pop.python_max_state(vals)
        assert has == int(bool(vals))
        if vals:
            assert _same_double(cmp, max(vals)), vals


@pytest.mark.parametrize("kind", ["episode", "min_steps"])
def test_block_length_against_stepping_the_stop_classes(pkg, kind):
    run, _, pop = _mods(pkg)
    rng = np.random.default_rng(3)
    for trial in range(200):
        Tt = int(rng.integers(1, 9))
        if kind == "episode":
            stop = pkg.StopAfterEpisode(int(rng.integers(0, 7)))
            stop.cur = int(rng.integers(0, 8))
        else:
            stop = pkg.StopAfterEpisodeWithMinSteps(int(rng.integers(0, 40)))
            stop.cur = int(rng.integers(1, 45))
        need = pop.episodes_still_needed(stop, Tt)
        # the least number of episodes: every episode as long as it can be
        twin = type(stop)(stop.episode if kind == "episode" else stop.step)
        twin.cur = stop.cur
        k = 0
        while True:
            k += 1
            if run._stop_fired(twin, None, Tt):
                break
        assert need == k, (kind, trial)
        # shorter episodes never need fewer
        twin = type(stop)(stop.episode if kind == "episode" else stop.step)
        twin.cur = stop.cur
        k2 = 0
        while True:
            k2 += 1
            if run._stop_fired(twin, None, int(rng.integers(1, Tt + 1))):
                break
        assert k2 >= need
    a, b, c = pkg.StopAfterEpisode(2), pkg.StopAfterEpisode(7), pkg.StopAfterEpisode(30)
    assert pop.block_length([a, b, c], [True, True, False], 5, 4) == 4
    assert pop.block_length([a, b, c], [True, False, False], 5, 4) == 2
    assert pop.block_length([a, b, c], [True, True, True], 5, 64) == 30


def test_book_slot_tables_equal_the_device_enums(pkg):
    """population.py's BOOK / BK_* and ELOG / EL_* are POP_BOOK / enum PopBookSlot and POP_ELOG / enum PopElogSlot of
    csrc/population.hpp, in order; so are the restatement's; row slot 15 stays free"""
    _, _, pop = _mods(pkg)
    hpp = open(os.path.join(ROOT, "distributedconvrl-pde-control_amd", "csrc", "population.hpp")).read()
    for enum, define, prefix, mine, size in (("PopBookSlot", "POP_BOOK", "PBK_", "BK_", pop.BOOK), ("PopElogSlot", "POP_ELOG", "PEL_", "EL_", pop.ELOG)):
        assert size == int(re.search(r"#define %s (\d+)" % define, hpp).group(1))
        body = re.sub(r"//.*", "", re.search(r"enum %s \{(.*?)\};" % enum, hpp, re.S).group(1))
        names = [n.strip() for n in body.split(",") if n.strip()]
        assert names[0].replace(" ", "").endswith("=0") and not any("=" in n for n in names[1:])
        names[0] = names[0].split("=")[0].strip()
        assert len(names) == size
        assert [getattr(pop, mine + n[len(prefix):]) for n in names] == list(range(size))
        assert [getattr(ref, n[len(prefix):]) for n in names] == list(range(size))
    assert pop.ROW == 16 and max(pop.LIMIT, pop.ETA_C) == 14
