"""Host-side checks of the per-trajectory episode clock (no GPU): its C ABI is declared, exported and bound, TrainPipeline
takes the two new arguments, and the NumPy restatement the GPU tests compare against (tests/episode_clock_ref.py) has the
properties the mode rests on -- the ledger's returns when nothing blows up, evenly spread time-outs under stagger, and one
Philox stream for W ranks of B trajectories and for one rank of W B."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from episode_clock_ref import ClockModel, init_offset, initial_clocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPCLOCK = {"pdec_epclock_create": 8, "pdec_epclock_set": 2, "pdec_epclock_step": 10, "pdec_epclock_read": 6}


def test_epclock_abi_is_declared_exported_and_bound(pkg):
    lib = ctypes.CDLL(pkg._lib.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pdeconv.h")).read(), flags=re.S)
    for name, nargs in EPCLOCK.items():
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(pkg._lib.SIGNATURES[name]), name
    src = open(os.path.join(ROOT, pkg.__name__, "csrc", "Makefile")).read()
    assert "episode_clock.hip" in re.search(r"^SRCS\s*=(.*)$", src, flags=re.M).group(1).split()


def test_pipeline_accepts_the_mode_arguments(pkg):
    sig = inspect.signature(pkg.TrainPipeline.__init__).parameters
    assert sig["episodes"].default == "lockstep" and sig["stagger"].default is False
    # (the defaults tests/test_pipeline_episodes_host.py pins are those of the lock-stepped mode and stay)
    defaults = dict(log_episodes=0, min_best_episode=0, random_init=False, init_seed=0, init_rng=None, init_rank=(0, 1))
    for k, v in defaults.items():
        assert sig[k].default == v, k
    assert callable(pkg.TrainPipeline.finished_episodes)
    assert isinstance(pkg.TrainPipeline.episodes_finished, property)


def _restate(rews, flags, E):
    """the ledger's order of arithmetic (tests/test_gpu_pipeline_episodes.py::_restate, restated): per step (sum over a in
    index order of fp64 values) / R added to the running return; per episode the batch mean summed in b order"""
    rets, blews, means = [], [], []
    for e in range(len(rews) // E):
        ret = np.zeros(rews[0].shape[0])
        blew = np.zeros(rews[0].shape[0], dtype=bool)
        for k in range(e * E, (e + 1) * E):
            r = rews[k].astype(np.float64)
            s = np.zeros(r.shape[0])
            for a in range(r.shape[1]):
                s = s + r[:, a]
            ret = ret + s / r.shape[1]
            blew |= flags[k] != 0
        t = 0.0
        for v in ret:
            t += v
        rets.append(ret)
        blews.append(blew)
        means.append(t / ret.shape[0])
    return np.array(rets), np.array(blews), means


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_model_is_the_ledger_when_nothing_blows_up(dtype):
    B, R, E, n_ep = 5, 8, 7, 3
    rng = np.random.default_rng(3)
    rews = [(-rng.uniform(0, 40, (B, R)) ** 2).astype(dtype) for _ in range(n_ep * E)]
    flags = [np.zeros(B, dtype=np.int32) for _ in rews]
    m = ClockModel(B, E, n_ep)
    for k, (r, f) in enumerate(zip(rews, flags)):
        out, ended, n = m.step(r, f)
        assert np.array_equal(out, r)
        assert ended.all() == ((k + 1) % E == 0) and ended.any() == ended.all()
        assert np.array_equal(n, np.full(B, (k + 1) // E if ended.all() else 0))
    ret, blew, _ = _restate(rews, flags, E)
    fin = m.finished()
    assert fin["dropped"] == 0 and not fin["blew_up"].any() and (fin["length"] == E).all()
    # sorted by (end_step, trajectory): episode e of trajectory b is entry e B + b
    assert np.array_equal(fin["trajectory"], np.tile(np.arange(B), n_ep))
    assert np.array_equal(fin["episode"], np.repeat(np.arange(n_ep), B))
    assert np.array_equal(fin["end_step"], np.repeat(E * np.arange(1, n_ep + 1), B))
    assert np.array_equal(fin["ret"].reshape(n_ep, B), ret)


def test_model_blow_up_rules():
    B, R, E = 4, 3, 3
    m = ClockModel(B, E, 2)
    r = np.ones((B, R), dtype=np.float32)
    r[1, 0], r[2, 1] = np.inf, np.nan            # row 1 blows up (sanitised), row 2 does not (left alone)
    out, ended, n = m.step(r, np.array([0, 1, 0, 0], dtype=np.int32))
    assert np.array_equal(ended, [False, True, False, False]) and np.array_equal(n, [0, 1, 0, 0])
    assert out[1, 0] == 0 and np.isnan(out[2, 1]) and np.array_equal(out[[0, 3]], r[[0, 3]])
    assert m.slots[1][0][:4] == (2.0 / 3.0, 1, True, 1)
    assert np.isnan(m.ret[2]) and m.ret[1] == 0 and m.ret[0] == 1.0
    assert np.array_equal(m.clock, [1, 0, 1, 1])
    m.step(np.ones((B, R), dtype=np.float32), np.zeros(B, dtype=np.int32))
    # a blow-up on the very step the clock times out: one episode, marked blown up
    out, ended, n = m.step(np.ones((B, R), dtype=np.float32), np.array([1, 0, 0, 0], dtype=np.int32))
    assert np.array_equal(ended, [True, False, True, True]) and m.slots[0][0][:4] == (3.0, 3, True, 3)
    assert m.slots[3][0][:4] == (3.0, 3, False, 3) and np.isnan(m.slots[2][0][0])
    assert np.array_equal(m.count, [1, 1, 1, 1]) and np.array_equal(m.clock, [0, 2, 0, 0])
    # the ring wraps: trajectory 1 ends twice more, capacity 2
    for _ in range(4):
        m.step(np.ones((B, R), dtype=np.float32), np.zeros(B, dtype=np.int32))
    assert m.count[1] == 3 and sorted(v[4] for v in m.slots[1].values()) == [1, 2]
    fin = m.finished()
    assert fin["dropped"] == 1 and np.array_equal(fin["end_step"], np.sort(fin["end_step"]))
    # pdec_epclock_set: the running episodes are cut without an entry, counts and logs stay
    before = (m.count.copy(), [dict(s) for s in m.slots])
    m.set()
    assert np.array_equal(m.count, before[0]) and m.slots == before[1] and not m.ret.any() and not m.len.any()


@pytest.mark.parametrize("B,E", [(8, 7), (64, 17), (5, 12), (512, 51), (7, 7), (3, 1)])
def test_staggered_clocks_spread_the_time_outs(B, E):
    c0 = initial_clocks(B, E, True)
    assert c0[0] == 0 and (c0 >= 0).all() and (c0 < E).all() and np.array_equal(c0, (np.arange(B) * E) // B)
    assert not initial_clocks(B, E, False).any()
    m = ClockModel(B, E, 4, c0)
    zero, flags = np.zeros((B, 2), dtype=np.float32), np.zeros(B, dtype=np.int32)
    per_phase = np.zeros((3, E), dtype=np.int64)
    first_len = np.zeros(B, dtype=np.int64)
    for k in range(3 * E):
        _, ended, n = m.step(zero, flags)
        per_phase[k // E, k % E] = ended.sum()
        first_len[ended & (n == 1)] = k + 1
    # every phase 0 .. E-1 receives floor(B / E) or ceil(B / E) time-outs in every window of E steps
    assert per_phase.sum(axis=1).tolist() == [B] * 3
    assert per_phase.min() >= B // E and per_phase.max() <= -(-B // E)
    assert np.array_equal(per_phase[0], per_phase[1]) and np.array_equal(per_phase[1], per_phase[2])
    # the first episode of trajectory b is shorter by its initial clock and is logged with the steps it really took
    assert np.array_equal(first_len, E - c0)
    fin = m.finished()
    first = fin["episode"] == 0
    assert np.array_equal(fin["length"][first][np.argsort(fin["trajectory"][first])], E - c0)
    assert (fin["length"][~first] == E).all()


@pytest.mark.parametrize("W,B,nc", [(2, 16, 8), (3, 8, 8), (4, 5, 7), (3, 4, 13)])
def test_rank_offsets_are_one_stream(W, B, nc):
    nblk = (nc + 3) // 4
    for n in range(4):
        split = [init_offset(n, r, W, B, nc) + b * nblk for r in range(W) for b in range(B)]
        whole = [init_offset(n, 0, 1, W * B, nc) + g * nblk for g in range(W * B)]
        assert split == whole
        # ... and consecutive episodes do not overlap: a draw takes W B nblk counters
        assert init_offset(n + 1, 0, W, B, nc) - init_offset(n, 0, W, B, nc) == W * B * nblk
    # the lock-stepped pipeline's Inits.draw: off = (e W + r) n with n = B ceil(nc / 4)
    assert init_offset(5, 1, 3, 8, 8) == (5 * 3 + 1) * (8 * 2)
