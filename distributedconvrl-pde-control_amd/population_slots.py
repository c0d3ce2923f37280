"""The tables a Population shares with the device, and the two functions that write them.

A member's row of the int64 counter table (include/pdeconv.h, pdec_population_create) holds its ring positions, Philox offsets,
update_step, halt flag and -- as bit patterns of doubles -- its own hyper-parameters; the agents' own attributes are the truth and
are read into the rows whenever an episode (or a block of episodes) begins.  A member's book holds what its hook and its stop
condition carry between two episodes, so that the episode boundary can be decided on the device (population_blocks.py)."""
import numpy as np

from .run import StopAfterEpisode

# a member's row of the device counter table: POP_ROW and enum PopSlot of csrc/population.hpp (tests/test_host_logic.py compares them)
ROW = 16
USTEP, NSA, NRT, NOISE, SAMPLE, HALT, ACTIVE, BPA, BPC, NOISE_AMP, LIMIT = range(11)
# a member's own gamma, rho and ADAM step sizes (bit patterns of doubles): enum PopHyperSlot of csrc/population.hpp; slot 15 is free
GAMMA, RHO, ETA_A, ETA_C = range(11, 15)
# a member's book -- what its hook and its stop condition hold between two episodes -- and the episode log of a block:
# POP_BOOK / enum PopBookSlot and POP_ELOG / enum PopElogSlot of csrc/population.hpp (tests/test_population_blocks_host.py compares them)
BOOK = 16
(BK_EP, BK_MIN_BEST, BK_COLLECT_NNA, BK_CMP_HAS, BK_CMP, BK_BESTREWARD, BK_BESTEPISODE, BK_STOP_KIND, BK_STOP_CUR, BK_STOP_LIMIT,
 BK_RANDOM_INIT, BK_INIT_SEED, BK_INIT_OFF, BK_INIT_INC, BK_FIRED, BK_SPARE) = range(BOOK)
ELOG = 4
EL_REWARD, EL_STEPS, EL_NEW_BEST, EL_RAN = range(ELOG)
HYPER_KEYS = ("gamma", "rho", "actor_lr", "critic_lr", "act_noise", "act_limit")


def _bits(values):
    """the bit patterns of doubles, as the int64 slots carry them"""
    return np.array(values, dtype=np.float64).view(np.int64)


def python_max_state(values):
    """(has, cmp) of Python's max(values) carried element by element: the first element unless a later one compares greater
    (a NaN that comes first stays; a later NaN never replaces)"""
    has, cmp = 0, 0.0
    for v in values:
        if not has:
            has, cmp = 1, v
        elif v > cmp:
            cmp = v
    return has, float(cmp)


def counter_rows(agents, active, hyper):
    """[M, ROW] of an episode's start: every member's counters from its agent, HALT / ACTIVE from `active`, and its own
    hyper-parameters from `hyper` [M, 6] (Population._hyper_rows, HYPER_KEYS' order); BPA / BPC are the library's to fill
    (pdec_population_bp_sel)"""
    rows = np.zeros((len(agents), ROW), dtype=np.int64)
    rows[:, GAMMA:ETA_C + 1] = hyper[:, :4].copy().view(np.int64)
    for m, ag in enumerate(agents):
        pol, tr = ag.policy, ag.trajectory
        rows[m, [USTEP, NSA, NRT, NOISE, SAMPLE]] = (pol.update_step, tr.n_sa, tr.n_rt, pol._noise_off, pol._sample_off)
        rows[m, HALT], rows[m, ACTIVE] = (0, 1) if active[m] else (1, 0)
        rows[m, NOISE_AMP:LIMIT + 1] = _bits([float(pol.act_noise), float(pol.act_limit)])
    return rows


def book_rows(hooks, stops, init_inc):
    """[M, BOOK] of a block's start from the members' hooks and stop conditions.  init_inc: the Philox blocks one random field
    consumes; None for the fluid, whose fields come from host-drawn vortex tables (INIT_OFF / INIT_INC carry 0)"""
    book = np.zeros((len(hooks), BOOK), dtype=np.int64)
    for m, (hk, st) in enumerate(zip(hooks, stops)):
        has, cmp = python_max_state(hk.rewards_compare)
        kind, lim = (0, st.episode) if type(st) is StopAfterEpisode else (1, st.step)
        cmp_bits, best_bits = _bits([cmp, hk.bestreward]).tolist()
        book[m, :BK_FIRED] = (hk.ep, hk.min_best_episode, int(bool(hk.collect_NNA)), has, cmp_bits, best_bits, hk.bestepisode, kind,
                              st.cur, lim, int(bool(hk.use_random_init)), hk.init_seed, 0 if init_inc is None else hk._init_off,
                              init_inc or 0)
    return book
