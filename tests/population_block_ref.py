"""NumPy restatement of a population's episode boundary on the device (csrc/pop_book.hip: pdec_population_episode_close), one
statement per rule.  tests/test_population_blocks_host.py checks it against the real PDEhook, stop conditions and Agent;
tests/test_gpu_population_blocks.py checks the launch against it, bit for bit."""
import numpy as np

# slots of a member's counter row, its book and the episode log (csrc/population.hpp: PopSlot, PopBookSlot, PopElogSlot)
USTEP, NSA, NRT, NOISE, SAMPLE, HALT, ACTIVE = range(7)
(EP, MIN_BEST, COLLECT_NNA, CMP_HAS, CMP, BESTREWARD, BESTEPISODE, STOP_KIND, STOP_CUR, STOP_LIMIT, RANDOM_INIT, INIT_SEED,
 INIT_OFF, INIT_INC, FIRED, SPARE) = range(16)
REWARD, STEPS, NEW_BEST, RAN = range(4)


def bits(v):
    return int(np.array([v], dtype=np.float64).view(np.int64)[0])


def dbl(b):
    return np.array([b], dtype=np.int64).view(np.float64)[0]


def executed_steps(flags_m, T):
    for t in range(T - 1):
        if flags_m[t] != 0:
            return t + 1
    return T


def close_phase0(rows, book, flags, means, log_y, log_state, env_y, env_state):
    """rows [M, 16], book [M, 16] int64 (book changes in place), flags [T, M], means [M, T]; log_y / log_state [T + 1, M, ...],
    env_y / env_state [M, ...] (change in place).  Returns elog [M, 4] int64 and which [M] int32."""
    T, M = flags.shape
    elog, which = np.zeros((M, 4), dtype=np.int64), np.zeros(M, dtype=np.int32)
    for m in range(M):
        bk = book[m]
        if not rows[m, ACTIVE]:
            bk[FIRED] = 0
            continue
        n = executed_steps(flags[:, m], T)
        acc = np.float64(means[m, 0])
        for i in range(1, n):
            acc = np.float64(acc + means[m, i])
        with np.errstate(invalid="ignore"):
            v = np.float64(0.0) + acc
            ep, new_best = int(bk[EP]), 0
            if n == T and ep >= bk[MIN_BEST]:
                cmp = dbl(bk[CMP])
                if not bk[CMP_HAS]:
                    cmp = v
                elif v > cmp:
                    cmp = v
                bk[CMP_HAS], bk[CMP] = 1, bits(cmp)
                if bk[COLLECT_NNA] and v >= cmp:
                    new_best = 1
                    bk[BESTREWARD], bk[BESTEPISODE] = bits(v), ep
        bk[EP] = ep + 1
        which[m] = new_best | (2 if bk[COLLECT_NNA] else 0)
        cur, lim = int(bk[STOP_CUR]), int(bk[STOP_LIMIT])
        if bk[STOP_KIND] == 0:
            fired, bk[STOP_CUR] = cur + 1 >= lim, cur + 1
        else:
            fired, bk[STOP_CUR] = cur + n - 1 >= lim, cur + n
        bk[FIRED] = int(fired)
        elog[m] = (bits(v), n, new_best, 1)
        env_y[m] = log_y[n, m]
        env_state[m] = log_state[n, m]
    return elog, which


def close_phase1(rows, book, cols, stride, reset_post, last):
    """the counters behind the POST_EPISODE push (rows and book change in place)"""
    for m in range(rows.shape[0]):
        row, bk = rows[m], book[m]
        if not row[ACTIVE]:
            continue
        row[NSA] += cols
        if reset_post:
            row[USTEP] = 0
        if bk[RANDOM_INIT]:
            bk[INIT_OFF] += bk[INIT_INC]
        if bk[FIRED]:
            row[ACTIVE], row[HALT] = 0, 1
            continue
        row[HALT] = 0
        if not last and row[NSA] > row[NRT]:
            row[NSA] -= stride
