"""The host logic of a fluid population (population.py): the vortex tables of a block of episodes drawn from every member's own
generator, the generators set back to what each member consumed, and the bytes behind max_log_bytes.  No GPU."""
import importlib

import numpy as np
import pytest


@pytest.fixture(scope="module")
def pop(pkg):
    return importlib.import_module(pkg.__name__ + ".population")


@pytest.fixture(scope="module")
def setup(pkg):
    return pkg.FluidSetup(nx=16, sensors_per_axis=4, oversampling=1)


@pytest.mark.parametrize("caseno,nv", [(3, 30), (4, 50)])
def test_block_tables_are_successive_solo_draws(pop, setup, caseno, nv):
    L, seeds = 4, [5, None, 9]
    rngs = [None if s is None else np.random.default_rng(s) for s in seeds]
    tables, states = pop.draw_block_tables(setup, rngs, L, caseno)
    assert tables.shape == (L, len(seeds), nv, 4) and tables.dtype == np.float64 and tables.flags.c_contiguous
    assert states[1] is None and np.array_equal(tables[:, 1], np.ones((L, nv, 4)))      # nothing drawn: a harmless table
    for m, s in enumerate(seeds):
        if s is None:
            continue
        solo = np.random.default_rng(s)
        assert states[m][0] == np.random.default_rng(s).bit_generator.state
        for e in range(L):
            assert np.array_equal(tables[e, m], setup.ic_vortices(caseno, solo, 1)[0]), (m, e)
            assert states[m][e + 1] == solo.bit_generator.state
    assert not np.array_equal(tables[0, 0], tables[0, 2]) and not np.array_equal(tables[0, 0], tables[1, 0])


def test_restore_leaves_each_generator_behind_what_its_member_consumed(pop, setup):
    L, seeds = 5, [1, 2, 3, 4]
    consumed = [0, 2, 5, 3]
    rngs = [np.random.default_rng(s) for s in seeds]
    rngs[3] = None                                       # a member that draws nothing is left alone
    tables, states = pop.draw_block_tables(setup, rngs, L, 3)
    pop.restore_block_rngs(rngs, states, consumed)
    for m, (s, k) in enumerate(zip(seeds, consumed)):
        if rngs[m] is None:
            continue
        solo = np.random.default_rng(s)
        for _ in range(k):
            setup.ic_vortices(3, solo, 1)
        # the next draw is the solo run's draw k + 1
        assert np.array_equal(setup.ic_vortices(3, rngs[m], 1), setup.ic_vortices(3, solo, 1)), m
        assert rngs[m].random() == solo.random()


def test_log_bytes_of_fluid_8_by_hand(pkg, pop):
    """Fluid_8: 128 x 128 complex spectra (2 x 8 bytes per cell), 64 actuators with 9 state rows and one action row, and 301 control
    steps: te / dt = 300, but the step loop's floating-point sum of 300 x 0.02 stays below 6.0 (run._episode_steps).  Per member:
    y 302 slots, state 302, action 302, p 301, reward 301; the best rows: action, p, y, reward, 301 each."""
    st = pkg.FluidSetup.Fluid_8()
    run = importlib.import_module(pkg.__name__ + ".run")
    T = run._episode_steps(st)
    assert T == 301
    spectrum = 128 * 128 * 2 * 8
    assert spectrum == 262144
    logs = 302 * spectrum + 302 * 64 * 9 * 8 + 302 * 64 * 8 + 301 * spectrum + 301 * 64 * 8
    best = 301 * (64 * 8 + spectrum + spectrum + 64 * 8)
    assert pop.episode_log_bytes(st, T, 8) == (logs, best)
    assert 158e6 < 603 * spectrum < 159e6                  # the (T + 1) + T full spectra are what counts
    # a 1-D setup is far below any such limit
    lk, bk = pop.episode_log_bytes(pkg.KSSetup.KS22(), 50, 8)
    assert lk + bk < 1 << 20
