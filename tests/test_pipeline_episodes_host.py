"""Host-side checks of the pipeline's episode bookkeeping (no GPU): the C ABI of the episode ledger is exported and bound,
and the NumPy restatement of the 2-D Keller-Segel initialiser that the GPU test compares against is the setup's own
generate_random_init on the Philox coefficients."""
import ctypes
import os

import numpy as np

from oracle import rng as orng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEDGER = ("pdec_ledger_create", "pdec_ledger_step", "pdec_ledger_snapshot", "pdec_ledger_close", "pdec_ledger_discard",
          "pdec_ledger_read", "pdec_ledger_best", "pdec_ledger_best_params")


def test_ledger_abi_is_exported_and_bound(pkg):
    lib = ctypes.CDLL(pkg._lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pdeconv.h")).read()
    for name in LEDGER:
        assert hasattr(lib, name), name
        assert name + "(" in hdr and name in pkg._lib.SIGNATURES, name


def test_pipeline_accepts_the_episode_arguments(pkg):
    import inspect
    sig = inspect.signature(pkg.TrainPipeline.__init__).parameters
    defaults = dict(log_episodes=0, min_best_episode=0, random_init=False, init_seed=0, init_rng=None, init_rank=(0, 1))
    for k, v in defaults.items():
        assert sig[k].default == v, k
    for name in ("episode_returns", "best_actor"):
        assert callable(getattr(pkg.TrainPipeline, name))


class _Rng:
    """hands generate_random_init the Philox coefficients, un-normalised (it normalises them itself)"""

    def __init__(self, a):
        self.a = a

    def uniform(self, lo, hi, shape):
        return self.a.reshape(shape)


def test_kseg2d_restatement_is_generate_random_init(pkg):
    setup = pkg.KellerSegel2DSetup(nx=64, ny=48)
    nsx, nsy = int(np.ceil(setup.Lx / 3)), int(np.ceil(setup.ny * setup.dx / 3))
    B, nc = 3, 2 * (nsx + nsy)
    a = orng.random_init_coefficients(5, 77, B, nc)
    want = setup.generate_random_init(_Rng(a), B)                  # [B, 2, ny, nx]
    assert want.shape == (B, 2, setup.ny, setup.nx)
    # the restatement the device kernel is held to: 1 + x-profile + y-profile per species
    xx, yy = setup.dx * np.arange(1, setup.nx + 1), setup.dx * np.arange(1, setup.ny + 1)
    a3 = a.reshape(B, 2, nsx + nsy)
    px = sum(a3[:, :, i - 1, None] * np.sin(i * xx / (2 * np.pi * (setup.Lx / 22)))[None, None, :] for i in range(1, nsx + 1))
    py = sum(a3[:, :, nsx + i - 1, None] * np.sin(i * yy / (2 * np.pi * (setup.ny * setup.dx / 22)))[None, None, :]
             for i in range(1, nsy + 1))
    got = (1.0 + px[:, :, None, :]) + py[:, :, :, None]
    assert np.abs(got - want).max() <= 1e-13
