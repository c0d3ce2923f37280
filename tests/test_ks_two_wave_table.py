"""The two-wave N = 256 KS step held without a GPU and without the library (ks_two_wave_model.py): the engine's data flow is a
256-point DFT in the mode order the kernel loads its per-mode constants by, forward and back; the host restatement of the route
(`route`, what the documents and the GPU tests are written against) reaches the new kernel for ONE combination of everything the
launch reads; the source names every term of that rule and reads the flag in one function only -- which ties the restatement to
`ks_step_engine` by its terms, not by its operators: the check of the rule itself is test_gpu_ks_two_wave.py's
test_other_environments_keep_their_kernel, on the setter's `effective`, which is that function's value --; and the C ABI, the Python layer, the pipeline
and the README's table of switches have the entry."""
import inspect
import itertools
import os
import re

import numpy as np

import ks_two_wave_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributedconvrl-pde-control_amd", "csrc")


def test_the_data_flow_is_the_256_point_transform():
    rng = np.random.default_rng(0)
    x = rng.normal(size=m.N) + 1j * rng.normal(size=m.N)
    a = np.stack([x[m.phys_index(j)] for j in range(2)])
    f = m.forward(a)
    want = np.fft.fft(x)
    modes = np.concatenate([m.mode_index(j) for j in range(2)])
    assert sorted(modes.tolist()) == list(range(m.N))                       # every mode is held exactly once
    assert sorted(np.concatenate([m.phys_index(j) for j in range(2)]).tolist()) == list(range(m.N))
    for j in range(2):                                                      # 8 levels of fp64 butterflies: 1e-13 is ~50 ulp of |X|
        assert np.abs(f[j] - want[m.mode_index(j)]).max() <= 1e-13 * np.abs(want).max()
    b = m.inverse(f)
    for j in range(2):
        assert np.abs(b[j] / m.N - x[m.phys_index(j)]).max() <= 1e-14 * np.abs(x).max() * 8


def test_one_combination_reaches_the_two_wave_kernel():
    names = list(m.AXES)
    hits = []
    for combo in itertools.product(*m.AXES.values()):
        kw = dict(zip(names, combo))
        r = m.route(**kw)
        if r == "Wave256x2":
            hits.append(kw)
        elif kw["pde"] == "ks_cnab2":                                       # every other launch keeps the environment's engine
            assert r == m.engine(kw["N"], kw["lds_fft"], kw["generic_fft"])
    assert hits == [dict(asked=True, fused=True, pde="ks_cnab2", N=256, dtype="f32", lds_fft=False, generic_fft=False, share=False,
                         mu=False, faults=False, member=False)]


def test_the_source_states_the_rule_once():
    with open(os.path.join(CSRC, "env.hpp")) as f:
        hpp = f.read()
    rule = re.search(r"inline KsEngine ks_step_engine\(const Env& E, bool fused\) \{(.*?)\n\}", hpp, re.S).group(1)
    for term in ("E.two_wave", "fused", "PDEC_PDE_KS_CNAB2", "E.engine == KsEngine::Wave256", "PDEC_F32", "!E.share_simd", "!E.member", "!E.mu_b",
                 "!E.faults()"):
        assert term in rule, term
    srcs = {n: open(os.path.join(CSRC, n)).read() for n in os.listdir(CSRC) if n.endswith((".hip", ".hpp"))}
    assert sum(s.count("E.two_wave") + s.count("E->two_wave") for s in srcs.values()) == 2          # the rule and the setter
    assert "ks_step_engine(E, fused)" in srcs["ks_step.hip"] and "ks_step_engine(*E, true)" in srcs["env.hip"]
    # the rollout keeps the environment's engine: only the step's list knows the new one
    assert "with_ks_engine<T>(E.engine" in srcs["ks_rollout.hip"] and "Wave256x2" not in srcs["ks_rollout.hip"]
    assert "with_ks_engine<T, true>(engine" in srcs["ks_step.hip"]


def test_the_entry_is_declared_and_bound(pkg):
    import ctypes as C
    with open(os.path.join(ROOT, "include", "pdeconv.h")) as f:
        header = f.read()
    assert re.search(r"int pdec_env_set_two_wave_step\(pdec_handle env, int on, int\* effective\);", header)
    sig = pkg._lib.SIGNATURES["pdec_env_set_two_wave_step"]
    assert len(sig) == 3 and sig[1] is C.c_int
    assert callable(pkg.PDEenv.set_two_wave_step)
    src = inspect.getsource(pkg.TrainPipeline.__init__)
    assert 'os.environ.get("PDEC_TWO_WAVE", "1") != "0"' in src and "pdec_env_set_two_wave_step" in src
    with open(os.path.join(ROOT, "README.md")) as f:
        assert re.search(r"^\| `PDEC_TWO_WAVE=0` \|", f.read(), re.M)
