"""Per-column terminal rows of the fluid env step (pdec_env_set_terminal_out on PDEC_PDE_FLUID_RK4; csrc/fluid_sense.hip:
fluid_feat_kernel): rows [B][A] = 1 on every column of a trajectory whose done flag of the step is set, under every
check_max_value mode, with and without a done array, with the batch split into parts; everything else the step writes bit for
bit what it writes without the buffer.

Shapes: FluidSetup(nx = 64 | 32, oversampling 2, dt = 2 / (16 nx), variance 0.08, 4 sensors per axis), B = 5; n = 64 takes the
wave-register transforms, n = 32 the LDS ones.  Fields: ic(3) by the device draw's rule (tests/fluid_ic_ref.py), rounded to
complex64, trajectory 3 multiplied by 30; actions N(0, 0.3^2).  On the CPU oracle the unscaled trajectories give max |reward| <=
0.14 and the scaled one 1.98 after one step, so max_value = 0.5 separates them by a factor >= 3.5 on both sides; the bound of
mode "y" is the geometric mean of the two sides' max |y^| after the oracle's step."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fluid_ic_ref import fields_of, jul, mem, pair, raw, vortex_table

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
B, SCALED = 5, 3
_ORACLE = {}


def _case(pkg, n):
    """inputs and the oracle's step, once per grid: y [B] complex (fp32-representable), a0, a1 [B, A, 1], the oracle's rewards
    [B, A] and max |y^| [B] after the step"""
    from oracle import fluid
    if n not in _ORACLE:
        _, cfg = pair(pkg, n)
        y = fields_of(cfg, vortex_table(11, 0, B, 3)).astype(np.complex64).astype(np.complex128)
        y[SCALED] *= 30.0
        y = y.astype(np.complex64).astype(np.complex128)
        rng = np.random.default_rng(n)
        A = 16
        a0 = (0.3 * rng.standard_normal((B, A, 1))).astype(np.float32).astype(np.float64)
        a1 = (0.3 * rng.standard_normal((B, A, 1))).astype(np.float32).astype(np.float64)
        r, ymax = [], []
        for b in range(B):
            yn = fluid.do_step(cfg, y[b], fluid.prepare_action(cfg, a1[b].T), 2)
            r.append(fluid.reward_function(cfg, yn, a1[b].T, a1[b].T - a0[b].T))
            ymax.append(np.abs(yn).max())
        _ORACLE[n] = (y, a0, a1, np.array(r), np.array(ymax))
    return _ORACLE[n]


def _dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda:0")


def _step(pkg, setup, dt, y, a0, a1, rows="new", done=True):
    """one step from (y, a0) under a1; rows: "new" = a [B, A] buffer prefilled with 7, None = no buffer.  Returns the outputs as
    host arrays (rows: None without a buffer)"""
    L = pkg._lib
    env = pkg.PDEenv(setup, B=B, dtype=dt, y0=_dev(mem(y), dt), autoreset=False)
    assert env.n_part_streams == 0               # the whole batch on one stream: what the split child is compared with
    buf = torch.full((B, setup.n_actuators), 7.0, dtype=dt, device="cuda:0") if rows == "new" else None
    if buf is not None:
        env.set_terminal_out(buf)
    if done:
        env.action.copy_(_dev(a0, dt))
        env(_dev(a1, dt))
        out = dict(y=env.y, p=env.p, state=env.state, reward=env.reward, done=env._done_flags)
    else:
        y2, st2, r2, p2 = torch.empty_like(env.y), torch.empty_like(env.state), torch.empty_like(env.reward), torch.empty_like(env.p)
        d1, d0 = _dev(a1, dt), _dev(a0, dt)
        L.check(env.lib.pdec_env_step(env.handle, L.ptr(env.y), L.ptr(d1), L.ptr(d0), None, L.ptr(y2), L.ptr(p2),
                                      L.ptr(st2), L.ptr(r2), None))
        out = dict(y=y2, p=p2, state=st2, reward=r2)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["rows"] = None if buf is None else buf.cpu().numpy()
    return env, buf, out


def _max_value_y(ymax):
    lo, hi = np.delete(ymax, SCALED).max(), ymax[SCALED]
    assert hi > 4 * lo, (lo, hi)
    return float(np.sqrt(lo * hi))


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [32, 64])
@pytest.mark.parametrize("mode", ["reward", "y"])
def test_rows_are_the_done_flags_and_the_oracles(pkg, mode, n, dt):
    y, a0, a1, r, ymax = _case(pkg, n)
    mv = 0.5 if mode == "reward" else _max_value_y(ymax)
    setup, _ = pair(pkg, n, max_value=mv, check_max_value=mode)
    oracle = [int(not np.all(np.abs(r[b]) <= mv)) for b in range(B)] if mode == "reward" else [int(not ymax[b] <= mv) for b in range(B)]
    if mode == "reward":
        rmax = np.abs(r).max(axis=1)
        print(f"{mode} n={n}: oracle max|r| unscaled {np.delete(rmax, SCALED).max():.4f}, scaled {rmax[SCALED]:.4f}, max_value {mv}")
        assert np.delete(rmax, SCALED).max() * 3.5 <= mv <= rmax[SCALED] / 3.5
    else:
        print(f"{mode} n={n}: oracle max|y^| unscaled {np.delete(ymax, SCALED).max():.4g}, scaled {ymax[SCALED]:.4g}, max_value {mv:.4g}")
    assert oracle == [0, 0, 0, 1, 0]
    env, buf, out = _step(pkg, setup, dt, y, a0, a1)
    A = setup.n_actuators
    assert out["done"].tolist() == [0, 0, 0, 1, 0] == oracle
    assert out["rows"].dtype == (np.float32 if dt == torch.float32 else np.float64)
    assert np.array_equal(out["rows"], np.repeat(out["done"].astype(out["rows"].dtype), A).reshape(B, A))
    # with / without the buffer: bit-identical outputs
    _, _, ref = _step(pkg, setup, dt, y, a0, a1, rows=None)
    for k in ("y", "p", "state", "reward", "done"):
        assert raw(out[k]) == raw(ref[k]), k
    # without a done array the rows are still written (mode "y": the environment's own flag slot)
    _, _, nod = _step(pkg, setup, dt, y, a0, a1, done=False)
    assert np.array_equal(nod["rows"], out["rows"])
    for k in ("y", "p", "state", "reward"):
        assert raw(nod[k]) == raw(ref[k]), k
    # NULL detaches: a buffer prefilled with 7 keeps its 7s
    buf.fill_(7.0)
    env.set_terminal_out(None)
    env(_dev(a0, dt))
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [32, 64])
def test_rows_are_zero_with_the_test_off(pkg, n, dt):
    y, a0, a1, _, _ = _case(pkg, n)
    setup, _ = pair(pkg, n, max_value=0.5, check_max_value="off")
    assert setup.env_cfg(B, 0).check_max_value == 0
    _, _, out = _step(pkg, setup, dt, y, a0, a1)
    assert out["done"].tolist() == [0] * B and bool((out["rows"] == 0).all())
    _, _, nod = _step(pkg, setup, dt, y, a0, a1, done=False)
    assert bool((nod["rows"] == 0).all())


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [32, 64])
@pytest.mark.parametrize("mode", ["reward", "y"])
def test_a_nan_cell_raises_its_trajectorys_rows_only(pkg, mode, n, dt):
    """!(|r| <= max_value) counts a NaN; rows are compared with rows (no oracle)"""
    y, a0, a1, _, ymax = _case(pkg, n)
    mv = 0.5 if mode == "reward" else _max_value_y(ymax)
    setup, _ = pair(pkg, n, max_value=mv, check_max_value=mode)
    _, _, ref = _step(pkg, setup, dt, y, a0, a1)
    ym = mem(y)
    ym[1, 3, 5, 0] = np.nan
    env = pkg.PDEenv(setup, B=B, dtype=dt, y0=_dev(ym, dt), autoreset=False)
    buf = torch.full((B, setup.n_actuators), 7.0, dtype=dt, device="cuda:0")
    env.set_terminal_out(buf)
    env.action.copy_(_dev(a0, dt))
    env(_dev(a1, dt))
    torch.cuda.synchronize()
    rows = buf.cpu().numpy()
    assert bool((rows[1] == 1).all()) and env._done_flags.cpu().tolist() == [0, 1, 0, 1, 0]
    got = dict(y=env.y, p=env.p, state=env.state, reward=env.reward, rows=buf)
    for b in (0, 2, 3, 4):
        for k, v in got.items():
            assert raw(v[b]) == raw(ref[k][b]), (b, k)


def test_split_batch_writes_every_parts_slice(pkg, tmp_path):
    """B = 5 as 2 + 3 (PDEC_FLUID_SPLIT=2 in a child process, the second part on a caller's part stream): rows and all outputs
    bit-identical to the unsplit step's"""
    for n, dt, mode in ((64, torch.float32, "reward"), (32, torch.float64, "y"), (64, torch.float64, "off")):
        y, a0, a1, _, ymax = _case(pkg, n)
        mv = _max_value_y(ymax) if mode == "y" else 0.5
        setup, _ = pair(pkg, n, max_value=mv, check_max_value=mode)
        _, _, out = _step(pkg, setup, dt, y, a0, a1)
        name = f"n{n}_{mode}"
        np.savez(tmp_path / f"{name}_in.npz", n=n, f64=int(dt == torch.float64), mode=mode, max_value=mv, y=mem(y), a0=a0, a1=a1)
        np.savez(tmp_path / f"{name}_out.npz", **out)
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "fluid_terminal_child.py"), str(tmp_path)],
                       env=dict(os.environ, PDEC_FLUID_SPLIT="2"), capture_output=True, text=True, timeout=120, cwd=os.path.dirname(here))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("split ok") == 3, r.stdout[-2000:]
