"""Child process of test_gpu_fluid_geometry.py::test_switch_rows_match_the_oracle: started with ONE of the documented switches set
(PDEC_FLUID_K2P=0, PDEC_FLUID_FUSE=1, PDEC_FLUID_FUSE=0 or PDEC_FLUID_LDS_FFT=1; csrc/fluid.hip and fluid_wave.hip read each once per process), it
runs the rows of fluid_geometry_cases.SWITCH_CASES that belong to that switch in both precisions on the inputs the parent left
in DIR (<row>_y.npy, <row>_p.npy: complex [B, n, n]) and writes, per row and precision, <row>_<prec>_rhs.npy and / or
<row>_<prec>_step.npy (complex128 [B, n, n]) plus meta.json: the switch as the process saw it, pdec_debug_fluid_plan of every
environment, the do_step flags and whether the inputs were left untouched.  The parent holds the arrays to oracle/fluid.py.
Also holds the device helpers the parent's in-process tests use.  usage: python fluid_geometry_child.py DIR"""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for path in (HERE, os.path.dirname(HERE)):
    if path not in sys.path:
        sys.path.insert(0, path)


def torch_dtype(torch, prec):
    return torch.float64 if prec == "f64" else torch.float32


def mem(z):
    """Julia complex [.., ny, nx] -> memory [.., nx, ny, 2]"""
    z = np.swapaxes(np.asarray(z, dtype=np.complex128), -1, -2)
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1))


def jul(t):
    """memory [.., nx, ny, 2] -> Julia complex128 [.., ny, nx]"""
    a = t.detach().cpu().numpy().astype(np.float64)
    return np.swapaxes(a[..., 0] + 1j * a[..., 1], -1, -2)


def to_dev(torch, a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda:0")


def device_plan(pkg, env):
    """the twelve numbers of pdec_debug_fluid_plan (include/pdeconv_debug.h) for this environment"""
    out = (C.c_int32 * 12)()
    pkg._lib.check(env.lib.pdec_debug_fluid_plan(env.handle, out))
    return [int(v) for v in out]


def device_rhs(torch, env, y, p, dtype):
    """env.rhs on host fields; (result, input untouched)"""
    yin, pin = to_dev(torch, mem(y), dtype), to_dev(torch, mem(p), dtype)
    out = jul(env.rhs(yin, pin))
    return out, bool(np.array_equal(jul(yin), y) and np.array_equal(jul(pin), p))


def device_step(torch, env, y, p, dtype):
    """env.do_step on host fields; (result, flags, input untouched)"""
    yin, pin = to_dev(torch, mem(y), dtype), to_dev(torch, mem(p), dtype)
    out, flags = env.do_step(yin, pin)
    return jul(out), [int(f) for f in flags.cpu().tolist()], bool(np.array_equal(jul(yin), y) and np.array_equal(jul(pin), p))


def main(out_dir):
    import torch

    import fluid_geometry_cases as fc
    pkg = importlib.import_module("distributedconvrl-pde-control_amd")
    seen = {k: os.environ[k] for k in fc.ENV_NAMES if k in os.environ}
    assert len(seen) == 1 and list(seen.items())[0] in fc.SWITCHES, seen
    (var, value), = seen.items()
    meta = dict(env=seen, rows={})
    setups = {}
    for row in fc.switch_rows(var, value):
        c = fc.SWITCH_CASES[row]
        y, p = np.load(os.path.join(out_dir, f"{row}_y.npy")), np.load(os.path.join(out_dir, f"{row}_p.npy"))
        key = (c.n, c.ifpad, c.K)
        if key not in setups:
            setups[key] = pkg.FluidSetup(nx=c.n, ifpad=c.ifpad, sensors_per_axis=c.spa, variance=c.variance, oversampling=c.K,
                                         dt=fc.dt_of(c), window_size=c.window, temporal_steps=c.tsteps)
        for prec in fc.PRECS:
            dt = torch_dtype(torch, prec)
            env = pkg.PDEenv(setups[key], B=c.B, dtype=dt, autoreset=False)
            m = dict(plan=device_plan(pkg, env))
            if "rhs" in c.run:
                out, m["rhs_input_untouched"] = device_rhs(torch, env, y, p, dt)
                np.save(os.path.join(out_dir, f"{row}_{prec}_rhs.npy"), out)
            if "step" in c.run:
                out, m["flags"], m["step_input_untouched"] = device_step(torch, env, y, p, dt)
                np.save(os.path.join(out_dir, f"{row}_{prec}_step.npy"), out)
            torch.cuda.synchronize()
            meta["rows"][f"{row} {prec}"] = m
            env.close()
    with open(os.path.join(out_dir, "meta.json"), "w") as fh:
        json.dump(meta, fh)


if __name__ == "__main__":
    main(sys.argv[1])
