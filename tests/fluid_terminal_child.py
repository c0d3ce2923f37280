"""Child process of tests/test_gpu_fluid_terminal_rows.py: the fluid env step with its batch split into parts (PDEC_FLUID_SPLIT is
read once per process, hence the fresh one).  argv[1]: a directory holding, per case `name`, `name_in.npz` (n, f64, mode,
max_value, y, a0, a1) and `name_out.npz` -- the arrays of the UNSPLIT step (y, p, state, reward, done, rows) --, all written by the
parent.  B = 5 steps as 2 + 3, the second part on a caller's part stream; the step is issued twice, with and without a done
array.  Prints one `split ok` line per case."""
import glob
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(d):
    from fluid_ic_ref import pair, raw
    assert os.environ.get("PDEC_FLUID_SPLIT") == "2"
    pkg = importlib.import_module("distributedconvrl-pde-control_amd")
    L = pkg._lib
    s_env, s_upd, s_part = pkg.make_streams((-1, 0, -1))
    for fin in sorted(glob.glob(os.path.join(d, "*_in.npz"))):
        name = os.path.basename(fin)[:-7]
        i, o = np.load(fin), np.load(os.path.join(d, name + "_out.npz"))
        dt = torch.float64 if int(i["f64"]) else torch.float32
        mode = str(i["mode"])
        setup, _ = pair(pkg, int(i["n"]), max_value=float(i["max_value"]), check_max_value=mode)
        dev = lambda a, t=dt: torch.as_tensor(np.ascontiguousarray(a), dtype=t, device="cuda:0")      # noqa: E731
        env = pkg.PDEenv(setup, B=5, dtype=dt, y0=dev(i["y"]), stream=s_env, part_streams=[s_part], autoreset=False)
        assert env.n_part_streams == 1
        with torch.cuda.stream(s_env):
            rows = torch.full((5, setup.n_actuators), 7.0, dtype=dt, device="cuda:0")
            env.set_terminal_out(rows)
            env.action.copy_(dev(i["a0"]))
            env(dev(i["a1"]))
        s_env.synchronize()
        got = dict(y=env.y, p=env.p, state=env.state, reward=env.reward, done=env._done_flags, rows=rows)
        for k, v in got.items():
            assert raw(v) == o[k].tobytes(), (name, k)
        # the same step without a done array: the rows are still written (mode "y": from the children's own flag slots)
        with torch.cuda.stream(s_env):
            rows.fill_(7.0)
            y2, st2, r2 = torch.empty_like(env.y), torch.empty_like(env.state), torch.empty_like(env.reward)
            dy, d1, d0 = dev(i["y"]), dev(i["a1"]), dev(i["a0"])
            L.check(env.lib.pdec_env_step(env.handle, L.ptr(dy), L.ptr(d1), L.ptr(d0), None, L.ptr(y2), None, L.ptr(st2),
                                          L.ptr(r2), None))
        s_env.synchronize()
        assert raw(rows) == o["rows"].tobytes() and raw(y2) == o["y"].tobytes() and raw(r2) == o["reward"].tobytes(), name
        assert raw(st2) == o["state"].tobytes(), name
        print(f"split ok {name}", flush=True)
        env.close()


if __name__ == "__main__":
    main(sys.argv[1])
