"""Child process of tests/test_gpu_pipeline_fluid.py::test_split_batch_ends_where_the_unsplit_run_does: the same twelve pipeline
steps with the fluid step's batch split into parts (PDEC_FLUID_SPLIT=2 is read once per process) on a caller's part stream made
with the pipeline's streams in one make_streams call.  argv[1]: the .npz to write the final state into."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(out):
    assert os.environ.get("PDEC_FLUID_SPLIT") == "2"
    import test_gpu_pipeline_fluid as t
    pkg = importlib.import_module("distributedconvrl-pde-control_amd")
    s_env, s_upd, s_part = pkg.make_streams((-1, 0, -1))
    p = t.split_run(pkg, part_streams=[s_part], streams=(s_env, s_upd))
    print(f"part streams {p.env.n_part_streams}", flush=True)
    np.savez(out, **t.final_state(p))
    p.close()


if __name__ == "__main__":
    main(sys.argv[1])
