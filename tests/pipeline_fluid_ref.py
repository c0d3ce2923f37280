"""The 2-D fluid as a third env oracle of the teacher-forced pipeline reference (tests/pipeline_ref.py, which this file imports
and does not edit): FluidEnvRef has the interface check_trace expects -- B, A, tol, featurize, step, random_init -- built on
oracle/fluid.py in the device layouts.  Test infrastructure, host only.

Layouts: y [B, nx, ny, 2] (the memory image of the Julia ComplexF64[ny, nx]: transposed, (re, im) trailing), state [B A, 9],
action [B A, 1], reward [B A]; done_b = not all(|r_b| <= max_value) (check_max_value "reward", a NaN counts).  random_init(seed,
off) is pdec_fluid_ic_rng's rule (tests/fluid_ic_ref.py).

Tolerances are the ones the env-step tests of the library hold it to: fp32 -- y, state, reward at 1e-5 max(1, |ref|)
(tests/test_gpu_fluid_fp32.py::test_closures_and_env_step_f32_match_oracle); fp64 -- 1e-11 max(1, |ref|)
(tests/test_gpu_fluid.py: y 1e-11 |ref|, reward and state 1e-11 max(1, |ref|) behind one env step)."""
import numpy as np

from fluid_ic_ref import fields_of, jul, mem, vortex_table
from oracle import fluid

TOL32 = dict(y=1e-5, state=1e-5, reward=1e-5)
TOL64 = dict(y=1e-11, state=1e-11, reward=1e-11)


def fluid_config(setup):
    """the oracle configuration of a FluidSetup"""
    return fluid.FluidConfig(nx=setup.nx, Lx=setup.Lx, Ly=setup.Ly, nu=setup.nu, dt=setup.dt, ifpad=setup.ifpad,
                             sensors_per_axis=setup.sensors_per_axis, variance=setup.variance, agent_power=setup.agent_power,
                             action_punish=setup.action_punish, delta_action_punish=setup.delta_action_punish,
                             window_size=setup.window_size, te=setup.te, max_value=setup.max_value,
                             oversampling=setup.oversampling)


class FluidEnvRef:
    def __init__(self, cfg, B, fp64=False, caseno=3):
        self.cfg, self.B, self.caseno = cfg, int(B), int(caseno)
        self.A = len(cfg.sensor_positions)
        self.tol = dict(TOL64 if fp64 else TOL32)

    def featurize(self, y):
        return np.concatenate([fluid.featurize(self.cfg, yb).T for yb in jul(np.asarray(y, np.float64))])

    def step(self, y, a_prev, a, s_prev=None):
        cfg, B, A = self.cfg, self.B, self.A
        yj = jul(np.asarray(y, np.float64))
        a, a_prev = (np.asarray(x, np.float64).reshape(B, A, -1).transpose(0, 2, 1) for x in (a, a_prev))     # [B, na, A]
        yn, r = [], []
        with np.errstate(all="ignore"):
            for b in range(B):
                yb = fluid.do_step(cfg, yj[b], fluid.prepare_action(cfg, a[b]), cfg.oversampling)
                yn.append(yb)
                r.append(fluid.reward_function(cfg, yb, a[b], a[b] - a_prev[b]))
        yn, r = np.stack(yn), np.stack(r)
        done = np.array([not np.all(np.abs(rb) <= cfg.max_value) for rb in r])
        state = np.concatenate([fluid.featurize(cfg, yb).T for yb in yn])
        return dict(y=mem(yn), state=state, reward=r.reshape(-1), done=done)

    def random_init(self, seed, off):
        return mem(fields_of(self.cfg, vortex_table(seed, off, self.B, self.caseno, self.cfg.Lx, self.cfg.Ly)))
