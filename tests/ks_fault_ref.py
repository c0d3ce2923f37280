"""The reference of test_gpu_ks_faults.py: one control step of the KS environment under actuator and sensor faults, composed from
the unchanged pieces of oracle/ks.py -- prepare_action on gain * action, the row's integrator, reward_function on the commanded
action and the true field -- and the featurize rule of KSSetup.jl:190-229 restated on gain * sensor_dots + bias.  numpy only; the
oracle module is passed in.  Each `wrong` names one mistake a kernel could make; test_ks_fault_table.py shows that every one of them
moves the step by many bounds of the GPU comparison."""
import numpy as np

import ks_geometry_cases as kc

WRONG = ("actuator_index", "bias_after_scale", "reward_sees_faults", "punish_applied_action")


def window_rows(cfg, sensors):
    """rows [-w .. w] of featurize (KSSetup.jl:204-207): row i of actuator a reads sensor (a2s[a] - i) mod S"""
    w = cfg.window_size // 2
    a2s = np.asarray(cfg.actuators_to_sensors) - 1
    return np.stack([np.roll(sensors, i) for i in range(-w, w + 1)])[:, a2s]


def featurize(ks, cfg, y, sensor_gain, sensor_bias, prev_state=None, wrong=None):
    """(gain[s] * dot_s + bias[s]) / max_value in the window of every actuator; temporal_steps > 1 stacks them on the previous
    state's newest rows, which keep the values they were written with (oracle/ks.py: featurize)"""
    d = ks.sensor_dots(cfg, y)
    S = len(d)
    if wrong == "bias_after_scale":
        fresh = window_rows(cfg, sensor_gain * d / cfg.max_value + sensor_bias)
    elif wrong == "actuator_index":         # every row of actuator a through the arrays' entry a (A <= S on every row)
        w, a2s = cfg.window_size // 2, np.asarray(cfg.actuators_to_sensors) - 1
        a = np.arange(len(a2s))
        fresh = np.stack([(sensor_gain[a] * d[(a2s - i) % S] + sensor_bias[a]) / cfg.max_value for i in range(-w, w + 1)])
    else:
        fresh = window_rows(cfg, (sensor_gain * d + sensor_bias) / cfg.max_value)
    T = getattr(cfg, "temporal_steps", 1)
    if T > 1:
        if prev_state is None:
            return np.concatenate([fresh] * T)
        prev = np.asarray(prev_state, dtype=np.float64)
        return np.concatenate([fresh, prev[:prev.shape[0] - fresh.shape[0], :]])
    return fresh


def env_step(ks, cfg, case, y, action_prev, action, actuator_gain, sensor_gain, sensor_bias, prev_state=None, wrong=None, p=None):
    """(env::PDEenv)(action) of trajectory b with its rows of the three arrays; action, action_prev [A].  p: integrate on this
    forcing instead of the reference's own (the teacher-forced comparison feeds the device's)"""
    action, action_prev = np.asarray(action, dtype=np.float64), np.asarray(action_prev, dtype=np.float64)
    applied = actuator_gain * action
    p_ref = ks.prepare_action(cfg, applied[None])
    y_new = kc.oracle_step(ks, cfg, case, y, p_ref if p is None else p)
    punished = applied if wrong == "punish_applied_action" else action
    punished_prev = actuator_gain * action_prev if wrong == "punish_applied_action" else action_prev
    if wrong == "reward_sees_faults":       # the reward's |6 d|^1.3 on the faulty read-out: the field that has those dots is not
        d = ks.sensor_dots(cfg, y_new)      # needed, reward_function is restated on them (KSSetup.jl:162-178)
        a2s = np.asarray(cfg.actuators_to_sensors) - 1
        seen = (sensor_gain * d + sensor_bias)[a2s]
        reward = -np.abs(6 * seen) ** 1.3 / (cfg.max_value * 3) - cfg.action_punish * action ** 2 \
            - cfg.delta_action_punish * (action - action_prev) ** 2
    else:
        reward = ks.reward_function(cfg, y_new, punished[None], (punished - punished_prev)[None])
    state = featurize(ks, cfg, y_new, sensor_gain, sensor_bias, prev_state, wrong)
    return dict(y=y_new, p=p_ref, reward=reward, state=state, applied=applied)
