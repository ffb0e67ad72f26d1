"""The four flights of the per-drone gain tests (gpd_set_pid_gains) on the CPU reference
tests/cmd_ref.CmdRefAviary, whose ``env.ctrl[k]`` (RefDSLPID) carry their own six coefficient arrays.
Test infrastructure only: tests/test_pid_gains_host.py checks the flights' conditions on the oracle
alone, tests/test_gpu_pid_gains.py flies them on the device.  Every reference is computed once.

Gain rows [N, 18] (a row = P/I/D_COEFF_FOR, P/I/D_COEFF_TOR) come from one recipe, ``gain_rows``.
"""
import functools

import numpy as np

from oracle import ref_pid
from tests.cmd_ref import CmdRefAviary
from tests.test_gpu_cmd_rollout import XYZ3
from tests.test_gpu_cmd_step import _oracle20, _waypoints
from tests.test_gpu_wide import _spiral

DEFAULT = np.array([ref_pid.P_COEFF_FOR, ref_pid.I_COEFF_FOR, ref_pid.D_COEFF_FOR,
                    ref_pid.P_COEFF_TOR, ref_pid.I_COEFF_TOR, ref_pid.D_COEFF_TOR])   # [6, 3]
ATTRS = ("P_COEFF_FOR", "I_COEFF_FOR", "D_COEFF_FOR", "P_COEFF_TOR", "I_COEFF_TOR", "D_COEFF_TOR")
START1 = np.array([[0, 0, 0.5]])

# name: mode, E, D, T, ctrl_freq, aero, start positions [D, 3], seed of the gain rows
FLIGHTS = {
    "wp3x3": dict(mode="waypoint", E=3, D=3, T=16, ctrl_freq=48, aero=(), xyz=XYZ3, seed=5),
    "wp2x65": dict(mode="waypoint", E=2, D=65, T=4, ctrl_freq=48, aero=("no_drone_contact",), xyz=_spiral(65), seed=6),
    "vel5x2": dict(mode="vel", E=5, D=2, T=16, ctrl_freq=240, aero=(), xyz=np.array([[0, 0, 0.5], [1, 0, 0.5]]), seed=7),
    "wp70x1": dict(mode="waypoint", E=70, D=1, T=8, ctrl_freq=48, aero=(), xyz=START1, seed=8),
}


def gain_rows(seed, n):
    """The tests' gain rows [n, 18]: the defaults times U[0.5, 1.5] per coefficient; I_COEFF_TOR x and y
    (0 by default: a zero column would hide a mix-up) drawn from U[0, 100]."""
    rng = np.random.default_rng(seed)
    g = DEFAULT[None] * rng.uniform(0.5, 1.5, (n, 6, 3))
    g[:, 4, 0:2] = rng.uniform(0, 100, (n, 2))
    return np.ascontiguousarray(g.reshape(n, 18))


def default_rows(n):
    return np.ascontiguousarray(np.broadcast_to(DEFAULT.reshape(1, 18), (n, 18)))


@functools.lru_cache(maxsize=None)
def actions(name):
    """The flight's commands [T, E, D, w] (float32 for "vel", float64 waypoint rows)."""
    f = FLIGHTS[name]
    E, D, T = f["E"], f["D"], f["T"]
    if f["mode"] == "vel":      # tests/test_gpu_cmd_step.py test_vel_mode_parity_pyb's actions
        rng = np.random.default_rng(22)
        a = rng.uniform(-1, 1, (T, E, D, 4)).astype(np.float32)
        a[:, 0, 0, 0:3] = 0.0
    elif name == "wp70x1":      # every env flies the same rows from the same start
        a = np.array([[_waypoints(START1, t, 0) for _ in range(E)] for t in range(T)])
    else:
        a = np.array([[_waypoints(f["xyz"], t, e) for e in range(E)] for t in range(T)])
    a.setflags(write=False)
    return a


def set_ref_gains(envs, rows):
    """Give drone d of env e row e * D + d."""
    n = 0
    for env in envs:
        for c in env.ctrl:
            for k, attr in enumerate(ATTRS):
                setattr(c, attr, np.array(rows[n, 3 * k:3 * k + 3], dtype=np.float64))
            n += 1


@functools.lru_cache(maxsize=None)
def reference(name, tuned=True):
    """The flight on the reference with the recipe's gains (``tuned``) or the defaults:
    dict(traj [T, N, 20] state vectors after every step, ctrl [N, 9] controller state at the end)."""
    f = FLIGHTS[name]
    E, D, T = f["E"], f["D"], f["T"]
    envs = [CmdRefAviary(num_drones=D, drones_per_env=D, integrator="bullet", aero=f["aero"], ctrl_freq=f["ctrl_freq"],
                         initial_xyzs=f["xyz"]) for _ in range(E)]
    if tuned:
        set_ref_gains(envs, gain_rows(f["seed"], E * D))
    a = actions(name)
    traj = []
    for t in range(T):
        for e, env in enumerate(envs):
            env.cmd_step(f["mode"], a[t, e])
        traj.append(_oracle20(envs))
    out = dict(traj=np.array(traj), ctrl=np.concatenate([e.ctrl_state() for e in envs]))
    for v in out.values():
        v.setflags(write=False)
    return out
