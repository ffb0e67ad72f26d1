"""A batched sweep of DSLPIDControl gains: E candidate gain sets fly the same circle at once.

E single-drone Physics.PYB envs (240 / 48) all track the circle of examples/pid.py in waypoint
mode.  Every env's drone owns its own controller coefficients (``set_pid_gains``): candidate 0
flies the default gains, candidates 1 .. E-1 the defaults times exp(U[-S, S]) per coefficient.
The whole flight is one ``cmd_rollout(..., record=False, metrics=True)`` call, whose per-drone
tracking figures rank the candidates.  One JSON line is printed (and written to ``--out``).

    python examples/pid_sweep.py --envs 4096 --steps 192 --spread 0.5
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gym_pybullet_drones_routing_amd import _lib  # noqa: E402
from gym_pybullet_drones_routing_amd.enums import ActionType, Physics  # noqa: E402
from gym_pybullet_drones_routing_amd.sim import PID_GAIN_KEYWORDS, BatchedAviarySim, pid_gain_rows  # noqa: E402

PYB_FREQ, CTRL_FREQ, RADIUS, PERIOD_SEC = 240, 48, 0.3, 10.0


def candidates(n, spread, seed):
    """Gain rows [n, 18]: row 0 the defaults, the others the defaults times exp(U[-spread, spread])."""
    rows = pid_gain_rows(n, 1, _lib.default_pid_params())
    rng = np.random.default_rng(seed)
    rows[1:] *= np.exp(rng.uniform(-spread, spread, (n - 1, rows.shape[1])))
    return rows


def run(envs=256, steps=192, spread=0.5, seed=0, out=None):
    E, T = int(envs), int(steps)
    # examples/pid.py's first drone: it starts on the circle, 10 cm up
    init_xyzs = np.array([[RADIUS * np.cos(np.pi / 2), RADIUS * np.sin(np.pi / 2) - RADIUS, 0.1]])
    sim = BatchedAviarySim(n_envs=E, drones_per_env=1, pyb_freq=PYB_FREQ, ctrl_freq=CTRL_FREQ, act=ActionType.VEL,
                           task="none", physics=Physics.PYB, autoreset=False, initial_xyzs=init_xyzs)
    dev = sim.device
    rows = candidates(E, spread, seed)
    g = rows.reshape(E, 1, 6, 3)
    sim.set_pid_gains(**{name: g[:, :, k] for k, name in enumerate(PID_GAIN_KEYWORDS)})
    # every candidate gets the same waypoint rows [T, E, 1, 7]: target_pos(3), target yaw, target_vel(3) = 0
    t = torch.arange(T, device=dev, dtype=torch.float64) / CTRL_FREQ
    ang = 2 * np.pi * t / PERIOD_SEC + np.pi / 2
    wp = torch.zeros((T, E, 1, 7), dtype=torch.float64, device=dev)
    wp[..., 0] = (RADIUS * torch.cos(ang)).reshape(T, 1, 1)
    wp[..., 1] = (RADIUS * torch.sin(ang) - RADIUS).reshape(T, 1, 1)
    wp[..., 2] = float(init_xyzs[0, 2])
    _, _, metrics = sim.cmd_rollout(wp, "waypoint", record=False, metrics=True)
    bad = sim.nonfinite().cpu().numpy()
    rms = np.sqrt(metrics[:, 0, 0].cpu().numpy() / max(T, 1))
    rms = np.where(bad | ~np.isfinite(rms), np.inf, rms)      # a diverged candidate never ranks first
    best = int(np.argmin(rms))
    in_force = sim.pid_gains()
    sim.close()
    res = {"envs": E, "steps": T, "spread": float(spread), "seed": int(seed),
           "nominal_rms": float(rms[0]), "best_rms": float(rms[best]), "best_index": best,
           "best_gains": {name: in_force[name][best, 0].tolist() for name in PID_GAIN_KEYWORDS},
           "nonfinite": int(bad.sum())}
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description="Fly E candidate DSLPIDControl gain sets on one trajectory in one launch")
    ap.add_argument("--envs", default=256, type=int)
    ap.add_argument("--steps", default=192, type=int)
    ap.add_argument("--spread", default=0.5, type=float)
    ap.add_argument("--seed", default=0, type=int)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    run(a.envs, a.steps, a.spread, a.seed, a.out)
