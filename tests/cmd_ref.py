"""CPU reference of the command step (gpd_cmd_step): CtrlAviary / VelocityAviary / the
examples/pid.py loop on the oracle's RefAviary.  Test infrastructure only.

``RefAviary.step`` casts its action to float32 (the RL surface), so raw RPMs cannot go through
it; ``cmd_step`` repeats its loop body (oracle/ref_aviary.py step()) with one of three command
stages:
  * ``"rpm"``       CtrlAviary._preprocessAction (envs/CtrlAviary.py:140): np.clip(a, 0, MAX_RPM)
  * ``"vel"``       VelocityAviary._preprocessAction (envs/VelocityAviary.py:148-168) =
                    ``pid_action_rpm("vel", ...)``, the RL VEL branch
  * ``"waypoint"``  ``computeControl(state, target_pos, target_rpy=[0, 0, yaw], target_vel)``
                    (examples/pid.py); the action row is target_pos(3), yaw, target_vel(3)
"""
import numpy as np

from oracle.ref_aviary import RefAviary
from oracle.ref_pid import pid_action_rpm


def adjacency_np(pos, radius):
    """BaseAviary._getAdjacencyMatrix (:658-675) restated without the double loop: pos [D, 3]."""
    d = pos[:, None, :] - pos[None, :, :]
    dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    adj = (dist < radius).astype(np.float64)
    np.fill_diagonal(adj, 1.0)
    return adj


def adjacency_loop(pos, radius):
    """BaseAviary._getAdjacencyMatrix (:658-675), the reference's double loop."""
    n = pos.shape[0]
    adjacency_mat = np.identity(n)
    for i in range(n - 1):
        for j in range(n - i - 1):
            if np.linalg.norm(pos[i, :] - pos[j + i + 1, :]) < radius:
                adjacency_mat[i, j + i + 1] = adjacency_mat[j + i + 1, i] = 1
    return adjacency_mat


class CmdRefAviary(RefAviary):
    """RefAviary (without a task unless one is named: ``step`` and ``cmd_step`` then interleave on
    one env), stepped by commands.  ``act="vel"`` (the default) owns the
    DSLPIDControl objects the "vel" and "waypoint" modes need; the racer has none: act="rpm"."""

    def __init__(self, act="vel", task="none", **kw):
        super().__init__(act=act, task=task, **kw)
        self.MAX_RPM = self.P["max_rpm"]

    def _command_rpm(self, mode, action):
        n = self.NUM_DRONES
        if mode == "rpm":
            a = np.asarray(action, dtype=np.float64).reshape(n, 4)
            return np.array([np.clip(a[i, :], 0, self.MAX_RPM) for i in range(n)])
        rpm = np.zeros((n, 4))
        if mode == "vel":
            a = np.asarray(action, dtype=np.float32).reshape(n, 4)
            for k in range(n):
                rpm[k, :] = pid_action_rpm("vel", self.ctrl[k], self._getDroneStateVector(k), a[k, :],
                                           self.CTRL_TIMESTEP, self.SPEED_LIMIT)
            return rpm
        if mode == "waypoint":
            w = np.asarray(action, dtype=np.float64).reshape(n, 7)
            for k in range(n):
                state = self._getDroneStateVector(k)
                rpm[k, :], _, _ = self.ctrl[k].computeControl(
                    control_timestep=self.CTRL_TIMESTEP, cur_pos=state[0:3], cur_quat=state[3:7],
                    cur_vel=state[10:13], cur_ang_vel=state[13:16], target_pos=w[k, 0:3],
                    target_rpy=np.array([0, 0, w[k, 3]]), target_vel=w[k, 4:7])
            return rpm
        raise ValueError(mode)

    def cmd_step(self, mode, action):
        clipped_action = np.reshape(self._command_rpm(mode, action), (self.NUM_DRONES, 4))
        plain_pyb = self.INTEGRATOR == "bullet" and not self.AERO
        for _ in range(self.PYB_STEPS_PER_CTRL):
            if self.PYB_STEPS_PER_CTRL > 1 and not plain_pyb:
                self._updateAndStoreKinematicInformation()
            self._substep_all(clipped_action)
            self.last_clipped_action = clipped_action
        self._updateAndStoreKinematicInformation()
        self.step_counter = self.step_counter + (1 * self.PYB_STEPS_PER_CTRL)
        return self.state20()
