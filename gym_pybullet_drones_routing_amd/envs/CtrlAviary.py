"""CtrlAviary on the HIP path (reference: ``envs/CtrlAviary.py``).

Raw motor RPMs in, the 20-float state vector of every drone out; reward, terminated and
truncated are the reference's dummies (-1, False, False).  One step is one launch of the command
step kernel (``BatchedAviarySim.cmd_step``).
"""
import numpy as np

from ..enums import ActionType, DroneModel, ObservationType, Physics
from .BaseRLAviary import BaseRLAviary
from .spaces import Box


def state20_space(num_drones, max_rpm):
    """CtrlAviary._observationSpace (:90-102): the bounds of the 20-float state vector."""
    lo = np.array([[-np.inf, -np.inf, 0., -1., -1., -1., -1., -np.pi, -np.pi, -np.pi,
                    -np.inf, -np.inf, -np.inf, -np.inf, -np.inf, -np.inf, 0., 0., 0., 0.]] * num_drones)
    hi = np.array([[np.inf, np.inf, np.inf, 1., 1., 1., 1., np.pi, np.pi, np.pi,
                    np.inf, np.inf, np.inf, np.inf, np.inf, np.inf, max_rpm, max_rpm, max_rpm, max_rpm]] * num_drones)
    return Box(low=lo, high=hi, dtype=np.float32)


class CommandAviary(BaseRLAviary):
    """What CtrlAviary and VelocityAviary share: the reference's BaseAviary constructor keywords,
    the state-vector observation, the dummy reward / flags, and the adjacency matrix from the
    device.  ``act`` is the action type the sim is created with (a PID type owns a controller)."""

    TASK = "none"
    CMD_MODE = "rpm"

    def __init__(self, drone_model=DroneModel.CF2X, num_drones=1, neighbourhood_radius=np.inf,
                 initial_xyzs=None, initial_rpys=None, physics=Physics.PYB, pyb_freq=240, ctrl_freq=240,
                 gui=False, record=False, obstacles=False, user_debug_gui=True, output_folder='results',
                 act=ActionType.RPM, precision="f64", device=None, urdf_path=None):
        if obstacles:
            raise NotImplementedError("obstacles need PyBullet's collision world (out of scope: headless batched sim)")
        del user_debug_gui, output_folder   # accepted and ignored: there is no GUI and nothing is recorded
        super().__init__(drone_model=drone_model, num_drones=num_drones, neighbourhood_radius=neighbourhood_radius,
                         initial_xyzs=initial_xyzs, initial_rpys=initial_rpys, physics=physics, pyb_freq=pyb_freq,
                         ctrl_freq=ctrl_freq, gui=gui, record=record, obs=ObservationType.KIN, act=act,
                         precision=precision, device=device, urdf_path=urdf_path)
        # the reference's BaseAviary has neither attribute; the sim's action type only says whether it
        # owns a controller state
        del self.ACT_TYPE, self.OBS_TYPE
        self.SPEED_LIMIT = 0.03 * self.MAX_SPEED_KMH * (1000 / 3600)
        self.observation_space = state20_space(self.NUM_DRONES, self.MAX_RPM)
        self.action_space = self._actionSpace()

    def _actionSpace(self):
        raise NotImplementedError

    # ------------------------------------------------------------------ Gymnasium surface
    def _obs(self, rows):
        return rows.reshape(self.NUM_DRONES, 20).cpu().numpy().astype(np.float64)

    def reset(self, seed=None, options=None):
        """BaseAviary.reset (:220-255): the initial state vectors.  The seed is ignored (:243)."""
        self.sim.reset()
        self.step_counter = 0
        return self._computeObs(), self._computeInfo()

    def _command(self, actions, mode):
        obs = self._obs(self.sim.cmd_step(actions, mode))
        self.step_counter += self.PYB_STEPS_PER_CTRL
        return obs, self._computeReward(), False, False, self._computeInfo()

    def step(self, action):
        """BaseAviary.step (:259-383): one launch for the command and the PYB_STEPS_PER_CTRL substeps."""
        return self._command(self._action_array(action), self.CMD_MODE)

    def _computeObs(self):
        return self._obs(self.sim.state20())

    def _computeReward(self):
        return -1

    def _getAdjacencyMatrix(self):
        """BaseAviary._getAdjacencyMatrix (:658-675), computed on the device."""
        return self.sim.adjacency(self.NEIGHBOURHOOD_RADIUS)[0].cpu().numpy().astype(np.float64)


class CtrlAviary(CommandAviary):
    """Multi-drone environment class for control applications."""

    CMD_MODE = "rpm"

    def __init__(self, drone_model=DroneModel.CF2X, num_drones=1, neighbourhood_radius=np.inf,
                 initial_xyzs=None, initial_rpys=None, physics=Physics.PYB, pyb_freq=240, ctrl_freq=240,
                 gui=False, record=False, obstacles=False, user_debug_gui=True, output_folder='results',
                 precision="f64", device=None, urdf_path=None):
        # a PID action type gives the sim a DSLPIDControl state, so that step_to() is available;
        # the racer has no controller (BaseRLAviary.py:75-78)
        has_ctrl = DroneModel(drone_model) in (DroneModel.CF2X, DroneModel.CF2P)
        super().__init__(drone_model, num_drones, neighbourhood_radius, initial_xyzs, initial_rpys, physics,
                         pyb_freq, ctrl_freq, gui, record, obstacles, user_debug_gui, output_folder,
                         act=ActionType.VEL if has_ctrl else ActionType.RPM, precision=precision, device=device,
                         urdf_path=urdf_path)

    def _actionSpace(self):
        """CtrlAviary._actionSpace (:74-86): commanded RPMs in [0, MAX_RPM]."""
        return Box(low=np.zeros((self.NUM_DRONES, 4)), high=np.full((self.NUM_DRONES, 4), self.MAX_RPM),
                   dtype=np.float32)

    def _action_array(self, action):
        return np.asarray(action, dtype=np.float64).reshape(1, self.NUM_DRONES, 4)

    def step_to(self, target_pos, target_rpy=None, target_vel=None):
        """ADDITION (not in the reference): one step under the on-device DSLPIDControl - what
        the loop of the reference's examples/pid.py does with ``computeControl(state, target_pos,
        target_rpy)`` followed by ``env.step(rpm)``.  ``target_pos`` (NUM_DRONES, 3); of
        ``target_rpy`` (NUM_DRONES, 3) the controller reads the yaw only; ``target_vel``
        (NUM_DRONES, 3) defaults to zero.  Returns what ``step`` returns."""
        D = self.NUM_DRONES
        w = np.zeros((1, D, 7))
        w[0, :, 0:3] = np.asarray(target_pos, dtype=np.float64).reshape(D, 3)
        if target_rpy is not None:
            w[0, :, 3] = np.asarray(target_rpy, dtype=np.float64).reshape(D, 3)[:, 2]
        if target_vel is not None:
            w[0, :, 4:7] = np.asarray(target_vel, dtype=np.float64).reshape(D, 3)
        return self._command(w, "waypoint")
