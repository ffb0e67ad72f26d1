"""VelocityAviary on the HIP path (reference: ``envs/VelocityAviary.py``).

Velocity commands (unit direction, fraction of the speed limit) through the on-device
DSLPIDControl, the 20-float state vector of every drone out; one step is one launch of the
command step kernel (``BatchedAviarySim.cmd_step(..., "vel")``).
"""
import numpy as np

from ..enums import ActionType, DroneModel, Physics
from .CtrlAviary import CommandAviary
from .spaces import Box


class VelocityAviary(CommandAviary):
    """Multi-drone environment class for high-level planning."""

    CMD_MODE = "vel"

    def __init__(self, drone_model=DroneModel.CF2X, num_drones=1, neighbourhood_radius=np.inf,
                 initial_xyzs=None, initial_rpys=None, physics=Physics.PYB, pyb_freq=240, ctrl_freq=240,
                 gui=False, record=False, obstacles=False, user_debug_gui=True, output_folder='results',
                 precision="f64", device=None, urdf_path=None):
        super().__init__(drone_model, num_drones, neighbourhood_radius, initial_xyzs, initial_rpys, physics,
                         pyb_freq, ctrl_freq, gui, record, obstacles, user_debug_gui, output_folder,
                         act=ActionType.VEL, precision=precision, device=device, urdf_path=urdf_path)

    def _actionSpace(self):
        """VelocityAviary._actionSpace (:82-94): X, Y, Z in [-1, 1], fraction of the speed limit in [0, 1]."""
        lo = np.array([[-1., -1., -1., 0.]] * self.NUM_DRONES)
        hi = np.array([[1., 1., 1., 1.]] * self.NUM_DRONES)
        return Box(low=lo, high=hi, dtype=np.float32)

    def _action_array(self, action):
        return np.asarray(action, dtype=np.float32).reshape(1, self.NUM_DRONES, 4)
