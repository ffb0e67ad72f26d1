"""The CPU reference of the command step (tests/cmd_ref.py) against the oracle it is built on."""
import numpy as np

from oracle.ref_aviary import RefAviary
from tests.cmd_ref import CmdRefAviary, adjacency_loop, adjacency_np


def test_vel_mode_is_the_rl_vel_path_bit_for_bit():
    rng = np.random.default_rng(3)
    acts = rng.uniform(-1, 1, (16, 2, 4)).astype(np.float32)
    acts[3, 0, 0:3] = 0.0          # zero direction -> zero target velocity
    xyz = [[0, 0, 0.5], [1, 0, 0.5]]
    for integrator in ("dyn", "bullet"):
        rl = RefAviary(num_drones=2, act="vel", task="none", integrator=integrator, ctrl_freq=240, initial_xyzs=xyz)
        cmd = CmdRefAviary(num_drones=2, integrator=integrator, ctrl_freq=240, initial_xyzs=xyz)
        for t in range(16):
            rl.step(acts[t])
            s = cmd.cmd_step("vel", acts[t])
            np.testing.assert_array_equal(s, rl.state20())
            np.testing.assert_array_equal(cmd.ctrl_state(), rl.ctrl_state())
        assert cmd.step_counter == rl.step_counter == 16


def test_rpm_mode_leaves_the_clipped_action():
    env = CmdRefAviary(num_drones=5, ctrl_freq=48)
    hover, mx = env.HOVER_RPM, env.MAX_RPM
    a = np.array([[hover, hover * 1.01, hover * 0.99, hover],
                  [-5.0, hover, hover, -1e9],
                  [mx + 1.0, mx * 3, hover, hover],
                  [0.0, mx, 0.0, mx],
                  [np.nextafter(mx, np.inf), np.nextafter(mx, 0), -0.0, 1e-300]])
    s = env.cmd_step("rpm", a)
    np.testing.assert_array_equal(s[:, 16:20], np.clip(a, 0, mx))
    assert s[:, 16:20].min() >= 0 and s[:, 16:20].max() == mx
    assert env.step_counter == 5
    # the second step's drag would read these: they are the stored last_clipped_action
    np.testing.assert_array_equal(env.last_clipped_action, np.clip(a, 0, mx))


def test_waypoint_mode_flies_toward_its_targets():
    env = CmdRefAviary(num_drones=3, integrator="bullet", aero=("gnd", "drag", "dw"), ctrl_freq=48,
                       drones_per_env=3, initial_xyzs=[[0, 0, 0.5], [0.5, 0, 0.7], [0, 0.5, 0.9]])
    start = env.state20()[:, 0:3].copy()
    tgt = start + np.array([0.0, 0.0, 0.3])
    w = np.hstack([tgt, np.full((3, 1), 0.2), np.zeros((3, 3))])
    for _ in range(16):
        s = env.cmd_step("waypoint", w)
    assert np.isfinite(s).all()
    assert (np.linalg.norm(s[:, 0:3] - tgt, axis=1) < np.linalg.norm(start - tgt, axis=1)).all()


def test_adjacency_restatement_equals_the_reference_loop():
    rng = np.random.default_rng(5)
    for D in (1, 2, 7):
        pos = rng.uniform(-1, 1, (D, 3))
        for radius in (0.0, 0.4, 1.0, 2.5, np.inf):
            np.testing.assert_array_equal(adjacency_np(pos, radius), adjacency_loop(pos, radius))
