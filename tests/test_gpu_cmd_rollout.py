"""GPU parity of the closed-loop rollout (gpd_cmd_rollout: T command steps in one launch) against
the CPU reference tests/cmd_ref.py and against the stepwise path (T gpd_cmd_step calls), at
tests/test_gpu_cmd_step.py's cases, horizons and gates (state_rel_err: f64 max <= 1e-10, f32
median <= 1e-5 / max <= 1e-3).  Launches of one flight, and calls that continue one another, are
compared bit for bit: the same kernel, the state round-tripping memory losslessly.  Rollout vs
stepwise on envs of up to 64 drones is gated like the reference (different instantiations), the
observed figure printed; on wider envs the rollout issues the stepwise kernels: bit for bit.
"""
import functools

import numpy as np
import pytest
import torch

from tests.cmd_ref import CmdRefAviary
from tests.test_gpu_cmd_step import (MAX_RPM, RPM_CASES, _check_ctrl, _check_state, _oracle20, _rpm_actions,
                                     _rpm_reference, _sim, _waypoints)
from tests.test_gpu_wide import _spiral

pytestmark = pytest.mark.gpu

XYZ3 = np.array([[0, 0, 0.5], [1, 0, 0.6], [0, 1, 0.7]])


def _np(t):
    return t.cpu().numpy()


def _track_ref(traj, wp):
    """metrics from the recorded rows: the sum over the steps (in step order) of the squared
    distance to the step's target, and the largest distance; every product and sum rounded."""
    d = traj[..., 0:3] - wp[..., 0:3]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    s = np.zeros(d2.shape[1:])
    for t in range(d2.shape[0]):
        s = s + d2[t]
    return s, np.sqrt(d2).max(axis=0)


# ------------------------------------------------------------------ 1. RPM mode
@pytest.mark.parametrize("case,prec", [("e70_d1", "f64"), ("e22_d3_pyb_all", "f64"), ("e70_d1", "f32")])
def test_rpm_rollout_vs_oracle_and_stepwise(case, prec):
    from gym_pybullet_drones_routing_amd.enums import ActionType, Physics
    c = RPM_CASES[case]
    E, D, T = c["E"], c["D"], c["T"]
    f32 = prec == "f32"
    acts = _rpm_actions(T, E * D, f32)
    ref = _rpm_reference(case, f32)
    kw = dict(c["sim"])
    kw["physics"] = Physics(kw.get("physics", "dyn"))
    sims = [_sim(n_envs=E, drones_per_env=D, act=ActionType.RPM, ctrl_freq=c["ctrl_freq"], precision=prec, **kw)
            for _ in range(2)]
    sim, step = sims
    nsub = 240 // c["ctrl_freq"]
    a = torch.from_numpy(acts.reshape(T, E, D, 4)).to(sim.real_dtype).cuda()
    traj, obs, met = sim.cmd_rollout(a, "rpm")
    assert met is None and traj.shape == (T, E, D, 20) and traj.dtype == sim.real_dtype
    assert obs is sim._obs20 and obs.shape == (E, D, 20)
    got = _np(traj).reshape(T, E * D, 20)
    clip = np.clip(acts, 0, MAX_RPM)
    if f32:
        clip = clip.astype(np.float32)
    np.testing.assert_array_equal(got[..., 16:20], clip)                      # np.clip(a, 0, MAX_RPM) exactly
    np.testing.assert_array_equal(_np(sim.step_counters()), np.full(E, T * nsub))
    assert torch.equal(obs, traj[-1]) and torch.equal(obs.reshape(-1, 20), sim.state20())
    _check_state(f"rollout rpm {case} {prec} vs oracle", got, ref, prec)
    sw = np.array([_np(step.cmd_step(a[t], "rpm")).reshape(E * D, 20) for t in range(T)])
    print(f"[cmd_rollout] rpm {case} {prec}: rollout vs stepwise max abs difference {np.abs(got - sw).max():.3e}")
    _check_state(f"rollout rpm {case} {prec} vs stepwise", got, sw, prec)
    np.testing.assert_array_equal(_np(sim.step_counters()), _np(step.step_counters()))
    for s in sims:
        s.close()


# ------------------------------------------------------------------ 2. / 4. waypoint mode, chunking
WP_E, WP_D, WP_T = 3, 3, 16


@functools.lru_cache(maxsize=None)
def _wp_rows():
    w = np.array([[_waypoints(XYZ3, t, e) for e in range(WP_E)] for t in range(WP_T)])
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _wp_reference():
    """(state20 [N, 20], ctrl_state [N, 9]) of the reference after the 16 waypoint steps."""
    w = _wp_rows()
    envs = [CmdRefAviary(num_drones=WP_D, drones_per_env=WP_D, integrator="bullet", ctrl_freq=48, initial_xyzs=XYZ3)
            for _ in range(WP_E)]
    for t in range(WP_T):
        for e, env in enumerate(envs):
            env.cmd_step("waypoint", w[t, e])
    return _oracle20(envs), np.concatenate([e.ctrl_state() for e in envs])


def _wp_sim(E=WP_E, D=WP_D, xyz=XYZ3, aero=()):
    from gym_pybullet_drones_routing_amd.enums import ActionType, Physics
    return _sim(n_envs=E, drones_per_env=D, act=ActionType.VEL, physics=Physics.PYB, aero=aero, ctrl_freq=48,
                initial_xyzs=xyz)


@functools.lru_cache(maxsize=None)
def _wp_run(how):
    """The waypoint flight flown as one call ("one"), as calls of 5 + 11 steps ("split") or as one
    call of launches of at most 3 steps ("chunk3"): everything it leaves, on the host."""
    w = torch.tensor(_wp_rows(), device="cuda")
    sim = _wp_sim()
    if how == "split":
        t1, _, _ = sim.cmd_rollout(w[:5], "waypoint", metrics=True)
        t2, obs, met = sim.cmd_rollout(w[5:], "waypoint", metrics=True)
        traj = torch.cat([t1, t2])
    else:
        traj, obs, met = sim.cmd_rollout(w, "waypoint", metrics=True, max_steps_per_launch=3 if how == "chunk3" else 0)
    out = dict(traj=_np(traj), obs=_np(obs), metrics=_np(met), raw=_np(sim.raw_state()), ctrl=_np(sim.ctrl_state()),
               counters=_np(sim.step_counters()), state20=_np(sim.state20()))
    sim.close()
    for v in out.values():
        v.setflags(write=False)
    return out


def test_waypoint_rollout_vs_reference():
    r = _wp_run("one")
    ref20, ref_cs = _wp_reference()
    assert np.abs(ref20[:, 9]).min() > 0.01           # the drones did turn toward their target yaw
    _check_state("rollout waypoint pyb", r["obs"].reshape(-1, 20), ref20)
    np.testing.assert_array_equal(r["obs"].reshape(-1, 20), r["state20"])
    np.testing.assert_array_equal(r["obs"], r["traj"][-1])
    np.testing.assert_allclose(r["ctrl"], ref_cs, rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(r["counters"], np.full(WP_E, WP_T * 5))
    s, m = _track_ref(r["traj"], _wp_rows())
    assert r["metrics"].shape == (WP_E, WP_D, 2) and s.min() > 0
    np.testing.assert_allclose(r["metrics"][..., 0], s, rtol=1e-12)
    np.testing.assert_allclose(r["metrics"][..., 1], m, rtol=1e-12)


@pytest.mark.parametrize("how", ["split", "chunk3"])
def test_chunking_is_exact(how):
    one, other = _wp_run("one"), _wp_run(how)
    for key in ("raw", "ctrl", "traj", "counters", "obs"):
        np.testing.assert_array_equal(other[key], one[key], err_msg=key)
    if how == "chunk3":     # one flight: the figures carry over from launch to launch
        np.testing.assert_array_equal(other["metrics"], one["metrics"])


# ------------------------------------------------------------------ 3. VEL mode
def test_vel_rollout_vs_reference():
    """test_vel_mode_parity_pyb's flight (Physics.PYB 240 / 240, the zero-direction row) in one call."""
    from gym_pybullet_drones_routing_amd.enums import ActionType, Physics
    E, D, T = 5, 2, 16
    xyz = [[0, 0, 0.5], [1, 0, 0.5]]
    rng = np.random.default_rng(22)
    acts = rng.uniform(-1, 1, (T, E, D, 4)).astype(np.float32)
    acts[:, 0, 0, 0:3] = 0.0                      # zero direction -> zero target velocity
    envs = [CmdRefAviary(num_drones=D, drones_per_env=D, integrator="bullet", ctrl_freq=240, initial_xyzs=xyz)
            for _ in range(E)]
    for t in range(T):
        for e, env in enumerate(envs):
            env.cmd_step("vel", acts[t, e])
    sim = _sim(n_envs=E, drones_per_env=D, act=ActionType.VEL, physics=Physics.PYB, ctrl_freq=240, initial_xyzs=xyz)
    traj, obs, met = sim.cmd_rollout(torch.from_numpy(acts).cuda(), "vel", record=False)
    assert traj is None and met is None
    _check_state("rollout vel pyb", _np(obs).reshape(-1, 20), _oracle20(envs))
    np.testing.assert_array_equal(_np(obs).reshape(-1, 20), _np(sim.state20()))
    _check_ctrl(sim, envs)
    np.testing.assert_array_equal(_np(sim.step_counters()), np.full(E, T))
    sim.close()


# ------------------------------------------------------------------ 5. record_every
def test_record_every_and_record_false():
    w = torch.tensor(_wp_rows()[:8], device="cuda")
    runs = {}
    for name, kw in (("all", {}), ("third", dict(record_every=3)), ("none", dict(record=False))):
        sim = _wp_sim()
        traj, obs, _ = sim.cmd_rollout(w, "waypoint", **kw)
        runs[name] = (None if traj is None else _np(traj), _np(obs), _np(sim.raw_state()), _np(sim.ctrl_state()))
        sim.close()
    full = runs["all"][0]
    assert full.shape[0] == 8 and runs["third"][0].shape == (2, WP_E, WP_D, 20) and runs["none"][0] is None
    np.testing.assert_array_equal(runs["third"][0], full[[2, 5]])
    for name in ("third", "none"):
        for k in (1, 2, 3):
            np.testing.assert_array_equal(runs[name][k], runs["all"][k], err_msg=f"{name} {k}")


# ------------------------------------------------------------------ 6. envs of more than 64 drones
def test_wide_fallback_is_the_stepwise_kernels():
    E, D, T = 1, 65, 4
    xyz = _spiral(D)
    w = np.array([[_waypoints(xyz, t, e) for e in range(E)] for t in range(T)])
    wt = torch.from_numpy(w).cuda()
    sim, step = (_wp_sim(E, D, xyz, ("no_drone_contact",)) for _ in range(2))
    traj, obs, met = sim.cmd_rollout(wt, "waypoint", metrics=True)
    sw = torch.stack([step.cmd_step(wt[t], "waypoint").clone() for t in range(T)])
    assert torch.equal(traj, sw) and torch.equal(obs, sw[-1])
    assert torch.equal(sim.raw_state(), step.raw_state()) and torch.equal(sim.ctrl_state(), step.ctrl_state())
    assert torch.equal(sim.step_counters(), step.step_counters()) and int(sim.step_counters()[0]) == T * 5
    s, m = _track_ref(_np(traj), w)
    np.testing.assert_allclose(_np(met)[..., 0], s, rtol=1e-12)
    np.testing.assert_allclose(_np(met)[..., 1], m, rtol=1e-12)
    # a flight whose last step is not recorded: obs20 comes from the last step's own launch
    traj2, obs2, _ = sim.cmd_rollout(wt[:3], "waypoint", record_every=2)
    sw2 = [step.cmd_step(wt[t], "waypoint").clone() for t in range(3)]
    assert traj2.shape[0] == 1 and torch.equal(traj2[0], sw2[1]) and torch.equal(obs2, sw2[2])
    sim.close()
    step.close()


# ------------------------------------------------------------------ 7. graph
def test_graph_replay_matches_eager():
    from gym_pybullet_drones_routing_amd.sim import graph_capture
    E, T = 70, 6
    a = torch.from_numpy(_rpm_actions(T, E).reshape(T, E, 1, 4)).cuda()
    eager = _sim(n_envs=E, task="hover")
    cap = _sim(n_envs=E, task="hover")
    cap._cmd_rows()     # allocated outside the capture
    eager.cmd_rollout(a, "rpm")
    g = torch.cuda.CUDAGraph()
    with graph_capture(g, cap.device):
        traj_g, obs_g, _ = cap.cmd_rollout(a, "rpm")
    assert int(cap.step_counters()[0]) == 0        # capture records only
    traj_e, obs_e, _ = eager.cmd_rollout(a, "rpm")
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(traj_g, traj_e) and torch.equal(obs_g, obs_e)
    assert torch.equal(cap.raw_state(), eager.raw_state())
    assert torch.equal(cap.step_counters(), eager.step_counters())
    assert int(cap.step_counters()[0]) == 2 * T * cap.pyb_steps_per_ctrl
    del g
    eager.close()
    cap.close()


# ------------------------------------------------------------------ 8. refusals
def test_refusals_run_nothing():
    from gym_pybullet_drones_routing_amd import _lib
    from gym_pybullet_drones_routing_amd.enums import ActionType
    from gym_pybullet_drones_routing_amd.sim import _ptr
    het = _sim(n_envs=2, env_params={})
    with pytest.raises(NotImplementedError, match="heterogeneous"):
        het.cmd_rollout(torch.zeros((3, 2, 1, 4), dtype=torch.float64, device="cuda"), "rpm")
    a = torch.zeros((3, 2, 1, 4), dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.GpdError, match="het sim") as exc:      # the library's own refusal
        het._call("gpd_cmd_rollout", _lib.GPD_CMD_RPM, _ptr(a), 3, 1, None, None, None, 0, None)
    assert exc.value.code == _lib.GPD_EUNSUPPORTED
    np.testing.assert_array_equal(_np(het.step_counters()), [0, 0])
    het.close()

    sim = _sim(n_envs=2, act=ActionType.RPM)
    m = torch.zeros((2, 1, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="metrics"):
        sim.cmd_rollout(a, "rpm", metrics=True)
    with pytest.raises(_lib.GpdError, match="metrics") as exc:
        sim._call("gpd_cmd_rollout", _lib.GPD_CMD_RPM, _ptr(a), 3, 1, None, None, _ptr(m), 0, None)
    assert exc.value.code == _lib.GPD_EINVAL
    with pytest.raises(_lib.GpdError, match="no controller") as exc:
        sim.cmd_rollout(torch.zeros((3, 2, 1, 7), dtype=torch.float64, device="cuda"), "waypoint")
    assert exc.value.code == _lib.GPD_EINVAL
    for bad, mode in ((torch.zeros((3, 2, 1, 7), dtype=torch.float64, device="cuda"), "rpm"), (a, "thrust")):
        with pytest.raises(ValueError):
            sim.cmd_rollout(bad, mode)
    with pytest.raises(ValueError, match="record_every"):
        sim.cmd_rollout(a, "rpm", record_every=0)
    np.testing.assert_array_equal(_np(sim.step_counters()), [0, 0])      # nothing ran

    # n_steps = 0: a successful no-op
    raw = sim.raw_state()
    sim._cmd_rows().fill_(7.0)
    traj, obs, met = sim.cmd_rollout(torch.zeros((0, 2, 1, 4), dtype=torch.float64, device="cuda"), "rpm")
    assert traj.shape == (0, 2, 1, 20) and met is None
    assert bool((obs == 7.0).all()) and torch.equal(sim.raw_state(), raw)
    np.testing.assert_array_equal(_np(sim.step_counters()), [0, 0])
    sim.close()


# ------------------------------------------------------------------ 9. the example
def test_pid_example_fused_matches_stepwise(tmp_path):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "pid.py")
    spec = importlib.util.spec_from_file_location("example_pid_fused", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    kw = dict(num_envs=4, num_drones=2, duration_sec=0.5, save=False)
    err_f, bad_f = mod.run(fused=True, output_folder=str(tmp_path / "fused"), **kw)
    err_s, bad_s = mod.run(fused=False, output_folder=str(tmp_path / "stepwise"), **kw)
    assert bad_f == bad_s and not bad_f
    assert abs(err_f - err_s) <= 1e-9, (err_f, err_s)
