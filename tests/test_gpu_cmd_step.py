"""GPU parity of the command step (gpd_cmd_step: CtrlAviary / VelocityAviary / the examples/pid.py
loop in one launch), of gpd_adjacency, and of the two Gym-surface classes, against the CPU
reference tests/cmd_ref.py.  Error measure and gates of tests/test_gpu_parity.py: state_rel_err,
f64 max <= 1e-10, f32 median <= 1e-5 / max <= 1e-3.
"""
import functools

import numpy as np
import pytest
import torch

from oracle.params import derived
from tests.cmd_ref import CmdRefAviary, adjacency_loop
from tests.oracle_runs import oracle_raw, state_rel_err
from tests.test_gpu_parity import HOVER, TOL, TOL_MEDIAN
from tests.test_gpu_wide import _spiral

pytestmark = pytest.mark.gpu

MAX_RPM = derived("cf2x")["max_rpm"]
STAGGER3 = [[0, 0, 0.5], [0.1, 0, 0.8], [0, 0.1, 1.1]]   # drones above one another: downwash, no contact


def _sim(**kw):
    from gym_pybullet_drones_routing_amd.sim import BatchedAviarySim
    kw.setdefault("task", "none")
    kw.setdefault("precision", "f64")
    return BatchedAviarySim(device="cuda:0", **kw)


def _oracle20(envs):
    return np.concatenate([e.state20() for e in envs])


def _check_state(name, got, ref, prec="f64"):
    err = state_rel_err(got, ref)
    print(f"\n[cmd_step] {name}: max {err.max():.3e} median {np.median(err):.3e}")
    assert err.max() <= TOL[prec], err.max()
    assert np.median(err) <= TOL_MEDIAN[prec], np.median(err)


# ------------------------------------------------------------------ RPM mode
def _rpm_actions(T, n, f32=False):
    """Random RPMs around hover; rows below 0, above MAX_RPM, exactly 0 and exactly MAX_RPM."""
    rng = np.random.default_rng(21)
    a = HOVER * (1 + 0.05 * rng.uniform(-1, 1, (T, n, 4)))
    a[1, 0] = [-100.0, HOVER, HOVER, MAX_RPM + 500.0]
    a[1, 1] = [0.0, MAX_RPM, 0.0, MAX_RPM]
    a[2, 2] = [-1e6, 1e9, HOVER, np.nextafter(MAX_RPM, np.inf)]
    return a.astype(np.float32).astype(np.float64) if f32 else a


RPM_CASES = {
    # five substeps; 16-drone blocks, the last one ragged
    "e70_d1": dict(E=70, D=1, T=12, ctrl_freq=48, sim={}, ref={}),
    # drag (substep 1 sees the previous step's RPMs), ground effect, downwash through LDS; a block of
    # 63 lanes and one of 3
    "e22_d3_pyb_all": dict(E=22, D=3, T=6, ctrl_freq=30,
                           sim=dict(physics="pyb_gnd_drag_dw", initial_xyzs=STAGGER3, tuning={"drones_per_block": 64}),
                           ref=dict(integrator="bullet", aero=("gnd", "drag", "dw"), initial_xyzs=STAGGER3)),
    # the wide kernel, one lane in the second wave
    "e2_d65_dw": dict(E=2, D=65, T=6, ctrl_freq=240,
                      sim=dict(aero=("dw",), initial_xyzs=_spiral(65)), ref=dict(aero=("dw",), initial_xyzs=_spiral(65))),
}


@functools.lru_cache(maxsize=None)
def _rpm_reference(case, f32=False):
    """[T, N, 20] oracle state vectors of an RPM case (computed once per case)."""
    c = RPM_CASES[case]
    E, D, T = c["E"], c["D"], c["T"]
    acts = _rpm_actions(T, E * D, f32)
    if D == 1:   # independent drones: one instance holds them all, each at a single-drone env's start
        p = derived("cf2x")
        z0 = p["collision_h"] / 2 - p["collision_z_offset"] + .1
        envs = [CmdRefAviary(act="rpm", num_drones=E, ctrl_freq=c["ctrl_freq"], initial_xyzs=[[0, 0, z0]] * E,
                             **c["ref"])]
    else:
        envs = [CmdRefAviary(act="rpm", num_drones=D, drones_per_env=D, ctrl_freq=c["ctrl_freq"], **c["ref"])
                for _ in range(E)]
    per = E * D // len(envs)
    out = []
    for t in range(T):
        out.append(np.concatenate([env.cmd_step("rpm", acts[t, k * per:(k + 1) * per]) for k, env in enumerate(envs)]))
    out = np.array(out)
    out.setflags(write=False)
    return out


def _run_rpm(case, prec):
    from gym_pybullet_drones_routing_amd.enums import ActionType, Physics
    c = RPM_CASES[case]
    E, D, T = c["E"], c["D"], c["T"]
    f32 = prec == "f32"
    acts = _rpm_actions(T, E * D, f32)
    ref = _rpm_reference(case, f32)
    kw = dict(c["sim"])
    kw["physics"] = Physics(kw.get("physics", "dyn"))
    sim = _sim(n_envs=E, drones_per_env=D, act=ActionType.RPM, ctrl_freq=c["ctrl_freq"], precision=prec, **kw)
    nsub = 240 // c["ctrl_freq"]
    got = []
    for t in range(T):
        obs = sim.cmd_step(torch.from_numpy(acts[t].reshape(E, D, 4)).to(sim.real_dtype).cuda(), "rpm")
        assert obs.shape == (E, D, 20) and obs.dtype == sim.real_dtype
        assert torch.equal(obs.reshape(-1, 20), sim.state20())      # the row store == the state20 readback
        got.append(obs.reshape(-1, 20).cpu().numpy())
    got = np.array(got)
    clip = np.clip(acts, 0, MAX_RPM)
    if f32:
        clip = clip.astype(np.float32)
    np.testing.assert_array_equal(got[..., 16:20], clip)                      # np.clip(a, 0, MAX_RPM) exactly
    np.testing.assert_array_equal(got[..., 16:20], ref[..., 16:20].astype(got.dtype))
    assert got[..., 16:20].min() == 0 and got[..., 16:20].max() == clip.max()
    np.testing.assert_array_equal(sim.step_counters().cpu().numpy(), np.full(E, T * nsub))
    _check_state(f"rpm {case} {prec}", got, ref, prec)
    sim.close()


@pytest.mark.parametrize("case", list(RPM_CASES))
def test_rpm_mode_parity_f64(case):
    _run_rpm(case, "f64")


def test_rpm_mode_parity_f32():
    _run_rpm("e70_d1", "f32")


# ------------------------------------------------------------------ controller modes
def _check_ctrl(sim, envs):
    cs_r = np.concatenate([e.ctrl_state() for e in envs])
    np.testing.assert_allclose(sim.ctrl_state().cpu().numpy(), cs_r, rtol=1e-9, atol=1e-9)


def test_vel_mode_parity_pyb():
    """VelocityAviary's defaults (Physics.PYB, 240 / 240), 16 steps: the horizon of this chaotic
    closed loop.  Two drones 1 m apart: the pair contact runs and finds nothing."""
    from gym_pybullet_drones_routing_amd.enums import ActionType, Physics
    E, D, T = 5, 2, 16
    xyz = [[0, 0, 0.5], [1, 0, 0.5]]
    rng = np.random.default_rng(22)
    acts = rng.uniform(-1, 1, (T, E, D, 4)).astype(np.float32)
    acts[:, 0, 0, 0:3] = 0.0                      # zero direction -> zero target velocity
    envs = [CmdRefAviary(num_drones=D, drones_per_env=D, integrator="bullet", ctrl_freq=240, initial_xyzs=xyz)
            for _ in range(E)]
    sim = _sim(n_envs=E, drones_per_env=D, act=ActionType.VEL, physics=Physics.PYB, ctrl_freq=240, initial_xyzs=xyz)
    for t in range(T):
        obs = sim.cmd_step(torch.from_numpy(acts[t]).cuda(), "vel")
        for e, env in enumerate(envs):
            env.cmd_step("vel", acts[t, e])
    _check_state("vel pyb", obs.reshape(-1, 20).cpu().numpy(), _oracle20(envs))
    np.testing.assert_array_equal(obs.reshape(-1, 20).cpu().numpy(), sim.state20().cpu().numpy())
    _check_ctrl(sim, envs)
    np.testing.assert_array_equal(sim.step_counters().cpu().numpy(), np.full(E, T))
    sim.close()


def _waypoints(start, t, e):
    """Moving targets near the start positions, non-zero target yaw and target velocity."""
    n = start.shape[0]
    ph = 0.2 * t + 0.5 * e + np.arange(n)
    w = np.zeros((n, 7))
    w[:, 0:3] = start + 0.15 * np.stack([np.cos(ph) - 1, np.sin(ph), 0.5 * np.sin(0.5 * ph)], 1)
    w[:, 3] = 0.3 + 0.02 * t + 0.1 * (np.arange(n) % 5)
    w[:, 4:7] = 0.1 * np.stack([-np.sin(ph), np.cos(ph), 0.25 * np.cos(0.5 * ph)], 1)
    return w


@pytest.mark.parametrize("E,D,T", [(3, 3, 16), (1, 65, 4)])
def test_waypoint_mode_parity_pyb(E, D, T):
    """computeControl(target_pos, target_rpy=(0, 0, yaw), target_vel) + step at 240 / 48 on
    Physics.PYB; D = 65 runs the wide kernel (PYB envs of more than 64 drones: no pair contact)."""
    from gym_pybullet_drones_routing_amd.enums import ActionType, Physics
    xyz = np.array([[0, 0, 0.5], [1, 0, 0.6], [0, 1, 0.7]]) if D == 3 else _spiral(D)
    aero = () if D <= 64 else ("no_drone_contact",)
    envs = [CmdRefAviary(num_drones=D, drones_per_env=D, integrator="bullet", aero=aero, ctrl_freq=48,
                         initial_xyzs=xyz) for _ in range(E)]
    sim = _sim(n_envs=E, drones_per_env=D, act=ActionType.VEL, physics=Physics.PYB, aero=aero, ctrl_freq=48,
               initial_xyzs=xyz)
    for t in range(T):
        w = np.array([_waypoints(xyz, t, e) for e in range(E)])
        obs = sim.cmd_step(torch.from_numpy(w).cuda(), "waypoint")
        for e, env in enumerate(envs):
            env.cmd_step("waypoint", w[e])
    ref = _oracle20(envs)
    assert np.abs(ref[:, 9]).min() > 0.01           # the drones did turn toward their target yaw
    _check_state(f"waypoint pyb D={D}", obs.reshape(-1, 20).cpu().numpy(), ref)
    _check_ctrl(sim, envs)
    np.testing.assert_array_equal(sim.step_counters().cpu().numpy(), np.full(E, T * 5))
    sim.close()


def test_contact_resynced_per_control_step():
    """A drone falling (zero RPM) onto another that lies on the plane 4 cm below: pair and plane
    contacts inside the command step.  Contact runs are chaotic, so the sim is set to the oracle's
    state before every control step (as resynced_substep_errors does per substep) and each step's
    own error is gated at test_gpu_drone_contact.py's f64 figure."""
    from gym_pybullet_drones_routing_amd.enums import ActionType, Physics
    hh = derived("cf2x")["collision_h"] / 2
    raw0 = np.zeros((2, 20))
    raw0[:, 0:3] = [[0, 0, hh], [0.01, 0.005, hh + 0.04]]
    raw0[:, 6] = 1.0
    env = CmdRefAviary(act="rpm", num_drones=2, drones_per_env=2, integrator="bullet", ctrl_freq=48)
    env.set_raw_state(raw0)
    sim = _sim(n_envs=1, drones_per_env=2, act=ActionType.RPM, physics=Physics.PYB, ctrl_freq=48)
    zero = np.zeros((2, 4))
    errs, vz = [], []
    for t in range(6):
        sim.set_raw_state(oracle_raw(env))
        obs = sim.cmd_step(torch.from_numpy(zero.reshape(1, 2, 4)).cuda(), "rpm")
        ref = env.cmd_step("rpm", zero)
        errs.append(state_rel_err(sim.raw_state().cpu().numpy()[:, :16], oracle_raw(env)[:, :16]))
        errs.append(state_rel_err(obs.reshape(-1, 20).cpu().numpy(), ref))
        vz.append(ref[1, 12])
    err = np.array(errs)
    print(f"\n[cmd_step] contact, resynced per control step: max {err.max():.3e}")
    # the upper drone was stopped by the lower one (free fall would reach -9.8 * 6 / 48 = -1.2 m/s)
    assert vz[-1] > -0.3 and min(vz) < -0.3, vz
    assert err.max() <= 1e-10, err.max()
    sim.close()


# ------------------------------------------------------------------ beside the RL step
def test_interleaves_with_the_rl_step():
    """step(a), cmd_step(rpm), step(a2) on an RPM / hover / DYN sim without drag - the sim whose
    RL step leaves last_clipped_action in the action ring and marks the state's columns stale
    (gpd_cmd_step reads no such value, stores its own and clears the mark in its kernel) -
    against the oracle doing the same sequence."""
    from gym_pybullet_drones_routing_amd.enums import ActionType
    E = 6
    rng = np.random.default_rng(23)
    a1 = rng.uniform(-1, 1, (E, 1, 4)).astype(np.float32)
    a2 = rng.uniform(-1, 1, (E, 1, 4)).astype(np.float32)
    r = HOVER * (1 + 0.05 * rng.uniform(-1, 1, (E, 1, 4)))
    r[0, 0] = [-3.0, MAX_RPM + 1, HOVER, 0.0]
    envs = [CmdRefAviary(act="rpm", task="hover") for _ in range(E)]
    # (no auto-reset: env 0's out-of-range RPMs tilt it past the hover task's 0.4 rad bound)
    sim = _sim(n_envs=E, task="hover", act=ActionType.RPM, autoreset=False)
    nsub = sim.pyb_steps_per_ctrl
    calls = (("step", a1), ("cmd", r), ("step", a2))
    for k, (kind, a) in enumerate(calls):
        if kind == "step":
            obs, _, _, _ = sim.step(torch.from_numpy(a).cuda())
            obs_r = np.stack([env.step(a[e])[0] for e, env in enumerate(envs)])
        else:
            sim.cmd_step(torch.from_numpy(a).cuda(), "rpm")
            for e, env in enumerate(envs):
                env.cmd_step("rpm", a[e])
        s, ref = sim.state20().cpu().numpy(), _oracle20(envs)
        _check_state(f"interleaved call {k} ({kind})", s, ref)
        np.testing.assert_array_equal(s[:, 16:20], ref[:, 16:20])
        np.testing.assert_array_equal(sim.step_counters().cpu().numpy(), np.full(E, (k + 1) * nsub))
    # the KIN rows of the last step: cmd_step left the action ring and its head alone
    np.testing.assert_array_equal(obs.cpu().numpy()[..., 12:], obs_r[..., 12:])
    np.testing.assert_array_equal(obs.cpu().numpy()[..., -8:].reshape(E, 8), np.hstack([a1[:, 0], a2[:, 0]]))
    sim.close()


def test_controller_modes_need_a_controller():
    from gym_pybullet_drones_routing_amd import _lib
    from gym_pybullet_drones_routing_amd.enums import ActionType
    sim = _sim(n_envs=2, act=ActionType.RPM)
    for mode, width, dtype in (("vel", 4, torch.float32), ("waypoint", 7, torch.float64)):
        with pytest.raises(_lib.GpdError, match="no controller") as exc:
            sim.cmd_step(torch.zeros((2, 1, width), dtype=dtype, device="cuda"), mode)
        assert exc.value.code == _lib.GPD_EINVAL
        assert sim._lib.gpd_last_error().decode() in str(exc.value)
    with pytest.raises(ValueError):
        sim.cmd_step(torch.zeros((2, 1, 4), dtype=torch.float64, device="cuda"), "thrust")
    with pytest.raises(ValueError):
        sim.cmd_step(torch.zeros((2, 1, 7), dtype=torch.float64, device="cuda"), "rpm")
    np.testing.assert_array_equal(sim.step_counters().cpu().numpy(), [0, 0])      # nothing ran
    sim.close()


def test_graph_replay_matches_eager():
    """gpd_cmd_step has no host mutable state: 8 captured calls replayed twice == 16 eager calls, bit
    for bit.  (RPM / no-drag sims, whose kernel also writes the last-action mark; no RL step runs
    here, so the mark is never pending: test_interleaves_with_the_rl_step covers that.)"""
    rng = np.random.default_rng(24)
    E, G = 70, 8
    acts = [torch.from_numpy(HOVER * (1 + 0.05 * rng.uniform(-1, 1, (E, 1, 4)))).cuda() for _ in range(G)]
    a = _sim(n_envs=E, task="hover")
    b = _sim(n_envs=E, task="hover")
    g = b.capture_cmd_graph(acts, "rpm")
    for rep in range(2):
        for k in range(G):
            oa = a.cmd_step(acts[k], "rpm")
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(oa, b._obs20)
    assert torch.equal(a.raw_state(), b.raw_state())
    assert torch.equal(a.step_counters(), b.step_counters())
    assert int(a.step_counters()[0]) == 16 * a.pyb_steps_per_ctrl
    a.close()
    b.close()


# ------------------------------------------------------------------ adjacency
def _set_positions(sim, pos):
    raw = sim.raw_state().cpu().numpy()
    raw[:, 0:3] = pos.reshape(-1, 3)
    sim.set_raw_state(raw)


def test_adjacency_matches_the_reference_loop():
    E, D = 3, 5
    R0 = 0.625                                    # |(3, 4, 0)| / 8, exact in binary
    rng = np.random.default_rng(25)
    pos = rng.uniform(-0.5, 0.5, (E, D, 3)) + [1.0, 2.0, 1.0]
    pos[0, 0] = [1.0, 2.0, 1.0]
    pos[0, 1] = pos[0, 0] + [0.375, 0.5, 0.0]     # exactly R0 from drone 0
    pos[0, 2] = pos[0, 0] + [0.0, -0.375, 0.5]    # exactly R0 from drone 0
    pos[0, 3] = pos[0, 1] + [-0.5, 0.0, 0.375]    # exactly R0 from drone 1
    sim = _sim(n_envs=E, drones_per_env=D)
    _set_positions(sim, pos)
    exact = [(0, 1), (0, 2), (1, 3)]
    for i, j in exact:
        assert np.linalg.norm(pos[0, i] - pos[0, j]) == R0
    for radius, at_r0 in ((R0, 0), (np.nextafter(R0, np.inf), 1)):
        for e in range(E):     # every other pair is far enough from the radius for any summation order
            d = np.linalg.norm(pos[e][:, None] - pos[e][None], axis=-1)
            far = np.abs(d - radius) >= 1e-9
            if e == 0:
                for i, j in exact:
                    far[i, j] = far[j, i] = True
            assert far.all()
        adj = sim.adjacency(radius)
        assert adj.shape == (E, D, D) and adj.dtype == torch.uint8
        adj = adj.cpu().numpy()
        for e in range(E):
            np.testing.assert_array_equal(adj[e], adjacency_loop(pos[e], radius))
        for i, j in exact:                        # strict <: 0 at the radius, 1 at its next double up
            assert adj[0, i, j] == adj[0, j, i] == at_r0
    assert bool((sim.adjacency(np.inf) == 1).all())
    assert bool((sim.adjacency(0.0) == torch.eye(D, dtype=torch.uint8, device="cuda")).all())
    sim.close()


def test_adjacency_65_drones():
    E, D, radius = 2, 65, 0.5
    rng = np.random.default_rng(26)
    pos = rng.uniform(0, 1.5, (E, D, 3)) + [0, 0, 0.5]
    d = np.linalg.norm(pos[:, :, None] - pos[:, None], axis=-1)
    assert (np.abs(d - radius) >= 1e-9).all()
    sim = _sim(n_envs=E, drones_per_env=D)
    _set_positions(sim, pos)
    adj = sim.adjacency(radius).cpu().numpy()
    for e in range(E):
        np.testing.assert_array_equal(adj[e], adjacency_loop(pos[e], radius))
    assert 0 < adj.mean() < 1
    sim.close()


# ------------------------------------------------------------------ Gym surface
def _check_surface(env, action):
    obs, info = env.reset()
    assert obs.shape == (2, 20) and obs.dtype == np.float64 and info == {"answer": 42}
    assert env.observation_space.shape == (2, 20) and env.action_space.shape == (2, 4)
    assert env.observation_space.contains(obs.astype(np.float32))
    assert env.action_space.contains(np.asarray(action, dtype=np.float32))
    out = env.step(action)
    assert len(out) == 5
    obs, reward, terminated, truncated, info = out
    assert obs.shape == (2, 20) and obs.dtype == np.float64
    assert reward == -1 and terminated is False and truncated is False and info == {"answer": 42}
    assert env.observation_space.contains(obs.astype(np.float32))
    np.testing.assert_array_equal(env._getDroneStateVector(1), obs[1])
    adj = env._getAdjacencyMatrix()
    assert adj.dtype == np.float64
    np.testing.assert_array_equal(adj, np.ones((2, 2)))            # NEIGHBOURHOOD_RADIUS = inf
    assert env.SPEED_LIMIT == 0.03 * 30.0 * (1000 / 3600) and env.MAX_RPM == MAX_RPM
    assert env.PYB_FREQ == env.CTRL_FREQ == 240 and env.step_counter == 1


def test_gym_classes():
    from gym_pybullet_drones_routing_amd.enums import Physics
    from gym_pybullet_drones_routing_amd.envs import CtrlAviary, VelocityAviary
    for cls in (CtrlAviary, VelocityAviary):
        for kw in (dict(gui=True), dict(record=True), dict(obstacles=True)):
            with pytest.raises(NotImplementedError):
                cls(**kw)
    from gym_pybullet_drones_routing_amd.enums import DroneModel
    env = CtrlAviary(DroneModel.CF2X, 2, user_debug_gui=False, output_folder="ignored")   # positional, as the reference allows
    assert env.PHYSICS == Physics.PYB and env.NUM_DRONES == 2 and not hasattr(env, "ACT_TYPE")
    assert float(env.action_space.high.max()) == float(np.float32(MAX_RPM)) and float(env.action_space.low.min()) == 0
    _check_surface(env, np.full((2, 4), HOVER))
    # ten steps at hover RPM against the reference; then the on-device controller (the addition)
    ref = CmdRefAviary(num_drones=2, drones_per_env=2, integrator="bullet", ctrl_freq=240)
    env.reset()
    for _ in range(10):
        obs = env.step(np.full((2, 4), HOVER))[0]
        want = ref.cmd_step("rpm", np.full((2, 4), HOVER))
    _check_state("CtrlAviary.step", obs, want)
    np.testing.assert_array_equal(obs[:, 16:20], want[:, 16:20])
    tgt = env.INIT_XYZS + [0, 0, 0.2]
    obs = env.step_to(tgt, target_rpy=np.array([[0, 0, 0.1]] * 2))[0]
    w = np.hstack([tgt, np.full((2, 1), 0.1), np.zeros((2, 3))])
    _check_state("CtrlAviary.step_to", obs, ref.cmd_step("waypoint", w))
    env.close()
    env = VelocityAviary(DroneModel.CF2X, 2, 10)
    _check_surface(env, np.array([[1, 0, 0, 0.5], [0, 0, 1, 1.0]]))
    env.close()
    try:
        import gymnasium
    except ImportError:
        return
    for gym_id in ("ctrl-aviary-v0", "velocity-aviary-v0", "hover-aviary-v0", "multihover-aviary-v0"):
        assert gym_id in gymnasium.envs.registration.registry
    for gym_id, cls in (("ctrl-aviary-v0", CtrlAviary), ("velocity-aviary-v0", VelocityAviary)):
        made = gymnasium.make(gym_id, num_drones=2, disable_env_checker=True)
        assert isinstance(made.unwrapped, cls)
        made.unwrapped.close()


def test_pid_example_runs(tmp_path):
    """examples/pid.py end to end at a tiny size (in this process): finite states, the drones stay
    near their circle, the log is saved."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "pid.py")
    spec = importlib.util.spec_from_file_location("example_pid", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    err, bad = mod.run(num_envs=4, num_drones=2, duration_sec=0.5, output_folder=str(tmp_path / "out"))
    assert not bad and np.isfinite(err) and err < 0.2, err
    assert any(name.endswith(".npy") for name in os.listdir(tmp_path / "out"))
