"""GPU tests of the per-drone DSLPIDControl gains (gpd_set_pid_gains) in the command step and the
rollout, against tests/cmd_ref.CmdRefAviary with each RefDSLPID's own coefficients
(tests/pid_gains_flights.py: the flights, the gain recipe and the references, whose conditions
tests/test_pid_gains_host.py checks on the oracle alone).  Gates of tests/test_gpu_cmd_step.py:
state_rel_err f64 max / median <= 1e-10, controller state rtol = atol = 1e-9, counters exact.
Everything that compares two device runs compares bit for bit.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.pid_gains_flights import FLIGHTS, START1, actions, gain_rows, reference
from tests.test_gpu_cmd_rollout import _track_ref
from tests.test_gpu_cmd_step import HOVER, _check_state, _sim, _waypoints

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("p_coeff_pos", "i_coeff_pos", "d_coeff_pos", "p_coeff_att", "i_coeff_att", "d_coeff_att")


def _np(t):
    return t.cpu().numpy()


def _kw(rows, E, D):
    g = np.asarray(rows).reshape(E, D, 6, 3)
    return {k: g[:, :, i] for i, k in enumerate(KEYS)}


def _flight_sim(name, rows=None, prec="f64"):
    from gym_pybullet_drones_routing_amd.enums import ActionType, Physics
    f = FLIGHTS[name]
    sim = _sim(n_envs=f["E"], drones_per_env=f["D"], act=ActionType.VEL, physics=Physics.PYB, aero=f["aero"],
               ctrl_freq=f["ctrl_freq"], initial_xyzs=f["xyz"], precision=prec)
    if rows is not None:
        sim.set_pid_gains(**_kw(rows, f["E"], f["D"]))
    return sim


def _acts(name, sim):
    a = torch.from_numpy(np.array(actions(name)))
    return (a if FLIGHTS[name]["mode"] == "vel" else a.to(sim.real_dtype)).cuda()


def _rows(name):
    f = FLIGHTS[name]
    return gain_rows(f["seed"], f["E"] * f["D"])


def _left(sim, **more):
    """What a flight leaves in the sim, on the host."""
    out = dict(raw=_np(sim.raw_state()), ctrl=_np(sim.ctrl_state()), counters=_np(sim.step_counters()),
               state20=_np(sim.state20()))
    out.update({k: _np(v) for k, v in more.items() if v is not None})
    return out


def _same(a, b, keys=None):
    for k in keys or sorted(set(a) & set(b)):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _check_against_reference(name, label, left):
    f = FLIGHTS[name]
    ref = reference(name)
    _check_state(f"pid_gains {name} {label}", left["state20"], ref["traj"][-1])
    np.testing.assert_allclose(left["ctrl"], ref["ctrl"], rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(left["counters"], np.full(f["E"], f["T"] * (240 // f["ctrl_freq"])))


@functools.lru_cache(maxsize=None)
def _fly(name, how, prec="f64", tuned=True):
    """The flight with the recipe's gains: "step" (T cmd_step calls), "one" (one cmd_rollout call),
    "split" (calls of 5 and T - 5 steps) or "chunk3" (one call, launches of at most 3 steps)."""
    f = FLIGHTS[name]
    sim = _flight_sim(name, _rows(name) if tuned else None, prec)
    a = _acts(name, sim)
    met = f["mode"] == "waypoint"
    more = {}
    if how == "step":
        for t in range(f["T"]):
            obs = sim.cmd_step(a[t], f["mode"])
        more["obs"] = obs
    elif how == "split":
        t1, _, _ = sim.cmd_rollout(a[:5], f["mode"], metrics=met)
        t2, obs, m = sim.cmd_rollout(a[5:], f["mode"], metrics=met)
        more.update(traj=torch.cat([t1, t2]), obs=obs, metrics=m)
    else:
        traj, obs, m = sim.cmd_rollout(a, f["mode"], metrics=met, max_steps_per_launch=3 if how == "chunk3" else 0)
        more.update(traj=traj, obs=obs, metrics=m)
    out = _left(sim, **more)
    out["gains"] = sim.pid_gains()
    sim.close()
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ------------------------------------------------------------------ 1. waypoint parity
def test_waypoint_step_parity_and_readback():
    name = "wp3x3"
    f = FLIGHTS[name]
    r = _fly(name, "step")
    _check_against_reference(name, "cmd_step", r)
    np.testing.assert_array_equal(r["obs"].reshape(-1, 20), r["state20"])
    want = _kw(_rows(name), f["E"], f["D"])
    assert sorted(r["gains"]) == sorted(KEYS)
    for k in KEYS:
        assert r["gains"][k].shape == (f["E"], f["D"], 3) and r["gains"][k].dtype == np.float64
        np.testing.assert_array_equal(r["gains"][k], want[k], err_msg=k)


# ------------------------------------------------------------------ 2. rollout, chunking
def test_waypoint_rollout_parity_and_chunking():
    name = "wp3x3"
    one = _fly(name, "one")
    _check_against_reference(name, "cmd_rollout", one)
    np.testing.assert_array_equal(one["obs"], one["traj"][-1])
    s, m = _track_ref(one["traj"], np.array(actions(name)))
    assert s.min() > 0
    np.testing.assert_allclose(one["metrics"][..., 0], s, rtol=1e-12)
    np.testing.assert_allclose(one["metrics"][..., 1], m, rtol=1e-12)
    for how in ("split", "chunk3"):
        other = _fly(name, how)
        _same(other, one, ("raw", "ctrl", "traj", "counters", "obs"))
        if how == "chunk3":     # one flight: the figures carry over from launch to launch
            np.testing.assert_array_equal(other["metrics"], one["metrics"])


# ------------------------------------------------------------------ 3. / 4. VEL mode, the wide kernel
@pytest.mark.parametrize("name", ["vel5x2", "wp2x65"])
@pytest.mark.parametrize("how", ["step", "one"])
def test_vel_and_wide_parity(name, how):
    """vel5x2: the VEL targets (pid_targets) on the lane's own constants.  wp2x65: cmd_step_kernel_wide;
    the rollout issues it once per step.  Two envs: the second workgroup's env offset into the table."""
    _check_against_reference(name, how, _fly(name, how))


# ------------------------------------------------------------------ 5. placement independence
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_result_follows_the_gains_not_the_lane(prec):
    name = "wp70x1"
    f = FLIGHTS[name]
    E = f["E"]
    rows = _rows(name)
    out = []
    for r in (rows, rows[::-1]):
        sim = _flight_sim(name, np.ascontiguousarray(r), prec)
        a = _acts(name, sim)
        _, _, met = sim.cmd_rollout(a, "waypoint", record=False, metrics=True)
        nxt = torch.from_numpy(np.array([_waypoints(START1, f["T"], 0) for _ in range(E)])).to(sim.real_dtype).cuda()
        sim.cmd_step(nxt, "waypoint")
        out.append(_left(sim, metrics=met))
        sim.close()
    fwd, rev = out
    assert np.isfinite(fwd["raw"]).all()
    assert len(np.unique(fwd["raw"][:, 0:3], axis=0)) == E      # the gains did tell the drones apart
    for k in ("state20", "raw", "ctrl", "metrics"):
        np.testing.assert_array_equal(rev[k].reshape(E, -1), fwd[k].reshape(E, -1)[::-1], err_msg=k)


# ------------------------------------------------------------------ 6. a table of the sim-wide gains
NONDEFAULT = dict(p_coeff_pos=[.5, .3, 1.0], i_coeff_pos=[.04, .06, .05], d_coeff_pos=[.25, .15, .6],
                  p_coeff_att=[60000., 80000., 50000.], i_coeff_att=[3., 7., 400.], d_coeff_att=[25000., 15000., 10000.])


@pytest.mark.parametrize("how", ["step", "rollout"])
@pytest.mark.parametrize("name,prec,coeffs", [("wp3x3", "f64", False), ("wp3x3", "f32", False), ("vel5x2", "f64", False),
                                              ("vel5x2", "f32", False), ("wp3x3", "f64", True),
                                              # the single-drone and the wide instantiations (the wide one holds the
                                              # row in registers)
                                              ("wp70x1", "f64", True), ("wp70x1", "f32", False),
                                              ("wp2x65", "f64", True), ("wp2x65", "f32", False)])
def test_table_of_the_sim_wide_gains_changes_nothing(name, prec, coeffs, how):
    """A sim whose table repeats the sim-wide coefficients against a sim without a table, bit for bit.

    The two are different instantiations of the same kernels, and the multi-drone Physics.PYB ones carry
    the Bullet integrator and the pair contact with FP contraction left to the compiler, so this also
    pins how the table's instantiation is written: its controller reads the constants through a
    pointer, as the no-table one does, and the row is staged ahead of every load the no-table kernel
    has.  With the row held in registers and loaded beside the controller state, 4 of these 10 cases
    differed in the last bit."""
    f = FLIGHTS[name]
    E, D, mode = f["E"], f["D"], f["mode"]
    met = mode == "waypoint"
    plain, tab = _flight_sim(name, None, prec), _flight_sim(name, None, prec)
    if coeffs:
        plain.set_pid_coefficients(**NONDEFAULT)
        tab.set_pid_coefficients(**NONDEFAULT)
    before = tab.pid_gains()
    tab.set_pid_gains()                      # the gains in force, now as a table
    after = tab.pid_gains()
    for k in KEYS:
        np.testing.assert_array_equal(after[k], before[k])
        np.testing.assert_array_equal(after[k], plain.pid_gains()[k])
        if coeffs:
            want = np.asarray(NONDEFAULT[k], dtype=np.float32 if prec == "f32" else np.float64).astype(np.float64)
            np.testing.assert_array_equal(after[k], np.broadcast_to(want, (E, D, 3)))
    a = _acts(name, plain)
    left = []
    for sim in (plain, tab):
        if how == "step":
            rows = torch.stack([sim.cmd_step(a[t], mode).clone() for t in range(f["T"])])
            left.append(_left(sim, traj=rows))
        else:
            traj, obs, m = sim.cmd_rollout(a, mode, metrics=met)
            left.append(_left(sim, traj=traj, obs=obs, metrics=m))
    assert np.isfinite(left[0]["raw"]).all()
    _same(left[1], left[0])
    # cleared: on as if there had never been a table
    tab.clear_pid_gains()
    for _ in range(2):
        o_p, o_t = plain.cmd_step(a[-1], mode), tab.cmd_step(a[-1], mode)
        assert torch.equal(o_p, o_t)
    _same(_left(tab), _left(plain))
    # RPM mode runs no controller: a table in force changes nothing
    tab.set_pid_gains(**_kw(_rows(name), E, D))
    rng = np.random.default_rng(3)
    rpm = torch.from_numpy(HOVER * (1 + 0.05 * rng.uniform(-1, 1, (E, D, 4)))).to(plain.real_dtype).cuda()
    assert torch.equal(plain.cmd_step(rpm, "rpm"), tab.cmd_step(rpm, "rpm"))
    _same(_left(tab), _left(plain))
    plain.close()
    tab.close()


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_rpm_mode_and_clear_on_their_own(prec):
    """With the recipe's table in force an RPM-mode step is the step of a sim without a table, and after
    clear_pid_gains() the flight is that sim's flight, by cmd_step and by cmd_rollout (the same kernels)."""
    name = "wp3x3"
    f = FLIGHTS[name]
    plain, tab = _flight_sim(name, None, prec), _flight_sim(name, _rows(name), prec)
    rng = np.random.default_rng(3)
    rpm = torch.from_numpy(HOVER * (1 + 0.05 * rng.uniform(-1, 1, (f["E"], f["D"], 4)))).to(plain.real_dtype).cuda()
    assert torch.equal(plain.cmd_step(rpm, "rpm"), tab.cmd_step(rpm, "rpm"))
    _same(_left(tab), _left(plain))
    tab.clear_pid_gains()
    a = _acts(name, plain)
    for t in range(8):
        assert torch.equal(plain.cmd_step(a[t], "waypoint"), tab.cmd_step(a[t], "waypoint"))
    out = [sim.cmd_rollout(a[8:], "waypoint", metrics=True) for sim in (plain, tab)]
    assert all(torch.equal(x, y) for x, y in zip(*out))
    _same(_left(tab), _left(plain))
    for k, v in tab.pid_gains().items():
        np.testing.assert_array_equal(v, plain.pid_gains()[k])
    plain.close()
    tab.close()


# ------------------------------------------------------------------ 7. graph
def test_graph_sees_new_values_without_recapture():
    from gym_pybullet_drones_routing_amd.sim import graph_capture
    name = "wp3x3"
    f = FLIGHTS[name]
    E, D, T = f["E"], f["D"], 4
    rows_a, rows_b = _rows(name), gain_rows(55, E * D)
    cap = _flight_sim(name, rows_a)
    w = _acts(name, cap)[:T].contiguous()
    raw0, cs0, sc0 = cap.raw_state(), cap.ctrl_state(), cap.step_counters()
    cap._cmd_rows()     # allocated outside the capture
    g = torch.cuda.CUDAGraph()
    with graph_capture(g, cap.device):
        traj_g, obs_g, met_g = cap.cmd_rollout(w, "waypoint", metrics=True)
    assert int(cap.step_counters()[0]) == 0        # capture records only
    g.replay()
    torch.cuda.synchronize()
    for rows in (rows_a, rows_b):
        if rows is rows_b:      # new values into the same table, the captured graph as it is, the start state again
            cap.set_pid_gains(**_kw(rows_b, E, D))
            cap.set_raw_state(raw0)
            cap.set_ctrl_state(cs0)
            cap.set_step_counters(sc0)
            g.replay()
            torch.cuda.synchronize()
        eager = _flight_sim(name, rows)
        traj_e, obs_e, met_e = eager.cmd_rollout(w, "waypoint", metrics=True)
        assert torch.equal(traj_g, traj_e) and torch.equal(obs_g, obs_e) and torch.equal(met_g, met_e)
        assert torch.equal(cap.raw_state(), eager.raw_state()) and torch.equal(cap.ctrl_state(), eager.ctrl_state())
        assert torch.equal(cap.step_counters(), eager.step_counters())
        assert int(cap.step_counters()[0]) == T * 5
        eager.close()
    assert not torch.equal(traj_g[-1], torch.from_numpy(np.array(_fly(name, "one")["traj"][T - 1])).cuda())
    del g
    cap.close()


# ------------------------------------------------------------------ 8. refusals
def test_refusals_run_nothing():
    from gym_pybullet_drones_routing_amd import _lib
    from gym_pybullet_drones_routing_amd.enums import ActionType
    from gym_pybullet_drones_routing_amd.sim import _dptr
    E = 3
    rows = gain_rows(9, E)
    sim, twin = (_sim(n_envs=E, act=ActionType.VEL, task="hover") for _ in range(2))
    sim.set_pid_gains(**_kw(rows, E, 1))
    a = torch.zeros((E, 1, 4), dtype=torch.float32, device="cuda")
    with pytest.raises(NotImplementedError, match="sim-wide"):
        sim.step(a)
    with pytest.raises(NotImplementedError, match="sim-wide"):
        sim.step_seq(a.reshape(1, E, 1, 4), 2)
    rc = sim._step_fn(sim._h, a.data_ptr(), *sim._out_ptrs, None, None)
    assert rc == _lib.GPD_EUNSUPPORTED and b"sim-wide" in sim._lib.gpd_last_error()
    rc = sim._lib.gpd_step_seq(sim._h, a.data_ptr(), 1, 2, *sim._out_ptrs, None, None)
    assert rc == _lib.GPD_EUNSUPPORTED and b"sim-wide" in sim._lib.gpd_last_error()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(sim.step_counters()), np.zeros(E))
    assert torch.equal(sim.raw_state(), twin.raw_state())

    # a NaN row: refused with its place named, the table in force stays what it was
    bad = rows.copy()
    bad[2, 13] = np.nan
    assert sim._lib.gpd_set_pid_gains(sim._h, _dptr(bad)) == _lib.GPD_EINVAL
    assert b"row 2, column 13" in sim._lib.gpd_last_error()
    with pytest.raises(ValueError, match="row 2, column 13"):
        sim.set_pid_gains(i_coeff_att=bad[:, 12:15].reshape(E, 1, 3))
    got = sim.pid_gains()
    for k, v in _kw(rows, E, 1).items():
        np.testing.assert_array_equal(got[k], v)
    twin.set_pid_gains(**_kw(rows, E, 1))
    v = torch.tensor([[[1.0, 0.5, -0.2, 0.7]]] * E, dtype=torch.float32, device="cuda")
    assert torch.equal(sim.cmd_step(v, "vel"), twin.cmd_step(v, "vel"))
    with pytest.raises(NotImplementedError):        # still in force
        sim.step(a)

    # cleared: the RL step works as before
    sim.clear_pid_gains()
    twin.clear_pid_gains()
    o1 = sim.step(a)[0].clone()
    o2 = twin.step(a)[0]
    assert torch.equal(o1, o2)
    np.testing.assert_array_equal(_np(sim.step_counters()), np.full(E, 2 * sim.pyb_steps_per_ctrl))
    sim.close()
    twin.close()

    # no controller: an RPM sim, and every het sim
    for s in (_sim(n_envs=E, act=ActionType.RPM), _sim(n_envs=E, env_params={})):
        assert s._lib.gpd_set_pid_gains(s._h, _dptr(rows)) == _lib.GPD_EINVAL
        assert b"no controller" in s._lib.gpd_last_error()
        assert s._lib.gpd_set_pid_gains(s._h, None) == _lib.GPD_EINVAL
        with pytest.raises(_lib.GpdError, match="no controller"):
            s.set_pid_gains()
        s.close()


def test_env_classes_pass_the_gains_on():
    from gym_pybullet_drones_routing_amd.enums import ActionType
    from gym_pybullet_drones_routing_amd.envs import CtrlAviary, HoverAviary
    xyz = np.array([[0, 0, 0.5], [1, 0, 0.6]])
    rows = gain_rows(10, 2)
    envs = [CtrlAviary(num_drones=2, initial_xyzs=xyz, ctrl_freq=48) for _ in range(2)]
    envs[0].set_pid_gains(**_kw(rows, 1, 2))
    tgt = xyz + [0.1, -0.1, 0.05]
    obs = [env.step_to(tgt)[0] for env in envs for _ in range(3)][2::3]
    assert np.isfinite(obs[0]).all() and not np.array_equal(obs[0][:, 0:3], obs[1][:, 0:3])
    got = envs[0].sim.pid_gains()
    for k, v in _kw(rows, 1, 2).items():
        np.testing.assert_array_equal(got[k], v)
    for env in envs:
        env.close()
    rl = HoverAviary(act=ActionType.PID)
    rl.reset()
    rl.set_pid_gains(p_coeff_pos=[.5, .5, 1.5])
    with pytest.raises(NotImplementedError, match="sim-wide"):
        rl.step(np.zeros((1, 3), dtype=np.float32))
    rl.sim.clear_pid_gains()
    rl.step(np.zeros((1, 3), dtype=np.float32))
    rl.close()


# ------------------------------------------------------------------ 9. the example
def test_pid_sweep_example(tmp_path):
    out = tmp_path / "sweep.json"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "pid_sweep.py"), "--envs", "64", "--steps", "48",
                          "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout
    r = json.loads(lines[0])
    assert json.loads(out.read_text()) == r
    assert r["envs"] == 64 and r["steps"] == 48 and 0 <= r["best_index"] < 64
    assert np.isfinite(r["nominal_rms"]) and np.isfinite(r["best_rms"]) and r["nominal_rms"] > 0
    assert r["best_rms"] <= r["nominal_rms"]            # candidate 0 is the nominal
    assert 0 <= r["nonfinite"] < 64
    assert sorted(r["best_gains"]) == sorted(KEYS)
    assert all(len(v) == 3 and np.isfinite(v).all() for v in r["best_gains"].values())
