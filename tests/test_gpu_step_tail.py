"""The tail of the three-wave step kernel (step_kernel_duo, IO = true).

The io wave forms its DMA offsets, the (row, column) mapping of its elements and its store
offsets in its slack at the first hand-offs, with one register-resident pass for blocks whose
nact * L history elements fit 4 per lane and the per-pass loop for longer ones, and stores the
terminal rows of that pass from registers; the pose wave holds the task target and the reset
template in registers from entry, decides `terminated` from the squared distance (the square
root only inside a 1 % band around 1e-8), and forms its last stores' addresses and values
before the final barrier.  None of this may change a result:
  * the io kernel against the one-wave kernel over block fills, action widths, precisions,
    ring lengths and substep counts, with resets in lanes other than lane 0 and a reset
    template that is not the default;
  * `terminated` (norm of the distance < 1e-4) against the C oracle for squared distances well
    below 1e-8, within 1 % of it on both sides (the kernel's band), and well above it.
"""
import numpy as np
import pytest

from oracle.c_oracle import COracle
from tests.oracle_runs import assert_obs_match, state_rel_err

HOVER_Z = 1.0   # HoverAviary's target is (0, 0, 1)
INIT_XYZ = np.array([[0.3, -0.2, 1.97]])
INIT_RPY = np.array([[0.05, -0.03, 0.2]])
T_STEPS = 20


def _sim(**kw):
    from gym_pybullet_drones_routing_amd.sim import BatchedAviarySim
    return BatchedAviarySim(device="cuda:0", **kw)


def _actions(E, A):
    """Small random actions; every odd env is driven out of bounds within the first steps: a
    full roll torque (RPM: tilt past 0.4 rad in 2-3 steps) or full thrust from z = 1.97
    (ONE_D_RPM: z > 2 after ~8 steps), again after each reset."""
    rng = np.random.default_rng(7)
    acts = rng.uniform(-0.05, 0.05, (T_STEPS, E, 1, A)).astype(np.float32)
    kick = np.array([1, -1, -1, 1], np.float32) if A == 4 else np.array([1], np.float32)
    acts[:, 1::2, 0, :] = kick
    if E == 1:
        acts[:, 0, 0, :] = kick
    return acts


def _run(waves, E, act, prec, dpb, pyb_freq, ctrl_freq):
    import torch
    from gym_pybullet_drones_routing_amd.enums import ActionType
    A = 4 if act == "rpm" else 1
    acts = _actions(E, A)
    sim = _sim(n_envs=E, task="hover", precision=prec, act=ActionType(act), pyb_freq=pyb_freq, ctrl_freq=ctrl_freq,
               initial_xyzs=INIT_XYZ, initial_rpys=INIT_RPY, tuning={"step_waves": waves, "drones_per_block": dpb})
    assert sim.constants.lanes_per_block == 64 * waves
    assert sim.constants.drones_per_block == dpb
    assert sim.constants.action_buffer_size == ctrl_freq // 2
    assert sim.constants.pyb_steps_per_ctrl == pyb_freq // ctrl_freq
    rec = []
    for t in range(T_STEPS):
        o, r, te, tr = sim.step(torch.from_numpy(acts[t]).cuda())
        rec.append((o.cpu().numpy().copy(), r.cpu().numpy().copy(), te.cpu().numpy().astype(bool),
                    tr.cpu().numpy().astype(bool), sim.terminal_obs.cpu().numpy().copy(),
                    sim.step_counters().cpu().numpy().copy()))
    st = sim.state20().cpu().numpy()
    sim.close()
    return rec, st


def _compare(E, act, prec, dpb, pyb_freq=240, ctrl_freq=30):
    ri, si = _run(3, E, act, prec, dpb, pyb_freq, ctrl_freq)
    rs, ss = _run(1, E, act, prec, dpb, pyb_freq, ctrl_freq)
    # as test_duo_kernel_matches_single_wave: the two code shapes contract a few multiply-adds differently
    tol = 1e-12 if prec == "f64" else 1e-4
    atol = tol if prec == "f64" else 1e-5
    done_envs = set()
    for t in range(T_STEPS):
        (oi, rwi, tei, tri, ti, sci), (os_, rws, tes, trs, ts, scs) = ri[t], rs[t]
        np.testing.assert_array_equal(tei, tes, err_msg=f"terminated, step {t}")
        np.testing.assert_array_equal(tri, trs, err_msg=f"truncated, step {t}")
        np.testing.assert_array_equal(sci, scs, err_msg=f"step counters, step {t}")
        assert_obs_match(oi, os_, tol, atol, err_msg=f"obs, step {t}")
        np.testing.assert_allclose(rwi, rws, rtol=tol, atol=atol, err_msg=f"reward, step {t}")
        for e in np.nonzero(tei | tri)[0]:
            done_envs.add(int(e))
            assert_obs_match(ti[e], ts[e], tol, atol, err_msg=f"terminal_obs of env {e}, step {t}")
            # the reset row: the (non-default) template's position and Euler angles, zero velocities
            np.testing.assert_allclose(oi[e, 0, 0:3], INIT_XYZ[0], rtol=1e-6, atol=0)
            np.testing.assert_allclose(oi[e, 0, 3:6], INIT_RPY[0], rtol=1e-5, atol=0)
            np.testing.assert_array_equal(oi[e, 0, 6:12], np.zeros(6, np.float32))
            assert sci[e] == 0
    assert state_rel_err(si, ss).max() <= tol
    assert done_envs, "the inputs should force resets"
    assert E == 1 or any(e % 64 != 0 for e in done_envs), "resets in lanes other than lane 0"


@pytest.mark.gpu
@pytest.mark.parametrize("dpb", [16, 64])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("act", ["rpm", "one_d_rpm"])
@pytest.mark.parametrize("E", [1, 17, 40])
def test_io_kernel_matches_single_wave(E, act, prec, dpb):
    """Ring length 15, 8 substeps.  16 drones per block: 16 x 15 = 240 elements, the io wave's
    register-resident pass (the bench's block shape), last blocks of 1 (E = 1, 17) and 8 (E = 40)
    drones; 64 per block: 17 or 40 lanes of one block active, RPM's 255 (E = 17) elements in one
    pass and 600 (E = 40) through the per-pass loop."""
    _compare(E, act, prec, dpb)


@pytest.mark.gpu
@pytest.mark.parametrize("act", ["rpm", "one_d_rpm"])
@pytest.mark.parametrize("pyb_freq,ctrl_freq", [(240, 48), (30, 30), (480, 30)])
def test_io_kernel_other_rings_and_substeps(pyb_freq, ctrl_freq, act):
    """ctrl_freq 48: ring length 24, 23 DMA slots (the loop unrolled by 8 plus its remainder), a
    full block's 16 x 24 = 384 elements through the per-pass loop and the last block's 24 in one
    pass; one substep (a single hand-off) and 16 substeps."""
    _compare(17, act, "f64", 16, pyb_freq, ctrl_freq)


# ------------------------------------------------------------------ `terminated` around |d| = 1e-4
# d2 = |target - pos|^2 against the band [0.99e-8, 1.01e-8] around the threshold's square: below
# it, inside it on both sides of 1e-8, above it.  Zero velocity and hover RPM keep the drone where it is put (the thrust
# balances gravity to rounding), so d2 after the step is the offset's square to ~1e-12 relative.
CLEAR = [((0.5e-4, 0, 0), True), ((0.99e-4, 0, 0), True),          # d2 = 0.25e-8, 0.9801e-8 < lo
         ((1.01e-4, 0, 0), False), ((2e-4, 0, 0), False),          # d2 = 1.0201e-8 > hi, 4e-8
         ((0, -0.7e-4, 0), True), ((0.8e-4, 0.8e-4, 0), False)]    # d2 = 0.49e-8, 1.28e-8
BAND = [((0.999e-4, 0, 0), True), ((1.001e-4, 0, 0), False),       # d2 = 0.998e-8, 1.002e-8
        ((0.9955e-4, 0, 0), True), ((1.0045e-4, 0, 0), False),     # just inside the band's ends
        ((0, 0.9999e-4, 0), True), ((0.7072e-4, -0.7072e-4, 0), False)]   # d2 = 0.9998e-8, 1.00026e-8
BAND_Z = [((0, 0, 0.999e-4), True), ((0, 0, -1.001e-4), False)]    # f64 only: 1 + 1e-4 is coarse in f32


def _term_cases(group, prec):
    cases = {"clear": CLEAR, "band": BAND + CLEAR[:2] + CLEAR[3:4]}[group]
    if group == "band" and prec == "f64":
        cases = cases + BAND_Z
    return cases


def _term_raw(cases):
    raw = np.zeros((len(cases), 20))
    raw[:, 2] = HOVER_Z
    raw[:, 0:3] += np.array([c[0] for c in cases])
    raw[:, 6] = 1.0   # identity quaternion
    return raw


def _oracle_terminated(cases):
    orc = COracle(len(cases), task="hover")
    orc.set_raw_state(_term_raw(cases))
    _, _, te, tr = orc.step(np.zeros((len(cases), 1, 4), np.float32))
    assert not tr.any()
    orc.close()
    return te.copy()


@pytest.mark.parametrize("group", ["clear", "band"])
def test_oracle_gives_both_outcomes(group):
    """CPU: the C oracle terminates exactly the chosen inputs whose offset is shorter than 1e-4."""
    cases = _term_cases(group, "f64")
    te = _oracle_terminated(cases)
    expect = np.array([c[1] for c in cases])
    np.testing.assert_array_equal(te, expect)
    assert expect.any() and not expect.all()
    d2 = np.array([np.dot(c[0], c[0]) for c in cases])
    in_band = (d2 >= 0.99e-8) & (d2 <= 1.01e-8)
    assert in_band.any() == (group == "band")
    if group == "band":
        assert (in_band & (d2 < 1e-8)).any() and (in_band & (d2 > 1e-8)).any()
        assert (d2 < 0.99e-8).any() and (d2 > 1.01e-8).any()


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [3, 2])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("group", ["clear", "band"])
def test_terminated_matches_oracle(group, prec, waves):
    """"clear": no lane of the wave is within 1 % of the threshold; "band": lanes inside the band
    on both sides of 1e-8 beside lanes outside it.  Both must give the oracle's flags."""
    import torch
    cases = _term_cases(group, prec)
    te_ref = _oracle_terminated(cases)
    E = len(cases)
    sim = _sim(n_envs=E, task="hover", precision=prec, tuning={"step_waves": waves})
    assert sim.constants.lanes_per_block == 64 * waves
    sim.set_raw_state(_term_raw(cases))
    _, _, te, tr = sim.step(torch.zeros((E, 1, 4), dtype=torch.float32, device="cuda:0"))
    te, tr = te.cpu().numpy().astype(bool), tr.cpu().numpy().astype(bool)
    sim.close()
    assert not tr.any()
    np.testing.assert_array_equal(te, te_ref)
