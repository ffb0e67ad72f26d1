"""Drone <-> drone contact under Physics.PYB* (envs of several drones), GPU vs the oracle.

MultiHoverAviary's drones are colliding Bullet bodies (BaseAviary.py:486-491, stepped together by
p.stepSimulation at :369-370).  The restatement (oracle/bullet_mb.py drone_contact, gpd_dcontact.h
drone_contact) is this repository's own contact set and solver order: parity unpinned against
pybullet, like the ground-plane contact.  These tests pin the HIP path to the oracle:
  * resynced substeps (integrate kernel, run-time flags) over head-on, glancing, stacked, tilted,
    resting-overlap and far-apart pairs, a four-drone pile-up, three-drone envs (64 % 3 != 0: a
    block's last lanes idle), a four-drone pile with six simultaneous contacts (more than the
    env's D) and eight-drone 2 x 2 x 2 stacks in 64-drone blocks (pairs past a block's first 64
    go through the row store, several contacts per env through the LDS rounds): f64 max <= 1e-10
    per substep; f32 median <= 1e-6, max <= 1e-3;
  * resynced control steps through the Physics.PYB flag-set step kernel (MultiHover layout);
  * physics: the pair's linear momentum is unchanged by the contact, the head-on pair stops
    short of interpenetration, and ``no_drone_contact`` lets the drones pass through each other.
"""
import numpy as np
import pytest
import torch

from oracle.bullet_math import quat_from_euler, quat_roundtrip
from oracle.ref_aviary import RefAviary
from tests.oracle_runs import oracle_raw, resynced_substep_errors, state_rel_err
from tests.test_gpu_parity import HOVER, _sim

pytestmark = pytest.mark.gpu


def _pair(p1, v1, p2, v2, rpy1=(0, 0, 0), rpy2=(0, 0, 0), w1=(0, 0, 0), w2=(0, 0, 0)):
    raw = np.zeros((2, 20))
    for k, (p, v, rpy, w) in enumerate(((p1, v1, rpy1, w1), (p2, v2, rpy2, w2))):
        raw[k, 0:3] = p
        raw[k, 3:7] = quat_roundtrip(quat_from_euler(np.array(rpy, dtype=np.float64)))
        raw[k, 7:10] = v
        raw[k, 10:13] = w
        raw[k, 13:16] = w
    raw[:, 16:20] = HOVER
    return raw


def _scenarios():
    """Pairs (D = 2) on collision courses at z = 1 (no plane)."""
    return np.concatenate([
        _pair([0, 0, 1], [1, 0, 0], [0.2, 0, 1], [-1, 0, 0]),                          # head-on, level
        _pair([0, 0, 1], [0.8, 0, 0], [0.2, 0.04, 1], [-0.8, 0, 0]),                    # glancing (friction)
        _pair([0.01, 0, 1.1], [0, 0, -0.6], [0, 0.01, 1.0], [0, 0, 0.6]),               # stacked
        _pair([0, 0, 1], [0.6, 0, 0], [0.17, 0, 1.005], [-0.4, 0, 0.1], rpy2=(0.3, -0.2, 0.5)),  # tilted
        _pair([0, 0, 1], [0, 0, 0], [0.119, 0, 1.0], [0, 0, 0]),                        # resting overlap
        _pair([0, 0, 1], [0.3, 0, 0], [0.25, 0.02, 1.0], [-0.2, 0.1, 0], w2=(0, 0, 4.0)),  # spinning
        _pair([0, 0, 1], [0.1, 0, 0], [1.0, 0, 1.0], [0, 0, 0]),                        # far apart
    ])


def _pileup():
    """Four drones converging on a point (several simultaneous contacts in one env)."""
    raw = np.zeros((4, 20))
    for k, a in enumerate(np.arange(4) * np.pi / 2 + 0.1):
        raw[k, 0:3] = [0.14 * np.cos(a), 0.14 * np.sin(a), 1.0 + 0.004 * k]
        raw[k, 3:7] = [0, 0, 0, 1.0]
        raw[k, 7:10] = [-0.7 * np.cos(a), -0.7 * np.sin(a), 0]
    raw[:, 16:20] = HOVER
    return raw


def _triples():
    """Three-drone envs (D = 3): a head-on pair beside a free drone, and a three-way collision."""
    raw = np.zeros((6, 20))
    raw[0:3, 0:3] = [[0, 0, 1.0], [0.2, 0, 1.0], [0.1, 0.5, 1.0]]
    raw[0:3, 7:10] = [[1, 0, 0], [-1, 0, 0], [0, 0, 0]]
    for k, a in enumerate(np.arange(3) * 2 * np.pi / 3):
        raw[3 + k, 0:3] = [0.075 * np.cos(a), 0.075 * np.sin(a), 1.0 + 0.003 * k]
        raw[3 + k, 7:10] = [-0.5 * np.cos(a), -0.5 * np.sin(a), 0]
    raw[:, 6] = 1.0
    raw[:, 16:20] = HOVER
    return raw


def _pile6():
    """Four drones with six contacts: a touching triangle and a fourth drone falling onto all three."""
    from oracle.params import derived
    hh = derived("cf2x")["collision_h"] / 2
    raw = np.zeros((4, 20))
    tri = [[0, 0, 1.0], [0.1195, 0, 1.0], [0.05975, 0.1035, 1.0]]
    raw[0:3, 0:3] = tri
    raw[3, 0:3] = np.mean(tri, axis=0) + [0, 0, 2 * hh - 0.0005]
    raw[3, 7:10] = [0, 0, -0.6]
    raw[0:3, 7:10] = [[-0.1, -0.05, 0], [0.1, -0.05, 0], [0, 0.1, 0.05]]
    raw[:, 6] = 1.0
    raw[:, 16:20] = HOVER
    return raw


def _cube(rng):
    """Eight drones as a 2 x 2 x 2 stack squeezed together (12+ contacts in one env)."""
    from oracle.params import derived
    hh = derived("cf2x")["collision_h"] / 2
    raw = np.zeros((8, 20))
    for k in range(8):
        raw[k, 0:3] = [0.1195 * (k & 1), 0.1195 * ((k >> 1) & 1), 1.0 + (2 * hh - 0.0005) * (k >> 2)]
        raw[k, 7:10] = -0.3 * (raw[k, 0:3] - [0.06, 0.06, 1.0 + hh]) + rng.uniform(-0.05, 0.05, 3)
        raw[k, 10:13] = rng.uniform(-1, 1, 3)
        raw[k, 13:16] = raw[k, 10:13]
    raw[:, 6] = 1.0
    raw[:, 16:20] = HOVER
    return raw


def _ground_stack():
    """Four drones at the plane: one resting on another that rests on the plane, and one falling onto
    a grounded drone beside them (pair and plane contacts of one env, the sequential split)."""
    from oracle.params import derived
    hh = derived("cf2x")["collision_h"] / 2
    raw = np.zeros((4, 20))
    raw[0:4, 0:3] = [[0, 0, hh], [0.01, 0.005, 3 * hh - 0.0005], [0.1195, 0, hh], [0.1195, 0.01, 3 * hh + 0.01]]
    raw[3, 7:10] = [0, 0, -0.5]
    raw[1, 10:13] = [0.5, -0.3, 0.2]
    raw[:, 6] = 1.0
    raw[:, 16:20] = HOVER
    return raw


def _pyb():
    from gym_pybullet_drones_routing_amd.enums import Physics
    return Physics.PYB


def _cases(D):
    rng = np.random.default_rng(D)
    if D == 2:
        return _scenarios(), None
    if D == 3:
        return _triples(), None
    if D == 4:
        return np.concatenate([_pileup(), _pileup()[::-1].copy(), _pile6()]), None
    # D = 8: eight stacks in one 64-drone block (224 pairs: three row-store chunks)
    return np.concatenate([_cube(rng) for _ in range(8)]), {"drones_per_block": 64}


def _contact_errors(D, prec, fixed_iters, monkeypatch):
    """Resynced substep errors of the _cases(D) batch.  fixed_iters: both solvers run all 50
    Gauss-Seidel iterations (solverResidualThreshold < 0 in the kernel and the oracle), so the
    comparison isolates rounding from WHERE the stopping rule ends a solve."""
    import oracle.bullet_mb as bm
    raw0, tuning = _cases(D)
    tuning = dict(tuning or {})
    if fixed_iters:
        tuning["solver_residual"] = -1.0
        monkeypatch.setattr(bm, "RESIDUAL_THRESHOLD", -1.0)
    n = raw0.shape[0]
    T = 40
    rpms = np.full((T, n, 4), HOVER)
    env = RefAviary(num_drones=n, task="none", integrator="bullet", aero=("no_plane",), drones_per_env=D)
    env.set_raw_state(raw0)
    sim = _sim(n_envs=n // D, drones_per_env=D, task="none", precision=prec, physics=_pyb(), aero=("no_plane",),
               tuning=tuning)
    bm.SOLVE_LOG = []
    try:
        err = resynced_substep_errors(sim, env, rpms)
        iters = list(bm.SOLVE_LOG)
    finally:
        bm.SOLVE_LOG = None
        sim.close()
    sep = np.linalg.norm(env._b_pos[0] - env._b_pos[1])
    big = np.argwhere(err > 1e-3)
    print(f"\n[parity] drone contact D={D} {prec}{' fixed 50 iterations' if fixed_iters else ''}: max {err.max():.3e} "
          f"median {np.median(err):.3e} (pair 0 separation after {T} substeps {sep:.4f} m; oracle solves: "
          f"{len(iters)}, most iterations {max(iters) if iters else 0}); {len(big)} of {err.size} drone-substeps "
          f"above 1e-3 at (substep, drone) {big[:12].tolist()}")
    return err, iters


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("D", [2, 3, 4, 8])
def test_drone_contact_resynced(prec, D, monkeypatch):
    err, _ = _contact_errors(D, prec, False, monkeypatch)
    if prec == "f64":
        assert err.max() <= 1e-10
    elif D < 8:
        # f32: the oracle steps from the sim's f32-rounded state (oracle_runs.resynced_substep_errors)
        assert np.median(err) <= 1e-6 and err.max() <= 1e-3
    else:
        # the squeezed 2 x 2 x 2 stacks: 12+ contacts of four rows each in one island (a face
        # manifold's normal rows span three directions), so f32 rounding inside the narrowphase and
        # the solve is amplified by its conditioning: measured 1.03e-3 on 1 of 2 560 drone-substeps
        # with 4 x 8 Newton chains, 5.1e-3 on 2 with round 6's 16 x 5 (with the oracle stepping from
        # its own f64 state, round 5 gated this at 0.2 - that 0.1 was the input rounding, which the
        # f64 oracle alone reproduces); f64 stays <= 1e-10
        assert np.median(err) <= 1e-6 and (err > 1e-3).mean() <= 1e-3 and err.max() <= 1e-2


@pytest.mark.parametrize("D", [2, 3, 4])
def test_drone_contact_resynced_f32_fixed_iterations(D, monkeypatch):
    """The solver parameters (pybullet's setPhysicsEngineParameter solverResidualThreshold < 0:
    every solve runs all 50 Gauss-Seidel iterations; gpd_config::solver_residual, bullet_mb alike)
    reach the contact kernels: f32 against the f64 oracle, every substep <= 1e-3, every oracle
    solve at the cap.  (The squeezed 8-drone stacks iterated 15 past their convergence drift to
    5.5e-3 in f32: an ill-conditioned island, not gated here.)"""
    err, iters = _contact_errors(D, "f32", True, monkeypatch)
    assert iters and min(iters) == 51             # SOLVER_ITERS + 1: no solve stopped early
    assert np.median(err) <= 1e-6 and err.max() <= 1e-3


@pytest.mark.parametrize("D", [16, 64])
def test_drone_contact_resynced_wide_envs(D):
    """Envs of 16 and 64 drones: 120 / 2016 pairs per env, so a block's pairs run past
    the four register chunks into the [P] pair table (chunks 4..31, the kDcChunks bound at D = 64)
    and hundreds of contacts go through the row store.  2 / 8 squeezed 2 x 2 x 2 stacks per env."""
    rng = np.random.default_rng(D)
    raw0 = np.concatenate([_cube(rng) for _ in range(D // 8)])
    for k in range(D // 8):                        # the stacks of one env side by side, touching
        raw0[8 * k:8 * k + 8, 0] += 0.2385 * (k % 4)
        raw0[8 * k:8 * k + 8, 1] += 0.2385 * (k // 4)
    raw0 = np.concatenate([raw0] * (64 // D))      # one 64-drone block
    n = raw0.shape[0]
    T = 12 if D == 16 else 6
    rpms = np.full((T, n, 4), HOVER)
    env = RefAviary(num_drones=n, task="none", integrator="bullet", aero=("no_plane",), drones_per_env=D)
    env.set_raw_state(raw0)
    sim = _sim(n_envs=n // D, drones_per_env=D, task="none", precision="f64", physics=_pyb(), aero=("no_plane",),
               tuning={"drones_per_block": 64})
    err = resynced_substep_errors(sim, env, rpms)
    print(f"\n[parity] drone contact D={D} f64: max {err.max():.3e} median {np.median(err):.3e}")
    assert err.max() <= 1e-10
    sim.close()


def test_drone_contact_counts_beyond_d():
    """The six-contact pile and the eight-drone stacks really hold more simultaneous contacts than
    their env's D (no slot cap in the oracle either)."""
    from oracle.bullet_math import quat_to_mat
    from oracle.bullet_mb import drone_contacts
    from oracle.params import derived
    p = derived("cf2x")
    for raw, D in ((_pile6(), 4), (_cube(np.random.default_rng(8)), 8)):
        rot = np.array([quat_to_mat(q) for q in raw[:, 3:7]])
        cons = drone_contacts(raw[:, 0:3], rot, p["collision_r"], p["collision_h"] / 2, p["collision_z_offset"])
        assert len(cons) > D


@pytest.mark.parametrize("case", ["2", "3", "4", "4-ground", "8", "2-480hz", "4-480hz", "4-ground-480hz", "8-480hz"])
def test_drone_contact_step_kernel_resynced(case):
    """The Physics.PYB flag-set step kernel (MultiHoverAviary's default physics; the parked call, one
    copy of the substep, the history DMA after the substeps) for D = 2, 3, 4, for a stack on the plane
    (pair and plane contacts together) and for two 2 x 2 x 2 stacks of 8 (near pairs compacted over
    the lanes, several Gauss-Seidel levels).  Not with the downwash: the reference's
    _downwash (BaseAviary.py:785-811) scales as (r_prop / 4 dz)^2 for ANY drone above another within
    10 m, so drones in contact (|dz| < 2.5 cm) or at rounding-level height differences push each
    other with tens to 1e30 N, and a control step amplifies rounding differences beyond any gate
    (tests/tools/dbg_dc8.py: the same stacks without the pair contact fail the same way).
    The -480hz cases run ctrl_freq 480 / pyb_freq 960: the 240-step action history's rows overflow
    the one-wave kernels' LDS tile, and the envs step on step_kernel_wide's one-wave instantiation
    with the same contact solve (48 steps of 2 substeps at 960 Hz: 0.1 s, the collisions included)."""
    from gym_pybullet_drones_routing_amd.enums import ActionType
    D = int(case.split("-")[0])
    hz = case.endswith("480hz")
    freq = dict(pyb_freq=960, ctrl_freq=480) if hz else {}
    physics, aero, lo, hi, tuning = _pyb(), (), -0.2, 0.2, None
    if case.startswith("4-ground"):
        raw0, lo, hi = _ground_stack(), -1.0, -0.9      # ~0.95 hover RPM: the stacks stay down
    elif D == 8:          # eight stacks in one 64-drone block: 224 pairs, several 64-pair passes
        raw0 = np.concatenate([_cube(np.random.default_rng(3 + k)) for k in range(8)])
        tuning = {"drones_per_block": 64}
    else:
        raw0 = {2: _scenarios, 3: _triples, 4: _pile6}[D]()
    n = raw0.shape[0]
    env = RefAviary(num_drones=n, task="none", integrator="bullet", act="rpm", drones_per_env=D, aero=aero, **freq)
    env.set_raw_state(raw0)
    sim = _sim(n_envs=n // D, drones_per_env=D, task="none", precision="f64", physics=physics, act=ActionType.RPM,
               tuning=tuning, **freq)
    if hz:
        assert sim.obs_width == 12 + 240 * 4     # a row only the wide kernel holds
    sim.reset()
    rng = np.random.default_rng(5)
    errs = []
    for t in range(48 if hz else 12):
        a = rng.uniform(lo, hi, (n, 4)).astype(np.float32)
        sim.set_raw_state(oracle_raw(env))
        sim.step(torch.from_numpy(a.reshape(n // D, D, 4)).cuda())
        env.step(a)
        errs.append(state_rel_err(sim.raw_state().cpu().numpy()[None, :, :16], oracle_raw(env)[None, :, :16])[0])
    err = np.array(errs)
    print(f"\n[parity] drone contact, Bullet step kernel {case}: max {err.max():.3e}")
    assert err.max() <= 1e-10
    sim.close()


def test_drone_contact_physics():
    raw0 = _pair([0, 0, 1], [1, 0, 0], [0.2, 0, 1], [-1, 0, 0])
    T = 30
    rpms = np.full((T, 2, 4), HOVER)
    out = {}
    for aero in (("no_plane",), ("no_plane", "no_drone_contact")):
        sim = _sim(n_envs=1, drones_per_env=2, task="none", precision="f64", physics=_pyb(), aero=aero)
        sim.set_raw_state(raw0)
        out[aero] = sim.integrate(rpms, record=True).cpu().numpy()
        sim.close()
    hit, free = out[("no_plane",)], out[("no_plane", "no_drone_contact")]
    d_hit = np.linalg.norm(hit[:, 0, 0:3] - hit[:, 1, 0:3], axis=-1)
    d_free = np.linalg.norm(free[:, 0, 0:3] - free[:, 1, 0:3], axis=-1)
    assert d_hit.min() > 0.11 and d_free.min() < 0.02           # stops short / passes through
    # the contact is internal: the pair's summed velocity equals the contact-free run's
    np.testing.assert_allclose(hit[:, 0, 10:13] + hit[:, 1, 10:13], free[:, 0, 10:13] + free[:, 1, 10:13],
                               atol=1e-12)
    assert hit[-1, 0, 10] < 0.0 < hit[-1, 1, 10]                   # pushed apart (ERP)
