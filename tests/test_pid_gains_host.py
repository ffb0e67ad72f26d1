"""Per-drone controller gains (gpd_set_pid_gains), the parts that need no GPU: the pure row
builder ``sim.pid_gain_rows``, the host-only argument checks of the two entry points, and the
conditions that make the GPU tests' flights (tests/pid_gains_flights.py) meaningful, checked on
the CPU reference alone: with the recipe's gains the reference stays finite and upright, and each
flight separates from the same flight on the default gains by far more than the parity gate, so
a kernel that ignored the table could not pass.
"""
import ctypes

import numpy as np
import pytest

from tests.oracle_runs import state_rel_err
from tests.pid_gains_flights import DEFAULT, FLIGHTS, default_rows, gain_rows, reference

KEYS = ("p_coeff_pos", "i_coeff_pos", "d_coeff_pos", "p_coeff_att", "i_coeff_att", "d_coeff_att")


def _rows(*a, **kw):
    from gym_pybullet_drones_routing_amd.sim import pid_gain_rows
    return pid_gain_rows(*a, **kw)


@pytest.fixture(scope="module")
def lib():
    from gym_pybullet_drones_routing_amd import _build, _lib
    _build.build()
    return _lib.load()


# ------------------------------------------------------------------ pid_gain_rows
def test_rows_from_pid_params_are_the_defaults(lib):
    from gym_pybullet_drones_routing_amd import _lib
    from gym_pybullet_drones_routing_amd.sim import PID_GAIN_KEYWORDS
    assert PID_GAIN_KEYWORDS == KEYS
    q = _lib.default_pid_params()
    rows = _rows(4, 3, q)
    assert rows.shape == (12, 18) and rows.dtype == np.float64 and rows.flags.c_contiguous
    np.testing.assert_array_equal(rows, default_rows(12))
    q.i_coeff_tor[0] = 7.0
    assert _rows(1, 1, q)[0, 12] == 7.0


def test_rows_broadcasting_and_none_keeps_the_base():
    E, D = 4, 3
    base = gain_rows(1, E * D)
    np.testing.assert_array_equal(_rows(E, D, base), base)
    np.testing.assert_array_equal(_rows(E, D, base, **{k: None for k in KEYS}), base)
    rng = np.random.default_rng(2)
    shapes = {"p_coeff_pos": (3,), "d_coeff_pos": (E, 3), "i_coeff_att": (E, 1, 3), "d_coeff_att": (E, D, 3)}
    vals = {k: rng.uniform(1, 2, s) for k, s in shapes.items()}
    got = _rows(E, D, base, **vals).reshape(E, D, 6, 3)
    want = base.reshape(E, D, 6, 3).copy()
    want[:, :, 0] = vals["p_coeff_pos"]
    want[:, :, 2] = vals["d_coeff_pos"][:, None, :]
    want[:, :, 4] = vals["i_coeff_att"]
    want[:, :, 5] = vals["d_coeff_att"]
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[:, :, [1, 3]], base.reshape(E, D, 6, 3)[:, :, [1, 3]])   # untouched triples
    # a list, and E == 3 where (3,) is still one triple for everybody
    np.testing.assert_array_equal(_rows(3, 2, default_rows(6), p_coeff_att=[1, 2, 3])[:, 9:12],
                                  np.tile([1.0, 2.0, 3.0], (6, 1)))
    assert not np.shares_memory(_rows(E, D, base), base)


@pytest.mark.parametrize("shape", [(2,), (4,), (3, 3), (5, 3), (4, 2, 3), (4, 3, 1), (1, 3), (3, 4), (4, 3, 3, 1), ()])
def test_rows_shape_errors(shape):
    E, D = 4, 3
    with pytest.raises(ValueError, match="shape"):
        _rows(E, D, default_rows(E * D), p_coeff_pos=np.ones(shape))


def test_rows_other_errors():
    E, D = 2, 2
    base = default_rows(E * D)
    for bad in (np.ones((E * D, 17)), np.ones((E * D + 1, 18)), np.ones(18)):
        with pytest.raises(ValueError, match="base"):
            _rows(E, D, bad)
    with pytest.raises(ValueError, match="unknown"):
        _rows(E, D, base, p_coeff=np.ones(3))
    for v in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="non-finite gain in row 3, column 7"):
            _rows(E, D, base, d_coeff_pos=np.array([[[1, 1, 1], [1, 1, 1]], [[1, 1, 1], [1, v, 1]]]))
        bad = base.copy()
        bad[1, 17] = v
        with pytest.raises(ValueError, match="row 1, column 17"):
            _rows(E, D, bad)


# ------------------------------------------------------------------ host-only entry points
def test_entry_points_refuse_a_null_sim(lib):
    from gym_pybullet_drones_routing_amd import _lib
    buf = (ctypes.c_double * 18)()
    assert lib.gpd_set_pid_gains(None, buf) == _lib.GPD_EINVAL
    assert b"gpd_set_pid_gains" in lib.gpd_last_error()
    assert lib.gpd_set_pid_gains(None, None) == _lib.GPD_EINVAL
    assert lib.gpd_get_pid_gains(None, buf) == _lib.GPD_EINVAL
    assert b"gpd_get_pid_gains" in lib.gpd_last_error()


# ------------------------------------------------------------------ the flights' conditions, on the oracle
def test_recipe():
    g = gain_rows(5, 9).reshape(9, 6, 3)
    ratio = np.delete(g.reshape(9, 18), [12, 13], axis=1) / np.delete(DEFAULT.reshape(18), [12, 13])
    assert ratio.min() >= 0.5 and ratio.max() <= 1.5 and len(np.unique(ratio)) == ratio.size
    assert g[:, 4, 0:2].min() > 0 and g[:, 4, 0:2].max() <= 100
    np.testing.assert_array_equal(gain_rows(5, 9), g.reshape(9, 18))      # deterministic
    assert not np.array_equal(gain_rows(6, 9), gain_rows(5, 9))


@pytest.mark.parametrize("name", list(FLIGHTS))
def test_flight_is_finite_and_upright(name):
    traj = reference(name)["traj"]
    assert np.isfinite(traj).all() and np.isfinite(reference(name)["ctrl"]).all()
    tilt = np.abs(traj[..., 7:9]).max()
    print(f"\n[pid_gains] {name}: largest |roll|, |pitch| {tilt:.3f}")
    assert tilt < 0.4, tilt


@pytest.mark.parametrize("name,bound", [("wp3x3", 1e-2), ("wp2x65", 1e-4), ("vel5x2", 1e-3)])
def test_flight_separates_from_the_default_gains(name, bound):
    sep = state_rel_err(reference(name)["traj"][-1], reference(name, tuned=False)["traj"][-1])
    print(f"\n[pid_gains] {name}: separation from the default gains min {sep.min():.3e} max {sep.max():.3e}")
    if name == "vel5x2":
        # (env 0, drone 0): a zero command from rest; gains cannot move it
        assert sep[0] == 0.0
        sep = sep[1:]
    assert sep.min() >= bound, sep.min()


def test_same_flight_different_gains_end_apart():
    """70 envs, one start, one waypoint sequence: only the gains differ, and every pair of final
    positions is at least 1e-6 apart (so a permutation of the rows is visible in the result)."""
    pos = reference("wp70x1")["traj"][-1][:, 0:3]
    d = np.linalg.norm(pos[:, None, :] - pos[None, :, :], axis=-1)
    d[np.diag_indices_from(d)] = np.inf
    print(f"\n[pid_gains] wp70x1: smallest distance between two final positions {d.min():.3e}")
    assert d.min() >= 1e-6, d.min()
