"""gpd_cmd_step / gpd_adjacency: exported, bound, and their host-side argument checks (which run
before any device call, so no GPU is needed)."""
import ctypes
import os
import re

import pytest


@pytest.fixture(scope="module")
def lib():
    from gym_pybullet_drones_routing_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    from gym_pybullet_drones_routing_amd import _lib
    out = os.popen(f"nm -D --defined-only {lib._name}").read()
    for name in ("gpd_cmd_step", "gpd_adjacency"):
        assert name in _lib.EXPORTED
        assert hasattr(lib, name), name
        assert re.search(rf"\bT {name}\b", out), f"{name} not exported as a text symbol"
    assert (_lib.GPD_CMD_RPM, _lib.GPD_CMD_VEL, _lib.GPD_CMD_WAYPOINT) == (0, 1, 2)
    assert lib.gpd_abi_version() == 7      # additive: no ABI bump


def test_host_checks_name_the_argument(lib):
    from gym_pybullet_drones_routing_amd import _lib
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.gpd_cmd_step(None, _lib.GPD_CMD_RPM, p, None, None) == _lib.GPD_EINVAL
    assert b"gpd_cmd_step" in lib.gpd_last_error() and b"sim" in lib.gpd_last_error()
    for mode in (-1, 3, 99):
        assert lib.gpd_cmd_step(None, mode, p, None, None) == _lib.GPD_EINVAL
        assert b"gpd_cmd_step" in lib.gpd_last_error() and b"mode" in lib.gpd_last_error()
    assert lib.gpd_adjacency(None, 1.0, p, None) == _lib.GPD_EINVAL
    assert b"gpd_adjacency" in lib.gpd_last_error() and b"sim" in lib.gpd_last_error()
