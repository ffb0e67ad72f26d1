"""gpd_cmd_rollout: exported, bound, and its host-side argument checks (which run before any
device call, so no GPU is needed)."""
import ctypes
import os
import re

import pytest


@pytest.fixture(scope="module")
def lib():
    from gym_pybullet_drones_routing_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_symbol_exported_and_bound(lib):
    from gym_pybullet_drones_routing_amd import _lib
    out = os.popen(f"nm -D --defined-only {lib._name}").read()
    assert "gpd_cmd_rollout" in _lib.EXPORTED
    assert hasattr(lib, "gpd_cmd_rollout")
    assert lib.gpd_cmd_rollout.argtypes is not None and len(lib.gpd_cmd_rollout.argtypes) == 10
    assert re.search(r"\bT gpd_cmd_rollout\b", out), "gpd_cmd_rollout not exported as a text symbol"
    assert lib.gpd_abi_version() == 7      # additive: no ABI bump


def _call(lib, p, mode=0, n_steps=4, record_every=1, max_steps=0, sim=None):
    return lib.gpd_cmd_rollout(sim, mode, p, n_steps, record_every, None, None, None, max_steps, None)


def test_host_checks_name_the_argument(lib):
    from gym_pybullet_drones_routing_amd import _lib
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for kw, word in ((dict(mode=-1), b"mode"), (dict(mode=3), b"mode"), (dict(n_steps=-1), b"n_steps"),
                     (dict(record_every=0), b"record_every"), (dict(max_steps=-1), b"max_steps_per_launch")):
        assert _call(lib, p, **kw) == _lib.GPD_EINVAL, kw
        msg = lib.gpd_last_error()
        assert b"gpd_cmd_rollout" in msg and word in msg, (kw, msg)
        assert b"NULL sim" not in msg, (kw, msg)          # these run ahead of the sim check
    assert _call(lib, p) == _lib.GPD_EINVAL
    assert b"gpd_cmd_rollout" in lib.gpd_last_error() and b"sim" in lib.gpd_last_error()
    assert _call(lib, p, n_steps=0) == _lib.GPD_EINVAL    # the sim check precedes the n_steps == 0 no-op
    assert b"sim" in lib.gpd_last_error()
