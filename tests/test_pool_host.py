"""Reset pools, host side (no GPU): the draw's C export against its Python restatements, the
argument checks that run before any device call, and learn.py's --randomize restriction."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import pool_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from gym_pybullet_drones_routing_amd import _build, _lib
    _build.build()
    return _lib.load()


def test_c_draw_equals_python_draw(lib):
    from gym_pybullet_drones_routing_amd.sim import reset_pool_draw
    rng = np.random.default_rng(0)
    N = 20000
    seeds = rng.integers(0, 2**32, N)
    streams = rng.integers(1, 3, N)
    envs = rng.integers(0, 2**31, N)
    eps = rng.integers(0, 2**31 - 1, N)
    ns = rng.integers(1, 2**20 + 1, N)
    ns[:100] = 2**20
    for seed, stream, e, k, n in zip(seeds.tolist(), streams.tolist(), envs.tolist(), eps.tolist(), ns.tolist()):
        got = lib.gpd_reset_pool_draw(seed, stream, e, k, n)
        assert 0 <= got < n
        assert got == pool_ref.draw(seed, stream, e, k, n), (seed, stream, e, k, n)
        assert got == reset_pool_draw(seed, stream, e, k, n)


@pytest.mark.parametrize("seed", [0, 0xffffffff, 7])
def test_draw_edges(lib, seed):
    for stream in (1, 2):
        for e in (0, 1, 69, 4095):
            for k in (1, 2, 1000):
                assert lib.gpd_reset_pool_draw(seed, stream, e, k, 1) == 0      # n = 1: always 0
                for n in (2, 5, 7, 2**20):
                    got = lib.gpd_reset_pool_draw(seed, stream, e, k, n)
                    assert 0 <= got < n and got == pool_ref.draw(seed, stream, e, k, n)
    # the two streams and consecutive episodes are different sequences
    a = [pool_ref.draw(seed, 1, 3, k, 2**20) for k in range(1, 9)]
    b = [pool_ref.draw(seed, 2, 3, k, 2**20) for k in range(1, 9)]
    assert a != b and len(set(a)) == 8


def test_draw_spread(lib):
    """seed 7, stream 1, 4096 envs x episodes 1..8 into 16 bins: every bin within +-10 % of 2048
    (a condition the hash meets with room: a binomial bin's standard deviation is 44, so the bound
    is 4.6 sigma; a hash that ignored the env or the episode would put whole blocks in one bin)."""
    bins = np.zeros(16, dtype=np.int64)
    for e in range(4096):
        for k in range(1, 9):
            bins[lib.gpd_reset_pool_draw(7, 1, e, k, 16)] += 1
    print(f"\n[pool] spread: bins {bins.min()}..{bins.max()}")
    assert bins.sum() == 4096 * 8
    assert (np.abs(bins - 2048) <= 204.8).all()


def test_null_sim_is_einval(lib):
    from gym_pybullet_drones_routing_amd import _lib
    rows = np.ones((2, 11))
    xyz = np.zeros((2, 1, 3))
    out = np.zeros((4, 18))
    assert lib.gpd_set_reset_pool(None, rows.ctypes.data_as(ctypes.c_void_p), 2, xyz.ctypes.data_as(ctypes.c_void_p),
                                  None, 2, 0) == _lib.GPD_EINVAL
    assert b"gpd_set_reset_pool" in lib.gpd_last_error()
    assert lib.gpd_get_reset_draws(None, None, None) == _lib.GPD_EINVAL
    assert lib.gpd_get_env_table(None, out.ctypes.data_as(ctypes.c_void_p)) == _lib.GPD_EINVAL


@pytest.mark.parametrize("extra", [["--physics", "pyb"], ["--physics", "dyn", "--gpus", "2"]])
def test_learn_randomize_names_its_restriction(extra):
    """--randomize outside Physics.DYN on one GPU exits before any GPU call (this suite has no GPU:
    a GPU call would fail with another message)."""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "learn.py"), "--randomize", "0.1"] + extra,
                         capture_output=True, text=True, timeout=120,
                         env={**os.environ, "HIP_VISIBLE_DEVICES": "", "CUDA_VISIBLE_DEVICES": ""})
    assert res.returncode != 0
    assert "--randomize needs --physics dyn and --gpus 1" in res.stderr
