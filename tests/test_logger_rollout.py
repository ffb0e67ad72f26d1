"""Logger.log_rollout leaves the logger exactly as the log_batch loop over the same rows does."""
import numpy as np
import pytest
import torch

from gym_pybullet_drones_routing_amd.logger import Logger

D, T = 3, 7


def _rows(seed, t):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(t, D, 20)), rng.normal(size=(t, D, 12))


def _same(a, b):
    np.testing.assert_array_equal(a.timestamps, b.timestamps)
    np.testing.assert_array_equal(a.states, b.states)
    np.testing.assert_array_equal(a.controls, b.controls)
    np.testing.assert_array_equal(a.counters, b.counters)


def _pair(tmp_path, **kw):
    kw.setdefault("logging_freq_hz", 48)
    return (Logger(num_drones=D, output_folder=str(tmp_path / "a"), device="cpu", **kw),
            Logger(num_drones=D, output_folder=str(tmp_path / "b"), device="cpu", **kw))


# duration 0: not preallocated, capacity 16; the small durations preallocate fewer rows than T = 7 (and
# than the 2 + 7 rows of the second test), so the rows run past the logical width, and 40 rows in
# test_after_log_batch_calls also past the capacity
@pytest.mark.parametrize("duration_sec", [0, 3 / 48, 0.25])
@pytest.mark.parametrize("with_controls", [True, False])
def test_matches_log_batch_loop(tmp_path, duration_sec, with_controls):
    a, b = _pair(tmp_path, duration_sec=duration_sec)
    st, ct = _rows(0, T)
    t0, dt = 0.125, 1.0 / 48
    for k in range(T):
        a.log_batch(t0 + k * dt, st[k], ct[k] if with_controls else None)
    b.log_rollout(t0, dt, torch.from_numpy(st), torch.from_numpy(ct) if with_controls else None)
    assert a.timestamps.shape == (D, max(T, int(duration_sec * 48)))
    _same(a, b)


@pytest.mark.parametrize("duration_sec,t", [(0, T), (3 / 48, T), (0.25, T), (0, 40)])
def test_after_log_batch_calls(tmp_path, duration_sec, t):
    a, b = _pair(tmp_path, duration_sec=duration_sec)
    st0, ct0 = _rows(1, 2)
    st, ct = _rows(2, t)
    for lg in (a, b):
        lg.log_batch(0.0, st0[0], ct0[0])
        lg.log_batch(0.5, st0[1])
    for k in range(t):
        a.log_batch(1.0 + k * 0.25, st[k], ct[k])
    b.log_rollout(1.0, 0.25, st, ct)
    assert a.timestamps.shape[1] >= 2 + t
    if t == 40:
        assert b._ts.shape[0] >= 42 > 16       # the capacity was outgrown, in one step
    _same(a, b)
    a.log_batch(99.0, st[0])                   # and the logger goes on as usual afterwards
    b.log_batch(99.0, st[0])
    _same(a, b)
