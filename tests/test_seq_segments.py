"""sim.seq_segments: how capture_graph splits a list of action tensors into gpd_step_seq calls.
A pure function of the tensors' addresses and the bytes of one action slot; no device."""
import pytest

from gym_pybullet_drones_routing_amd.sim import seq_segments

S = 4096 * 4 * 4          # one slot of 4096 single-drone envs, RPM actions
B = 0x7F0000000000        # a device address


def _expand(segments, slot_bytes):
    """The addresses a list of segments reads, step by step."""
    return [base + (k % n_slots) * slot_bytes for base, n_slots, n_steps in segments for k in range(n_steps)]


def test_periodic_pool_is_one_segment():
    ptrs = [B + (k % 64) * S for k in range(256)]
    assert seq_segments(ptrs, S) == [(B, 64, 256)]
    # a pool that the sequence does not go round completely
    assert seq_segments([B + k * S for k in range(44)], S) == [(B, 44, 44)]
    # ... or leaves in the middle of a round
    assert seq_segments([B + (k % 7) * S for k in range(20)], S) == [(B, 7, 20)]


def test_one_repeated_tensor_is_one_slot():
    assert seq_segments([B] * 5, S) == [(B, 1, 5)]


def test_unrelated_pointers_are_one_step_each():
    ptrs = [B, B + 3 * S, B + S + 16, B - S]
    assert seq_segments(ptrs, S) == [(p, 1, 1) for p in ptrs]


def test_contiguous_run_then_a_stray_tensor():
    stray = B + 100 * S
    assert seq_segments([B, B + S, B + 2 * S, stray], S) == [(B, 3, 3), (stray, 1, 1)]
    # a stray tensor in the middle of a periodic run ends it; what follows starts a new run
    ptrs = [B, B + S, B, B + S, stray, B + S, B + 2 * S]
    assert seq_segments(ptrs, S) == [(B, 2, 4), (stray, 1, 1), (B + S, 2, 2)]


def test_list_of_one_and_empty_list():
    assert seq_segments([B], S) == [(B, 1, 1)]
    assert seq_segments([], S) == []


def test_a_pool_left_before_its_end_is_not_continued_past_the_wrap():
    # 0 1 2 0 1 2 3: the return to the base fixes three slots, so slot 3 starts a new run
    ptrs = [B, B + S, B + 2 * S, B, B + S, B + 2 * S, B + 3 * S]
    assert seq_segments(ptrs, S) == [(B, 3, 6), (B + 3 * S, 1, 1)]


@pytest.mark.parametrize("ptrs", [
    [B + (k % 64) * S for k in range(300)],
    [B, B, B + S, B + S, B, B + 2 * S, B + 3 * S, B + 2 * S],
    [B + (k * k % 5) * S for k in range(40)],
])
def test_segments_cover_the_sequence_in_order(ptrs):
    segs = seq_segments(ptrs, S)
    assert _expand(segs, S) == ptrs
    assert all(1 <= n_slots <= n_steps for _, n_slots, n_steps in segs)
