"""The fused open-loop sequence (step_seq_kernel, csrc/gpd_step_seq.h): gpd_step_seq and a replayed
capture_graph on the sims of the three-wave step kernel run T steps in one launch per 256 steps.

Every comparison is bit-equality (torch.equal) between a sim stepped with sim.step - the per-step
kernel, pinned to the oracle by tests/test_gpu_parity.py - and a twin stepped with step_seq or a
replayed graph: outputs, terminal rows, state, counters, and the next single step's observation,
which shows the action ring in HBM."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

L = 15   # ACTION_BUFFER_SIZE at ctrl_freq 30


def _sim(**kw):
    from gym_pybullet_drones_routing_amd.sim import BatchedAviarySim
    kw.setdefault("task", "hover")
    kw.setdefault("precision", "f64")
    return BatchedAviarySim(device="cuda:0", **kw)


def _pool(rng, P, E, A, scale=1.0):
    return torch.from_numpy((rng.uniform(-1, 1, (P, E, 1, A)) * scale).astype(np.float32)).cuda()


def _plan(sim, n_steps):
    return sim._lib.gpd_step_seq_plan(sim._h, int(n_steps))


def _assert_twins_equal(a, b, terminal_obs=True):
    torch.cuda.synchronize()
    pairs = [("obs", a.obs, b.obs), ("reward", a.reward, b.reward), ("terminated", a.terminated, b.terminated),
             ("truncated", a.truncated, b.truncated), ("raw_state", a.raw_state(), b.raw_state()),
             ("step_counters", a.step_counters(), b.step_counters())]
    if terminal_obs:
        pairs.append(("terminal_obs", a.terminal_obs, b.terminal_obs))
    for name, x, y in pairs:
        assert torch.equal(x, y), name


def _compare(T, P, E=17, act="rpm", lead=0, seed=0, terminal_obs=True, scale=1.0, fused=True, **kw):
    """a: lead + T single steps; b: lead single steps, then step_seq(pool, T).  Then one more single
    step on both: its history columns are the HBM ring's.  Returns the envs a reset in each of the T
    steps (terminated or truncated), [T, E]."""
    from gym_pybullet_drones_routing_amd.enums import ActionType
    rng = np.random.default_rng(seed)
    A = 4 if act == "rpm" else 1
    pool = _pool(rng, P, E, A, scale)
    pre = _pool(rng, max(lead, 1), E, A, scale)
    a, b = _sim(n_envs=E, act=ActionType(act), **kw), _sim(n_envs=E, act=ActionType(act), **kw)
    try:
        if fused:   # the fused path is the one under test
            assert _plan(b, T) == -(-T // 256)
        for k in range(lead):
            a.step(pre[k], terminal_obs=terminal_obs)
            b.step(pre[k], terminal_obs=terminal_obs)
        done = []
        for t in range(T):
            _, _, te, tr = a.step(pool[t % P], terminal_obs=terminal_obs)
            done.append(te.bool() | tr.bool())
        b.step_seq(pool, T, terminal_obs=terminal_obs)
        _assert_twins_equal(a, b, terminal_obs)
        a.step(pre[0])
        b.step(pre[0])
        torch.cuda.synchronize()
        assert torch.equal(a.obs, b.obs), "next step's obs (HBM ring)"
        return torch.stack(done).cpu()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("E", [1, 17, 96])
@pytest.mark.parametrize("T", [2, 14, 15, 16, 40])
def test_fused_matches_single_steps(E, T):
    """One lane, a partial second block, several blocks; the ring (L = 15) does not wrap, wraps
    exactly, wraps past.  U[-1, 1] actions: envs leave the bounds and reset on the way at T = 40."""
    _compare(T, 7, E=E, seed=100 * E + T)


@pytest.mark.parametrize("act", ["rpm", "one_d_rpm"])
@pytest.mark.parametrize("P", [1, 7])
def test_fused_action_types_and_slot_counts(act, P):
    _compare(40, P, E=17, act=act, seed=3)


@pytest.mark.parametrize("kw", [dict(autoreset=False), dict(terminal_obs=False), dict(task="none"),
                                dict(autoreset=False, act="one_d_rpm"), dict(terminal_obs=False, act="one_d_rpm")],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_fused_options(kw):
    _compare(40, 7, E=17, seed=4, **kw)


@pytest.mark.parametrize("T", [5, 16, 40])
def test_fused_from_a_partly_filled_ring(T):
    """The twin starts after 3 single steps: head != 0 and the ring holds 3 actions."""
    _compare(T, 7, E=17, lead=3, seed=5)


@pytest.mark.parametrize("pyb_freq", [30, 60, 240, 480])
def test_fused_substep_counts(pyb_freq):
    """nsub = 1 (no look-ahead in the rate wave), 2, 8, 16."""
    _compare(5, 7, E=17, seed=6, pyb_freq=pyb_freq, ctrl_freq=30)


@pytest.mark.parametrize("tuning", [dict(store_policy=1), dict(store_policy=4), dict(drones_per_block=64)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_fused_store_policies_and_full_blocks(tuning):
    """Plain and write-through row / state stores; 64-drone blocks, whose history columns take
    more than one pass of the io wave."""
    _compare(20, 7, E=96, seed=7, tuning=dict(step_waves=3, **tuning))


@pytest.mark.parametrize("store_policy", [1, 2], ids=["plain", "write-through"])
@pytest.mark.parametrize("drones_per_block", [16, 64])
@pytest.mark.parametrize("act", ["rpm", "one_d_rpm"])
def test_fused_io_wave_passes(act, drones_per_block, store_policy):
    """The io wave's store pass and terminal-row pass (csrc/gpd_step_seq.h, wave 2) in each of
    their forms: float4 and float elements; 16-drone blocks, whose
    16 * 15 elements fit one pass from registers, and 64-drone blocks, which take several from the
    tile; plain and write-through rows.  A time limit of one control period and small actions
    truncate every env in the third of the four steps (test_gpu_step_seq_ahead.py), so every block
    writes terminal rows inside the launch and runs a step behind the reset."""
    done = _compare(4, 4, E=96, act=act, seed=14, scale=0.05, episode_len_sec=1 / 30.0,
                    tuning=dict(step_waves=3, drones_per_block=drones_per_block, store_policy=store_policy))
    assert done.sum(dim=1).tolist() == [0, 0, 96, 0]


def test_fused_long_sequence_crosses_launch_and_time_limit():
    """T = 300 crosses the 256-step launch boundary and the time limit (8 s at 30 Hz: an env that
    stays inside the bounds is truncated in its 242nd step).  U[-1, 1] actions; the first four envs
    get one U[-1, 1] value for all four motors (no torque), because no env with four independent
    random motors lives that long: over 400 seeds x 16 envs the C oracle's longest such episode is
    66 steps.  With seed 11 the oracle shows three of the four reaching the time limit; the other
    twelve leave the bounds early and reset some twenty times each on the way."""
    from gym_pybullet_drones_routing_amd.enums import ActionType
    E, T, P, LIMIT = 16, 300, 64, 242
    rng = np.random.default_rng(11)
    pool = _pool(rng, P, E, 4)
    pool[:, :4] = pool[:, :4, :, :1].clone()
    a, b = _sim(n_envs=E, act=ActionType.RPM), _sim(n_envs=E, act=ActionType.RPM)
    try:
        assert _plan(b, T) == 2
        by_time, early = 0, 0
        age = torch.zeros(E, dtype=torch.int64, device="cuda")
        for t in range(T):
            _, _, te, tr = a.step(pool[t % P])
            age += 1
            done = (te | tr).bool()
            by_time += int((tr.bool() & (age == LIMIT)).sum().item())
            early += int((done & (age < LIMIT)).sum().item())
            age[done] = 0
        b.step_seq(pool, T)
        assert by_time >= 1, "no env reached the time limit"
        assert early >= 1, "no env ended before the time limit"
        _assert_twins_equal(a, b)
        a.step(pool[0])
        b.step(pool[0])
        torch.cuda.synchronize()
        assert torch.equal(a.obs, b.obs)
    finally:
        a.close()
        b.close()


def test_plan_counts_launches():
    """gpd_step_seq_plan: the fused path is taken where it should be, and only there."""
    s = _sim(n_envs=64)
    assert s.constants.action_buffer_size == L and s.constants.lanes_per_block == 192
    assert (_plan(s, 40), _plan(s, 300), _plan(s, 256), _plan(s, 257), _plan(s, 1), _plan(s, 0)) == (1, 2, 1, 2, 1, 0)
    assert s._lib.gpd_step_seq_plan(None, 5) < 0
    s.close()
    two = _sim(n_envs=64, tuning=dict(step_waves=2))
    assert (_plan(two, 40), _plan(two, 300)) == (40, 300)
    two.close()
    het = _sim(n_envs=64, env_params={"m": np.full(64, 0.027)})
    assert (_plan(het, 40), _plan(het, 300)) == (40, 300)
    het.close()


def test_per_step_sims_keep_their_loop():
    """A two-wave sim's step_seq is still the per-step loop, and still equals single steps."""
    _compare(20, 7, E=96, seed=8, fused=False, tuning=dict(step_waves=2))


def test_graph_of_a_cycled_pool_replayed_twice():
    """capture_graph([pool[k % 7] for k in range(20)]) is one fused launch; two replays equal 40
    single steps."""
    E, P, K = 17, 7, 20
    rng = np.random.default_rng(12)
    pool = _pool(rng, P, E, 4)
    a, b = _sim(n_envs=E), _sim(n_envs=E)
    try:
        g = b.capture_graph([pool[k % P] for k in range(K)])
        for rep in range(2):
            for k in range(K):
                a.step(pool[k % P])
            g.replay()
        _assert_twins_equal(a, b)
        a.step(pool[0])
        b.step(pool[0])
        torch.cuda.synchronize()
        assert torch.equal(a.obs, b.obs)
    finally:
        a.close()
        b.close()


def test_graph_of_mixed_tensors():
    """A contiguous run, a stray tensor and a repeated tensor in one graph: a fused segment, a plain
    step and a one-slot segment."""
    E = 17
    rng = np.random.default_rng(13)
    pool = _pool(rng, 5, E, 4)
    stray = _pool(rng, 1, E, 4)[0]
    seq = [pool[0], pool[1], pool[2], stray, pool[4], pool[4], pool[4]]
    a, b = _sim(n_envs=E), _sim(n_envs=E)
    try:
        g = b.capture_graph(seq)
        for x in seq:
            a.step(x)
        g.replay()
        _assert_twins_equal(a, b)
    finally:
        a.close()
        b.close()


def test_fused_matches_oracle():
    """E = 64, T = 40 with the action mix of bench.state_parity (small actions, an eighth of the
    envs on U[-1, 1], which forces resets): the state after the fused sequence against the C fp64
    restatement of BaseAviary.step, under the project's f64 gate."""
    from oracle.c_oracle import COracle
    from tests.oracle_runs import state_rel_err
    E, T = 64, 40
    rng = np.random.default_rng(0)
    acts = np.clip(rng.normal(0, 0.1, (T, E, 1, 4)), -1, 1).astype(np.float32)
    acts[:, : E // 8] = rng.uniform(-1, 1, (T, E // 8, 1, 4)).astype(np.float32)
    sim = _sim(n_envs=E)
    orc = COracle(n_envs=E, task="hover", act="rpm")
    try:
        assert _plan(sim, T) == 1
        sim.step_seq(torch.from_numpy(acts).cuda(), T)
        for t in range(T):
            orc.step(acts[t])
        err = state_rel_err(sim.state20().cpu().numpy(), orc.state20())
        print("fused vs C oracle: state rel L2 max", err.max())
        assert err.max() <= 1e-10
    finally:
        sim.close()
        orc.close()


def test_f32_step_seq_matches_single_steps():
    """f32 sims: the same bit-equality, on whichever path gpd_step_seq takes for them."""
    _compare(40, 7, E=96, seed=9, precision="f32", fused=False)
