"""step_seq_kernel's rate chains run a step ahead (csrc/gpd_step_seq.h): chain a from the true rates,
chain b from a reset env's zero rates, the pose wave picks per lane behind ONE barrier per step.

Every comparison is bit-equality (torch.equal) between a twin stepped with sim.step and one stepped
with step_seq: outputs, terminal rows, state, counters, and the next single step's observation.  The
cases aim at the choice between the two chains and at the launch's first and last steps."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E_BLOCKS = 17          # a full 16-drone block and a one-lane block
TPB = 16               # drones per block of these sims (lanes_per_block / 4 waves)


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


def _twins(T, E=E_BLOCKS, act="rpm", calls=1, seed=0, scale=1.0, P=None, fused=True, seed_raw=None, out=None,
           **kw):
    """a: calls * T single steps; b: `calls` step_seq calls of T steps each, one straight after the
    other, compared after every call.  Then one more single step on both (the HBM ring).  Returns
    the done flags of every single step of a, [calls * T, E] each (terminated, truncated).
    fused: what gpd_step_seq_plan must say (None: either form).  seed_raw(raw [E, 20]) changes the
    raw state both twins start from; out["raw_end"] gets a's raw state after the last call."""
    from gym_pybullet_drones_routing_amd.enums import ActionType
    rng = np.random.default_rng(seed)
    A = 4 if act == "rpm" else 1
    P = P or T
    pool = _pool(rng, P, E, A, scale)
    extra = _pool(rng, 1, E, A, scale)[0]
    a, b = _sim(n_envs=E, act=ActionType(act), **kw), _sim(n_envs=E, act=ActionType(act), **kw)
    term, trunc = [], []
    try:
        if fused is None:
            assert _plan(b, T) in (-(-T // 256), T)
        else:
            assert _plan(b, T) == (-(-T // 256) if fused else T)
        if out is not None:
            out["plan"] = _plan(b, T)
        if seed_raw is not None:
            raw = a.raw_state().cpu().numpy().reshape(E, 20).copy()
            seed_raw(raw)
            a.set_raw_state(raw)
            b.set_raw_state(raw)
        for _ in range(calls):
            for t in range(T):
                _, _, te, tr = a.step(pool[t % P])
                term.append(te.bool().clone())
                trunc.append(tr.bool().clone())
            b.step_seq(pool, T)
            _assert_twins_equal(a, b)
        if out is not None:
            out["raw_end"] = a.raw_state().cpu().numpy().reshape(E, 20).copy()
        a.step(extra)
        b.step(extra)
        torch.cuda.synchronize()
        assert torch.equal(a.obs, b.obs), "next step's obs (HBM ring)"
        return torch.stack(term).cpu(), torch.stack(trunc).cpu()
    finally:
        a.close()
        b.close()


def _mixed_in_one_block(done, E):
    """Steps after which one 16-drone block holds both a reset lane and a lane that goes on."""
    n = 0
    for t in range(done.shape[0]):
        for b0 in range(0, E, TPB):
            blk = done[t, b0:b0 + TPB]
            n += int(blk.any() and not blk.all())
    return n


@pytest.mark.parametrize("periods", [1, 2])
@pytest.mark.parametrize("T", [2, 3, 4, 9])
def test_whole_block_resets_at_known_steps(periods, T):
    """episode_len_sec of one / two control periods and small actions: every lane is truncated in
    every 3rd / 4th step (the C oracle shows 17 truncations in steps 3, 6, 9, .. and 4, 8, 12, ..
    and none between).  With T = 2, 3, 4, 9 and a second call straight after the first the resets
    fall on a launch's first step, on its last, and inside; the second launch starts from what the
    first left (rates, counters, ring).  The time limit cannot reset a lane in two consecutive
    steps (a reset env's counter starts at zero): test_resets_in_consecutive_steps does that."""
    every = periods + 2
    te, tr = _twins(T, calls=2, seed=20 + T, scale=0.05, episode_len_sec=periods / 30.0)
    want = [E_BLOCKS if (i + 1) % every == 0 else 0 for i in range(2 * T)]
    assert tr.sum(dim=1).tolist() == want
    assert int(te.sum()) == 0


@pytest.mark.parametrize("T", [2, 4])
def test_resets_in_consecutive_steps(T):
    """The start pose lies above the z bound (2.0), so every env is truncated and reset in every
    step: a lane that ran a step on chain b is reset again at its end.  Two calls in a row."""
    te, tr = _twins(T, calls=2, seed=21, scale=0.05, initial_xyzs=np.array([[0.0, 0.0, 2.5]]))
    assert tr.sum(dim=1).tolist() == [E_BLOCKS] * (2 * T)


@pytest.mark.parametrize("E", [17, 96])
def test_mixed_lanes(E):
    """U[-1, 1] actions: envs leave the bounds at different steps, so a block's lanes take chain a
    and chain b in the same step."""
    te, tr = _twins(40, E=E, seed=30 + E, P=7)
    assert _mixed_in_one_block(te | tr, E) >= 1


@pytest.mark.parametrize("episode_len_sec", [8, 2 / 30.0])
def test_mixed_lanes_one_d_rpm(episode_len_sec):
    """The kernel's other instantiation through the mixed-lanes case.  One value for all four
    motors gives no torque, so within 40 steps no env leaves the bounds (measured: no `done` at
    all); the second run has the two-period time limit, which resets every lane on chain b."""
    te, tr = _twins(40, E=17, act="one_d_rpm", seed=31, P=7, episode_len_sec=episode_len_sec)
    if episode_len_sec < 1:
        assert int(tr.sum()) >= 17


def _rising_lanes(raw):
    """Lanes 0, 3, 5, 9 and 16 start just under the z bound (2.0), rising at different speeds."""
    for k, i in enumerate((0, 3, 5, 9, 16)):
        raw[i, 2] = 1.95          # z
        raw[i, 9] = 0.5 + 0.5 * k   # vz


def test_mixed_lanes_one_d_rpm_seeded():
    """ONE_D_RPM with some lanes of the first block about to leave through the z bound at
    different steps, the others staying: chain a and chain b in the same block and step."""
    te, tr = _twins(12, E=17, act="one_d_rpm", seed=37, P=7, seed_raw=_rising_lanes)
    assert _mixed_in_one_block(te | tr, 17) >= 2
    assert int(tr[:, [0, 3, 5, 9, 16]].any(dim=0).sum()) == 5 and int(tr[:, [1, 2, 4]].sum()) == 0


def test_resets_on_both_sides_of_the_launch_boundary():
    """T = 260 with the two-period time limit: two launches (256 + 4 steps), every lane reset in
    every 4th step, the last of them step 256 - the first launch's last."""
    T = 260
    te, tr = _twins(T, seed=32, scale=0.05, P=13, episode_len_sec=2 / 30.0)
    assert tr.sum(dim=1).tolist() == [E_BLOCKS if (i + 1) % 4 == 0 else 0 for i in range(T)]


def test_no_autoreset_keeps_chain_a():
    """Finished envs are not reset: their rates go on from chain a although `done` is set."""
    te, tr = _twins(40, seed=33, P=7, autoreset=False)
    assert int((te | tr).sum()) >= 1


@pytest.mark.parametrize("pyb_freq", [30, 60])
def test_longest_substeps_with_full_scale_actions(pyb_freq):
    """nsub = 1 and 2 with full-scale actions, T = 10.  From rest these actions turn a drone by
    well under 0.5 rad per half substep, so this does NOT reach the weights' large-angle branch;
    test_large_angle_weights_on_chain_a does."""
    te, tr = _twins(10, seed=34, P=7, pyb_freq=pyb_freq, ctrl_freq=30)
    assert int((te | tr).sum()) >= 1


def _spinning(pyb_freq):
    def seed(raw):
        # |w| = 1.68 * pyb_freq rad/s: half a substep turns 0.84 rad, past the branch at 0.5
        raw[:, 10:13] = np.array([1.3, -1.0, 0.4]) * pyb_freq * np.linspace(1.0, 1.2, raw.shape[0])[:, None]
    return seed


@pytest.mark.parametrize("autoreset", [False, True])
@pytest.mark.parametrize("pyb_freq", [30, 60])
def test_large_angle_weights_on_chain_a(pyb_freq, autoreset):
    """Both twins start with body rates of 1.68 x pyb_freq rad/s and more, so |w| dt / 2 >= 0.84 rad:
    rate_weights_big's rows go through the hand-off buffer, in the chain computed in front of the
    entry barrier and, with autoreset off (the rates go on, the envs only flagged), in every later
    step: the rates at the end are still past the threshold.  With autoreset on the spinning envs
    tilt, are reset and go on from chain b.  Chain b itself starts every step from zero rates and
    cannot reach the branch within one step; only chain a can."""
    out = {}
    te, tr = _twins(10, seed=38, P=7, pyb_freq=pyb_freq, ctrl_freq=30, autoreset=autoreset,
                    seed_raw=_spinning(pyb_freq), out=out)
    assert int(tr.sum()) >= E_BLOCKS     # every env tilts past the limit
    if not autoreset:
        w = np.linalg.norm(out["raw_end"][:, 10:13], axis=1)
        assert (w * (1.0 / pyb_freq) / 2 >= 0.5).all(), w


def test_sixteen_substeps_in_full_blocks():
    """nsub = 16 with 64-drone blocks.  Whatever the host decides, gpd_step_seq_plan is one of the
    two forms and the twins are equal on it.  By the buffers' arithmetic (2 parities x 2 chains x
    ((5 nsub + 3) | 1) rows x 64 lanes x 8 B = 169 984 B, alone past the 163 840 B of a workgroup's
    LDS) it is the per-step loop; a layout that fits may fuse it."""
    T, nsub, tpb = 6, 16, 64
    out = {}
    _twins(T, E=96, seed=35, P=7, fused=None, out=out, pyb_freq=480, ctrl_freq=30,
           tuning=dict(step_waves=3, drones_per_block=tpb))
    if 2 * 2 * ((5 * nsub + 3) | 1) * tpb * 8 > 160 * 1024:
        assert out["plan"] == T


def test_sixteen_substeps_in_thin_blocks_stay_fused():
    """nsub = 16 at 16 drones per block (42 496 B of hand-off buffers) is one fused launch."""
    _twins(6, seed=36, P=7, pyb_freq=480, ctrl_freq=30)
