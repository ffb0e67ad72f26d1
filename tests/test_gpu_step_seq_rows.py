"""step_seq_kernel's io wave makes the observation rows, and its pose wave takes the thrust from the
rate chains (csrc/gpd_step_seq.h).

The pose wave publishes per lane what a row is made of (f64 position, velocity, ang_v, the Euler
arguments, the reward) and its terminated / truncated masks; behind the step's barrier lane i of the
io wave makes row i: the float32 angles with the gimbal fix-up, the terminal row and the template's
row of a reset lane, reward and flags.  Each rate chain publishes rpm_wrench's fz with its rows.

Every comparison is bit-equality (torch.equal) between a twin stepped with sim.step and one stepped
with step_seq: outputs, terminal rows, raw state, counters, and the next single step's observation.
Each case also asserts its input pattern on the sim.step twin, so that it cannot pass without
reaching the branch it is about.  17 envs: a full 16-drone block and a one-lane block."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E = 17
TPB = 16
HALF_PI = float(np.float32(np.pi / 2))
ACTS = ["rpm", "one_d_rpm"]


def _sim(act, **kw):
    from gym_pybullet_drones_routing_amd.enums import ActionType
    from gym_pybullet_drones_routing_amd.sim import BatchedAviarySim
    kw.setdefault("task", "hover")
    return BatchedAviarySim(n_envs=E, act=ActionType(act), precision="f64", device="cuda:0", **kw)


def _assert_twins_equal(a, b, terminal_obs):
    torch.cuda.synchronize()
    pairs = [("obs", a.obs, b.obs), ("reward", a.reward, b.reward), ("terminated", a.terminated, b.terminated),
             ("truncated", a.truncated, b.truncated), ("raw_state", a.raw_state(), b.raw_state()),
             ("step_counters", a.step_counters(), b.step_counters())]
    if terminal_obs:
        pairs.append(("terminal_obs", a.terminal_obs, b.terminal_obs))
    for name, x, y in pairs:
        assert torch.equal(x, y), name


def _twins(T, act, pool, seed_raw, calls=1, terminal_obs=True, each_step=None, out=None, launches=1, **kw):
    """a: calls * T single steps; b: `calls` fused step_seq calls of T steps, compared after every
    call; then one more single step on both (the HBM ring).  pool [P, E, 1, A] on the device; step
    t of a call reads pool[t % P].  each_step(i, a, tmpl) sees twin a after its i-th single step
    (tmpl: the template row's state columns [E, 12]).  Returns a's truncated flags [calls * T, E]."""
    P = pool.shape[0]
    a, b = _sim(act, **kw), _sim(act, **kw)
    trunc = []
    try:
        assert b._lib.gpd_step_seq_plan(b._h, int(T)) == launches, "fused: one launch per 256 steps"
        tmpl = a.reset().clone()[:, 0, :12]
        b.reset()
        raw = a.raw_state().cpu().numpy().reshape(E, 20).copy()
        seed_raw(raw)
        a.set_raw_state(raw)
        b.set_raw_state(raw)
        for c in range(calls):
            for t in range(T):
                _, _, _, tr = a.step(pool[t % P], terminal_obs=terminal_obs)
                trunc.append(tr.bool().clone())
                if each_step is not None:
                    torch.cuda.synchronize()
                    each_step(c * T + t, a, tmpl)
            b.step_seq(pool, T, terminal_obs=terminal_obs)
            _assert_twins_equal(a, b, terminal_obs)
        if out is not None:
            out["raw_end"] = a.raw_state().cpu().numpy().reshape(E, 20).copy()
        extra = pool[P - 1].clone()
        a.step(extra)
        b.step(extra)
        torch.cuda.synchronize()
        assert torch.equal(a.obs, b.obs), "next step's obs (HBM ring)"
        return torch.stack(trunc).cpu()
    finally:
        a.close()
        b.close()


def _width(act):
    return 4 if act == "rpm" else 1


# ---------------------------------------------------------------- 1. gimbal rows on the io wave
UP, DOWN, NEAR = (0, 1, 16), (2, 3), 4


def _gimbal_poses(raw):
    raw[:, 2] = 1.0
    raw[:, 7:16] = 0.0
    s, c = np.sin(np.pi / 4), np.cos(np.pi / 4)
    for i in UP:
        raw[i, 3:7] = (0.0, s, 0.0, c)
    for i in DOWN:
        raw[i, 3:7] = (0.0, -s, 0.0, c)
    raw[NEAR, 3:7] = (0.0, np.sin(0.78), 0.0, np.cos(0.78))     # pitch 1.56 rad: the regular branch


def _equal_rotor_pool(rng, P, act):
    """A random action per env and slot with its components equal: exactly zero torques."""
    one = rng.uniform(-1, 1, (P, E, 1, 1)).astype(np.float32)
    return torch.from_numpy(np.repeat(one, _width(act), axis=3).copy()).cuda()


def _assert_gimbal_angles(rows):
    """rows [E, 12]: pitch +-float32(pi/2) and roll 0 on the seeded envs, 1.56 on the near one."""
    rpy = rows[:, 3:6].cpu().numpy()
    for i in UP:
        assert rpy[i, 1] == np.float32(HALF_PI) and rpy[i, 0] == 0.0, (i, rpy[i])
    for i in DOWN:
        assert rpy[i, 1] == np.float32(-HALF_PI) and rpy[i, 0] == 0.0, (i, rpy[i])
    assert abs(float(rpy[NEAR, 1]) - 1.56) < 1e-5, rpy[NEAR]


@pytest.mark.parametrize("store_policy", [1, 2], ids=["plain", "write-through"])
@pytest.mark.parametrize("T", [2, 4])
@pytest.mark.parametrize("act", ACTS)
def test_gimbal_rows_live(act, T, store_policy):
    """autoreset off: the seeded envs keep their attitude, so every step's live row comes from the
    gimbal fix-up on the io wave (pitch = +-float32(pi/2), roll = 0); env 4 at pitch 1.56 takes the
    regular branch beside them and is truncated (the C oracle shows the same in each of 4 steps)."""
    pool = _equal_rotor_pool(np.random.default_rng(50 + T), T, act)

    def each_step(i, a, tmpl):
        _assert_gimbal_angles(a.obs[:, 0, :12])
        assert bool(a.truncated[NEAR]) and all(bool(a.truncated[k]) for k in UP + DOWN)

    _twins(T, act, pool, _gimbal_poses, each_step=each_step, autoreset=False,
           tuning=dict(store_policy=store_policy))


@pytest.mark.parametrize("store_policy", [1, 2], ids=["plain", "write-through"])
@pytest.mark.parametrize("T", [2, 4])
@pytest.mark.parametrize("act", ACTS)
def test_gimbal_rows_terminal(act, T, store_policy):
    """autoreset on: step 0 truncates the seeded envs, so their gimbal angles go to the terminal
    rows and the live rows are the template's."""
    pool = _equal_rotor_pool(np.random.default_rng(60 + T), T, act)
    seeded = list(UP + DOWN) + [NEAR]

    def each_step(i, a, tmpl):
        if i == 0:
            _assert_gimbal_angles(a.terminal_obs[:, 0, :12])
            assert all(bool(a.truncated[k]) for k in seeded)
            assert torch.equal(a.obs[seeded, 0, :12], tmpl[seeded])

    _twins(T, act, pool, _gimbal_poses, each_step=each_step, tuning=dict(store_policy=store_policy))


# ---------------------------------------------------------------- 2. another lane reset in every step
def _staggered_ceiling(raw):
    """Env i crosses the z bound (2.0) in step i mod 8: z = 2 - 0.01 (i mod 8) - 0.005, vz = 0.3."""
    i = np.arange(E)
    raw[:, 2] = 2.0 - 0.01 * (i % 8) - 0.005
    raw[:, 9] = 0.3


def _zero_pool(P, act):
    return torch.zeros((P, E, 1, _width(act)), dtype=torch.float32, device="cuda:0")


def _staggered_want(n):
    return [[(i % 8) == t for i in range(E)] for t in range(n)]


@pytest.mark.parametrize("terminal_obs", [True, False], ids=["terminal", "no-terminal"])
@pytest.mark.parametrize("T,calls", [(10, 1), (5, 2)])
@pytest.mark.parametrize("act", ACTS)
def test_another_lane_reset_in_every_step(act, T, calls, terminal_obs):
    """Steps 0..7 each reset their own lanes (i mod 8 = t) next to lanes that go on, in both blocks,
    so the row buffer and the masks of both parities carry a different reset set in consecutive
    steps; steps 8 and 9 reset nothing.  T = 5 twice puts a reset on a launch's last step and on the
    next launch's first."""
    tr = _twins(T, act, _zero_pool(T, act), _staggered_ceiling, calls=calls, terminal_obs=terminal_obs)
    assert tr.tolist() == _staggered_want(10)


# ---------------------------------------------------------------- 3. last_clipped_action at the end
@pytest.mark.parametrize("act", ACTS)
def test_last_clipped_action_after_a_mixed_last_step(act):
    """T = 3 of the staggered pattern: the launch's last step resets lanes 2 and 10 and no other.
    Raw-state columns 16..19 are zero on them and the hover RPM (action 0) on the rest."""
    out = {}
    tr = _twins(3, act, _zero_pool(3, act), _staggered_ceiling, out=out)
    assert tr.tolist() == _staggered_want(3)
    last = out["raw_end"][:, 16:20]
    reset = np.array([(i % 8) == 2 for i in range(E)])
    assert (last[reset] == 0.0).all() and (last[~reset] > 1000.0).all(), last


@pytest.mark.parametrize("act", ACTS)
def test_last_clipped_action_from_the_right_slot(act):
    """T = 260 from a pool of 7 different slots: the second launch starts at slot 256 % 7 = 4 and its
    last step reads slot 259 % 7 = 0.  Actions of +-0.02 keep the envs inside the bounds (the time
    limit resets them all in step 240, none in the last step), so columns 16..19 hold action_to_rpm
    of slot 0 on every lane and of no other slot."""
    rng = np.random.default_rng(90)
    pool = torch.from_numpy(rng.uniform(-0.02, 0.02, (7, E, 1, _width(act))).astype(np.float32)).cuda()
    out = {}
    tr = _twins(260, act, pool, lambda raw: None, out=out, launches=2)
    assert not bool(tr[-1].any())
    last = out["raw_end"][:, 16:20]
    a = pool.cpu().numpy()[:, :, 0, :]                       # [7, E, A]
    ratio = last / last[:, :1].mean()                        # proportional to 1 + 0.05 a
    want = (1 + 0.05 * a) / (1 + 0.05 * a[0, :, :1]).mean()
    err = [np.abs(ratio - want[k]).max() for k in range(7)]
    assert err[0] < 1e-5 and min(err[1:]) > 1e-4, err


# ---------------------------------------------------------------- 4. fz across steps
@pytest.mark.parametrize("pyb_freq", [240, 30])
@pytest.mark.parametrize("act", ACTS)
def test_thrust_from_the_rate_chains(act, pyb_freq):
    """Full-scale random actions that differ per step (and per rotor for RPM) from a pool of 3
    slots, T = 9, on the staggered envs: a stale or wrong-parity fz moves the position within one
    step, on chain a's lanes and on the reset lanes that follow chain b.  pyb_freq 30 is nsub 1,
    where the chains' loop has no look-ahead."""
    rng = np.random.default_rng(70 + pyb_freq)
    pool = torch.from_numpy(rng.uniform(-1, 1, (3, E, 1, _width(act))).astype(np.float32)).cuda()
    assert not torch.equal(pool[0], pool[1]) and not torch.equal(pool[1], pool[2])
    tr = _twins(9, act, pool, _staggered_ceiling, pyb_freq=pyb_freq, ctrl_freq=30)
    # lanes reset and lanes that go on, in one block and step
    mixed = sum(int(tr[t, :TPB].any() and not tr[t, :TPB].all()) for t in range(tr.shape[0]))
    assert mixed >= 2 and bool(tr[0, 0]) and bool(tr[0, 8]) and bool(tr[0, 16])
