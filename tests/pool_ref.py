"""Reference for reset pools: a vector of oracle envs that get a new drone and start pose,
drawn from the pools, each time they end.

Test infrastructure only.  The loop is ``tests.oracle_runs.run_vec``'s plus one thing: when an env
ends, it becomes the pool's drone (``het_ref.apply_row``) at the pool's pose (``het_ref.apply_poses``)
before ``env.reset()``, which is what building a new env object from another URDF and start pose
would give.  The draw is restated here in Python ints (numpy's int64 scalars warn on the multiply).
"""
import numpy as np

from tests import het_ref

STREAM_ROWS, STREAM_POSES = 1, 2
M32 = 0xffffffff


def mix32(x):
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def draw(seed, stream, e, k, n):
    """Index in [0, n) of env e's k-th auto-reset; stream 1 = parameter rows, 2 = poses."""
    seed, stream, e, k, n = int(seed), int(stream), int(e), int(k), int(n)
    h = mix32((seed ^ (0x9e3779b9 * stream)) & M32)
    h = mix32((h + e) & M32)
    h = mix32((h + k) & M32)
    return (h * n) >> 32


def run_pool(actions, envs, pool_rows=None, pool_xyz=None, pool_rpy=None, seed=0, draws=None):
    """actions [T, E, D, A] float32 over the oracle envs ``envs`` -> run_vec's outputs (obs
    [T, E, D, W], reward [T, E], term / trunc [T, E], terminal obs {(t, e): [D, W]}) plus the draws
    [E, 3] int32 {episode number, row index, pose index; -1 = not drawn}.  pool_rows: {name: array[P]}
    or None (parameters never redrawn); pool_xyz / pool_rpy: [Q, D, 3] or None (poses never redrawn;
    rpy None = zeros).  Pass ``draws`` to continue a run."""
    T, E = actions.shape[0], len(envs)
    P = 0 if pool_rows is None else len(next(iter(pool_rows.values())))
    Q = 0 if pool_xyz is None else len(pool_xyz)
    if draws is None:
        draws = np.tile(np.array([0, -1, -1], dtype=np.int32), (E, 1))
    obs_l, rew, te, tr, term_obs = [], np.zeros((T, E)), np.zeros((T, E), bool), np.zeros((T, E), bool), {}
    for t in range(T):
        row = []
        for e, env in enumerate(envs):
            o, r, a_t, b_t, _ = env.step(actions[t, e])
            rew[t, e], te[t, e], tr[t, e] = r, a_t, b_t
            if a_t or b_t:
                term_obs[(t, e)] = o
                k = int(draws[e, 0]) + 1
                draws[e, 0] = k
                if P:
                    draws[e, 1] = draw(seed, STREAM_ROWS, e, k, P)
                    het_ref.apply_row(env, het_ref.rows_of(pool_rows, draws[e, 1]))
                if Q:
                    q = draws[e, 2] = draw(seed, STREAM_POSES, e, k, Q)
                    het_ref.apply_poses(env, pool_xyz[q], pool_rpy[q] if pool_rpy is not None else np.zeros_like(pool_xyz[q]))
                o, _ = env.reset()
            row.append(o)
        obs_l.append(np.stack(row))
    return np.stack(obs_l), rew, te, tr, term_obs, draws
