"""A plain high-precision restatement of gpd_policy_rollout_step (include/gpd_policy.h) on the host:
numpy and CPU torch only, nothing native, so CPU tests can import it (tests/test_policy_ref.py
pins it; tests/test_gpu_policy_edges.py compares the kernel with it).

  forward64 / forward32   the actor and critic MLPs (Linear-Tanh-Linear-Tanh-Linear) in float64, and
                          the same arithmetic in float32: the yardstick of the float32 kernel's error
  philox4x32_10           Salmon et al.'s counter-based generator, vectorised in uint64 arithmetic
  u01                     the kernel's uniform in (0, 1], computed in float32 exactly as it writes it
  std_normal64            the kernel's Box-Muller draw of (seed, call, row, a), from u01 on in float64
  bootstrap64 / 32        buf_rew and buf_done of the previous step as the header defines them
"""
import math

import numpy as np
import torch

MASK32 = np.uint64(0xFFFFFFFF)
GROUP_ROWS = 16            # rows that share a Philox call counter


def _np(x, dtype):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x).astype(dtype)


def _linears(seq):
    return [m for m in seq if isinstance(m, torch.nn.Linear)]


def _mlp(seq, x, dtype):
    lin = _linears(seq)
    assert len(lin) == 3
    for i, l in enumerate(lin):
        x = x @ _np(l.weight, dtype).T + _np(l.bias, dtype)
        if i < 2:
            x = np.tanh(x)
    assert x.dtype == dtype
    return x


def layer1_preact64(module, obs):
    """The actor's layer-1 pre-activations z = W1 x + b1 in float64 (how saturated tanh is)."""
    l = _linears(module.pi)[0]
    return _np(obs, np.float64) @ _np(l.weight, np.float64).T + _np(l.bias, np.float64)


def _forward(module, obs, dtype):
    x = _np(obs, dtype)
    return _mlp(module.pi, x, dtype), _mlp(module.vf, x, dtype)[:, 0]


def forward64(module, obs):
    """mu [E, n_act] and v [E] in float64 from the module's parameters cast to float64."""
    return _forward(module, obs, np.float64)


def forward32(module, obs):
    """The same arithmetic in float32 on the CPU."""
    return _forward(module, obs, np.float32)


def philox4x32_10(counter, key):
    """Philox4x32-10: counter [..., 4] and key [..., 2] (broadcast against each other) of 32-bit
    words -> [..., 4] uint64 holding 32-bit words."""
    c = np.asarray(counter, dtype=np.uint64) & MASK32
    k = np.asarray(key, dtype=np.uint64) & MASK32
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                    # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & MASK32, (p0 >> s32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + w0) & MASK32, (k1 + w1) & MASK32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def u01(x):
    """((float)(x >> 8) + 0.5f) * 2^-24 in float32: for x >> 8 >= 2^23 the sum rounds to even, so
    the result can be exactly 1.0 (a float64 restatement would not be)."""
    n = (np.asarray(x, dtype=np.uint64) >> np.uint64(8)).astype(np.float32)
    u = (n + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    assert u.dtype == np.float32
    return u


def std_normal64(seed, call, row, a, with_radius=False):
    """Standard normal number ``a`` (< 8) of ``row`` for call counter ``call`` under the 64-bit key
    ``seed`` (arguments broadcast).  Counter (row, a >> 2, call lo, call hi), key (seed lo, seed hi);
    the pair (c0, c1) serves a & 3 in {0, 1}, (c2, c3) serves {2, 3}; even a takes the cosine, odd a
    the sine.  The uniforms are the kernel's float32 ones; everything after them is float64."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    row, a, call = np.broadcast_arrays(np.asarray(row, dtype=np.uint64), np.asarray(a, dtype=np.uint64),
                                       np.asarray(call, dtype=np.uint64))
    s32 = np.uint64(32)
    ctr = np.stack([row & MASK32, a >> np.uint64(2), call & MASK32, call >> s32], axis=-1)
    out = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    second = ((a & np.uint64(3)) >> np.uint64(1)).astype(bool)
    u0 = u01(np.where(second, out[..., 2], out[..., 0])).astype(np.float64)
    u1 = u01(np.where(second, out[..., 3], out[..., 1])).astype(np.float64)
    rad = np.sqrt(-2.0 * np.log(u0))
    ang = 2.0 * math.pi * u1
    eps = np.where((a & np.uint64(1)).astype(bool), rad * np.sin(ang), rad * np.cos(ang))
    return (eps, rad) if with_radius else eps


def _bootstrap(module, reward, terminated, truncated, terminal_obs, gamma, dtype):
    rew = _np(reward, dtype)
    te, tr = _np(terminated, bool), _np(truncated, bool)
    boot = tr & ~te
    out = rew.copy()
    if boot.any():      # V only of the rows that are used: the others may hold anything, NaN included
        tobs = _np(terminal_obs, dtype)[boot]
        v = _forward(module, tobs, dtype)[1]
        out[boot] = rew[boot] + dtype(np.float32(gamma)) * v      # the kernel's gamma is a float
    assert out.dtype == dtype
    return out, (te | tr).astype(np.float32), boot


def bootstrap64(module, reward, terminated, truncated, terminal_obs, gamma):
    """buf_rew (float64), buf_done (1.0 / 0.0) and the mask of bootstrapped rows:
    buf_rew = reward + gamma * V(terminal_obs) where truncated and not terminated, reward elsewhere."""
    return _bootstrap(module, reward, terminated, truncated, terminal_obs, gamma, np.float64)


def bootstrap32(module, reward, terminated, truncated, terminal_obs, gamma):
    """The same in float32 (the yardstick beside forward32)."""
    return _bootstrap(module, reward, terminated, truncated, terminal_obs, gamma, np.float32)
