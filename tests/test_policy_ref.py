"""Pins tests/policy_ref.py, the host restatement the GPU policy tests compare the kernel with, so
those tests do not rest on an unchecked reference: Philox against Random123's published
known-answer vectors, the float64 forward against torch's own, the normal draw by its moments and
by which counter / key word each argument reaches."""
import math
import os
import sys

import numpy as np
import torch

from tests import policy_ref as ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def _words(s):
    return [int(w, 16) for w in s.split()]


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    kats = [("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
            ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
            ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kats:
        assert ref.philox4x32_10(_words(ctr), _words(key)).tolist() == _words(want)
    # vectorised: the three at once give the same rows
    got = ref.philox4x32_10(np.array([_words(c) for c, _, _ in kats]), np.array([_words(k) for _, k, _ in kats]))
    assert got.tolist() == [_words(w) for _, _, w in kats]


def test_u01_is_the_float32_expression():
    x = np.array([0, 255, 256, (1 << 31) - 1, 1 << 31, (1 << 32) - 1], dtype=np.uint64)
    u = ref.u01(x)
    assert u.dtype == np.float32
    assert u[0] == u[1] == np.float32(2.0 ** -25) and u[2] == np.float32(1.5 * 2.0 ** -24)
    assert u[3] == np.float32((2 ** 23 - 0.5) * 2.0 ** -24)         # the last value the sum holds exactly
    assert u[4] == np.float32(0.5)                                    # 2^23 + 0.5 rounds to even: 2^23
    assert u[5] == np.float32(1.0)                                    # 2^24 - 0.5 rounds up to 2^24
    assert (u > 0).all()


def test_forward64_matches_torch_double():
    import copy

    import learn
    for n_obs, n_act in ((1, 1), (27, 3), (192, 8)):
        torch.manual_seed(n_obs)
        pol = learn.ActorCritic(n_obs, n_act)
        with torch.no_grad():
            for p in pol.parameters():
                if p.dim() == 1:
                    p.copy_(0.1 * torch.randn_like(p))
        obs = torch.randn(41, n_obs) * 2.0
        mu, v = ref.forward64(pol, obs)
        mu32, v32 = ref.forward32(pol, obs)
        assert mu.dtype == v.dtype == np.float64 and mu.shape == (41, n_act) and v.shape == (41,)
        assert mu32.dtype == v32.dtype == np.float32
        pd = copy.deepcopy(pol).double()
        with torch.no_grad():
            tmu, tv = pd.pi(obs.double()).numpy(), pd.value(obs.double()).numpy()
        assert np.abs(mu - tmu).max() <= 1e-13 and np.abs(v - tv).max() <= 1e-13
        assert np.abs(mu32 - mu).max() < 1e-5 and np.abs(v32 - v).max() < 1e-5


def test_std_normal_moments_and_argument_routing():
    rows = np.arange(125000)[:, None]
    a = np.arange(8)[None, :]
    seed = (0x01234567 << 32) | 0x89ABCDEF
    eps, rad = ref.std_normal64(seed, 7, rows, a, with_radius=True)
    assert eps.shape == rad.shape == (125000, 8) and eps.dtype == np.float64
    n = eps.size
    assert n == 10 ** 6
    assert abs(eps.mean()) < 5 / math.sqrt(n)
    assert abs(eps.var(ddof=1) - 1.0) < 6 * math.sqrt(2.0 / n)
    assert abs((np.abs(eps) < 1).mean() - 0.682689) < 0.01
    assert (np.abs(eps) <= rad).all()
    # a pair shares its radius: cosine on even a, sine on odd a
    np.testing.assert_allclose(eps[:, 0::2] ** 2 + eps[:, 1::2] ** 2, rad[:, 0::2] ** 2, rtol=1e-12, atol=1e-300)
    assert np.array_equal(rad[:, 0::2], rad[:, 1::2])
    # every argument reaches the generator: a different call (low or high word), row, a >> 2 or seed
    # word (low or high) gives different draws, the same arguments the same draws
    r = np.arange(64)
    base = ref.std_normal64(seed, 7, r, 1)
    assert np.array_equal(base, ref.std_normal64(seed, 7, r, 1))
    for other in (ref.std_normal64(seed, 8, r, 1), ref.std_normal64(seed, 7 + (1 << 32), r, 1),
                  ref.std_normal64(seed, 7, r + 64, 1), ref.std_normal64(seed, 7, r + (1 << 16), 1),
                  ref.std_normal64(seed, 7, r, 5), ref.std_normal64(seed, 7, r, 3),
                  ref.std_normal64(seed ^ 1, 7, r, 1), ref.std_normal64(seed ^ (1 << 32), 7, r, 1),
                  ref.std_normal64(seed ^ (1 << 63), 7, r, 1)):
        assert not np.any(other == base)
    # per-element call counters (one per row group) are honoured element by element
    calls = np.array([3, 3, 9, (1 << 32) + 1], dtype=np.uint64)
    mixed = ref.std_normal64(seed, calls, np.arange(4), 0)
    for i in range(4):
        assert mixed[i] == ref.std_normal64(seed, int(calls[i]), i, 0)
    # the seed is a 64-bit key: taken mod 2^64
    assert np.array_equal(ref.std_normal64(-1, 7, r, 1), ref.std_normal64(2 ** 64 - 1, 7, r, 1))


def test_bootstrap64_definition():
    import learn
    torch.manual_seed(3)
    pol = learn.ActorCritic(5, 2)
    rew = np.array([1.0, 2.0, 3.0, 4.0], dtype=np.float32)
    te = np.array([0, 1, 0, 1], dtype=np.uint8)
    tr = np.array([0, 0, 1, 1], dtype=np.uint8)
    tobs = torch.randn(4, 5)
    tobs[[0, 1, 3]] = float("nan")          # rows that are not bootstrapped may hold anything
    out, done, boot = ref.bootstrap64(pol, rew, te, tr, tobs, 0.99)
    v = ref.forward64(pol, tobs[2:3])[1][0]
    assert boot.tolist() == [False, False, True, False] and done.tolist() == [0.0, 1.0, 1.0, 1.0]
    assert out.tolist() == [1.0, 2.0, 3.0 + float(np.float32(0.99)) * v, 4.0]
    out32, _, _ = ref.bootstrap32(pol, rew, te, tr, tobs, 0.99)
    assert out32.dtype == np.float32 and abs(float(out32[2]) - out[2]) < 1e-6 and not np.isnan(out32).any()
