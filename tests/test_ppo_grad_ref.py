"""tests/ppo_grad_ref.py (numpy float64, hand-written backward) against torch float64 autograd of
examples/learn.py's minibatch loss (``GraphedMinibatch._body``): <= 1e-10 relative per tensor.  The
GPU tests then hold the HIP kernel (gpd_policy_ppo_grad) against both."""
import numpy as np
import pytest
import torch

from tests import ppo_grad_ref as ref

CASES = [(27, 1, 37), (72, 4, 5), (144, 8, 64)]
VF_COEF = 0.5


@pytest.mark.parametrize("n_obs,n_act,rows", CASES)
def test_reference_matches_autograd(n_obs, n_act, rows):
    module, c, cls = ref.covered_case(n_obs, n_act, rows)
    p = ref.module_params(module)
    # sign of A x ratio below / inside / above the range: all six (five rows hold five of them)
    assert len(cls) == min(6, rows), cls
    # every row >= 0.1 from a clip boundary (the ratios are 0.7 .. 1.3 up to old_logp's f32 rounding)
    assert ref.classes(p, c)[1] > 0.1 - 1e-5
    flat, stats, g = ref.ppo_grad_ref(p, c["obs"], c["act"], c["old_logp"], c["adv"], c["ret"], c["clip"], VF_COEF,
                                      idx=c["idx"])
    tg, tl = ref.torch_grad(module, c, torch.float64, VF_COEF)
    off = 0
    for name in ref.NAMES:
        scale = np.abs(tg[name]).max()
        assert scale > 0, name
        assert np.abs(g[name] - tg[name]).max() <= 1e-10 * scale, name
        np.testing.assert_array_equal(flat[off:off + g[name].size], g[name].reshape(-1))   # the flat order
        off += g[name].size
    assert off == flat.size == sum(prm.numel() for prm in module.parameters())
    np.testing.assert_allclose(stats[:2], tl, rtol=1e-12)
    assert abs(stats[2] - np.sqrt(sum((t ** 2).sum() for t in tg.values()))) <= 1e-10 * stats[2]


def test_clip_scale_and_clip_fraction():
    module, c = ref.make_case(27, 1, 37, seed=0)
    p = ref.module_params(module)
    args = (p, c["obs"], c["act"], c["old_logp"], c["adv"], c["ret"], c["clip"], VF_COEF)
    flat, stats, _ = ref.ppo_grad_ref(*args)
    clipped, stats2, _ = ref.ppo_grad_ref(*args, max_grad_norm=0.5 * stats[2])
    np.testing.assert_array_equal(stats, stats2)               # the norm is reported before clipping
    np.testing.assert_allclose(clipped, flat * (0.5 * stats[2] / (stats[2] + 1e-6)), rtol=1e-15)
    same, _, _ = ref.ppo_grad_ref(*args, max_grad_norm=1e30)
    np.testing.assert_array_equal(same, flat)
    ratio = np.exp(ref.logp_of(p, c["obs"], c["act"]) - c["old_logp"])
    assert stats[3] == np.mean((ratio < 0.8) | (ratio > 1.2)) and 0 < stats[3] < 1
