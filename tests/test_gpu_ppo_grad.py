"""The PPO minibatch gradient kernel (gpd_policy_ppo_grad, csrc/policy/gpd_ppo_grad.hip; policy.PpoGradKernel)
against torch float64 autograd of examples/learn.py's minibatch loss and tests/ppo_grad_ref.py.

The parity gate is relative to torch itself: per tensor, err = max |g - g64| / max |g64|; e32 is that
error of torch's own float32 autograd on the same inputs (on the GPU, as the eager loop runs it), and
the kernel must stay within K * max(e32, 2^-23).  K covers the one thing the kernel does differently
from torch at equal precision: the order in which the rows are summed (16-row MFMA chains, then
groups per block, then slabs in block order, instead of torch's GEMM and reduction trees).  The floor
of 2^-23 - one float32 ulp of the tensor's largest element - is for tensors of one or a few elements
(vf_b3, pi_b3, log_std), where a float32 result can land on the rounded float64 value by luck and
e32 is then 0.

MEASURED on an MI355X (the first run of these cases; profiles/ppo_grad/README.md has the table): the
worst kernel-error / max(e32, 2^-23) per case was 3.15, 2.69, 0.98, 7.62, 2.04, 2.84, 3.75, 3.23 over
the gradient tensors, and <= 6.4 over the three stats, so K = 8, the smallest power of two that holds.
Both values above 4 are one-number sums that cancel: vf_b3 = mean(V - ret) of (72, 4, 37) with idx (the
kernel 9.1e-7, i.e. 7.6 ulp of the sum itself, where torch's float32 landed 0.3 ulp from the float64
value) and the policy loss of (144, 8, 1000) with idx (8.8e-6 against torch's 1.4e-6); their error is
the rounding of terms many times larger than the result, and which order of summation happens to
come out closer is luck.  Over the tensors with more than eight elements the worst ratio was 3.15.
"""
import math

import numpy as np
import pytest
import torch

from tests import ppo_grad_ref as ref

pytestmark = pytest.mark.gpu

K = 8
FLOOR = 2.0 ** -23
VF_COEF = 0.5
# (n_obs, n_act, rows, max_blocks): fewer rows than one group; a partial last group; several groups
# accumulated per block (13 groups on 2 blocks); many slabs (63 blocks)
SHAPES = [(27, 1, 5, 0), (72, 4, 37, 0), (54, 2, 200, 2), (144, 8, 1000, 0)]


class Case:
    """One seeded case on the device with its references, computed once and shared (read-only)."""

    def __init__(self, n_obs, n_act, rows, max_blocks, pool):
        from gym_pybullet_drones_routing_amd.policy import PpoGradKernel
        self.module, self.c, self.cls = ref.covered_case(n_obs, n_act, rows, pool=pool)
        self.p = ref.module_params(self.module)
        self.rows = rows
        self.g64, self.l64 = ref.torch_grad(self.module, self.c, torch.float64, VF_COEF)
        self.g32, self.l32 = ref.torch_grad(self.module, self.c, torch.float32, VF_COEF, device="cuda")
        self.dev = {k: torch.as_tensor(self.c[k], dtype=torch.float32, device="cuda").contiguous()
                    for k in ("obs", "act", "old_logp", "adv", "ret")}
        self.idx = torch.as_tensor(self.c["idx"], device="cuda") if self.c["idx"] is not None else None
        self.kernel = PpoGradKernel(self.module.to("cuda"), max_rows=rows, max_blocks=max_blocks)

    def run(self, max_grad_norm=0.0):
        d = self.dev
        self.kernel.grad_step(self.idx, d["obs"], d["act"], d["old_logp"], d["adv"], d["ret"], self.c["clip"], VF_COEF,
                              max_grad_norm, n_rows=self.rows)
        torch.cuda.synchronize()
        return self.kernel.grad.clone(), self.kernel.stats.clone()


_cases = {}


def case(shape, pool):
    if (shape, pool) not in _cases:
        _cases[(shape, pool)] = Case(*shape, pool)
    return _cases[(shape, pool)]


def _err(a, b64):
    return float(np.abs(a - b64).max() / np.abs(b64).max())


@pytest.mark.parametrize("pool", [1, 3], ids=["rows", "idx"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_gradient_parity(shape, pool):
    """pool = 3: a shuffled idx into buffers of 3 x the rows, gathered by the kernel."""
    cs = case(shape, pool)
    assert len(cs.cls) == min(6, shape[2])
    grad, stats = cs.run()
    grad = grad.double().cpu().numpy()
    for prm, view in zip(cs.kernel._params, cs.kernel.views):      # the per-parameter views are the .grad
        assert prm.grad is view and view.data_ptr() >= cs.kernel.grad.data_ptr()
    off, worst = 0, 0.0
    for name in ref.NAMES:
        g64 = cs.g64[name]
        mine = grad[off:off + g64.size].reshape(g64.shape)
        off += g64.size
        e, e32 = _err(mine, g64), _err(cs.g32[name], g64)
        print(f"{shape} pool {pool} {name}: kernel {e:.3e} torch-f32 {e32:.3e} ratio {e / max(e32, FLOOR):.2f}")
        worst = max(worst, e / max(e32, FLOOR))
        assert e <= K * max(e32, FLOOR), (name, e, e32)
    assert off == grad.size
    print(f"{shape} pool {pool}: worst ratio {worst:.2f}")
    # stats: the two losses and the norm under the same rule, the clip fraction exactly
    flat64, s64, _ = ref.ppo_grad_ref(cs.p, cs.c["obs"], cs.c["act"], cs.c["old_logp"], cs.c["adv"], cs.c["ret"],
                                      cs.c["clip"], VF_COEF, idx=cs.c["idx"])
    st = stats.double().cpu().numpy()
    n32 = math.sqrt(sum(float((t.astype(np.float32) ** 2).sum()) for t in cs.g32.values()))
    e32s = [abs(cs.l32[0] - s64[0]) / abs(s64[0]), abs(cs.l32[1] - s64[1]) / abs(s64[1]), abs(n32 - s64[2]) / s64[2]]
    for q in range(3):
        e = abs(st[q] - s64[q]) / abs(s64[q])
        print(f"{shape} pool {pool} stats[{q}]: kernel {e:.3e} torch-f32 {e32s[q]:.3e}")
        assert e <= K * max(e32s[q], FLOOR), (q, st[q], s64[q])
    assert st[3] == np.float32(s64[3])


def test_clip_scales_like_clip_grad_norm():
    cs = case(SHAPES[1], 1)
    raw, stats = cs.run(0.0)
    norm = stats[2]
    assert float(norm) > 0.5 * 1.01, "the case must be clipped at 0.5"
    clipped, stats2 = cs.run(0.5)
    assert torch.equal(stats, stats2)                       # the norm is the one before clipping
    want = raw * torch.clamp(0.5 / (norm + 1e-6), max=1.0)  # float32, as clip_grad_norm_ forms it
    ulp = 2.0 ** -23
    assert float(((clipped - want).abs() / want.abs().clamp_min(1e-30)).max()) <= 4 * ulp
    same, _ = cs.run(1e30)
    assert torch.equal(same, raw)


def test_deterministic_and_capturable():
    from gym_pybullet_drones_routing_amd.sim import graph_capture
    cs = case(SHAPES[2], 3)
    a, sa = cs.run(0.5)
    b, sb = cs.run(0.5)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    d = cs.dev
    graph = torch.cuda.CUDAGraph()
    with graph_capture(graph, torch.cuda.current_device()):      # statistics + main + reduce + finish
        cs.kernel.grad_step(cs.idx, d["obs"], d["act"], d["old_logp"], d["adv"], d["ret"], cs.c["clip"], VF_COEF, 0.5)
    for _ in range(2):
        cs.kernel.grad.zero_()
        cs.kernel.workspace.fill_(float("nan"))              # nothing survives from an earlier call
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cs.kernel.grad, a) and torch.equal(cs.kernel.stats, sa)


def test_wrapper_refuses_bad_calls():
    cs = case(SHAPES[0], 1)
    d = cs.dev
    with pytest.raises(ValueError, match="rows"):
        cs.kernel.grad_step(torch.zeros(cs.rows + 1, dtype=torch.int64, device="cuda"), d["obs"], d["act"],
                            d["old_logp"], d["adv"], d["ret"], 0.2, VF_COEF, 0.5)
    with pytest.raises(ValueError, match="idx"):
        cs.kernel.grad_step(torch.zeros(cs.rows, dtype=torch.int32, device="cuda"), d["obs"], d["act"],
                            d["old_logp"], d["adv"], d["ret"], 0.2, VF_COEF, 0.5)
    with pytest.raises(ValueError, match="same"):
        cs.kernel.grad_step(None, d["obs"], d["act"], d["old_logp"], d["adv"][:-1], d["ret"], 0.2, VF_COEF, 0.5)


def test_learner_runs_with_the_fused_update():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import learn
    policy, hist, _, _ = learn.train(n_envs=64, n_steps=8, minibatch=128, epochs=1, total_timesteps=1024, fused=True,
                                     fused_update=True, log=lambda *a: None)
    assert len(hist) == 2 and all("update_s" in h for h in hist)
    for prm in policy.parameters():
        assert bool(torch.isfinite(prm).all())
    # the optimizer saw the kernel's views as the parameters' .grad: log_std left its zero initialisation
    assert float(policy.log_std.detach().abs().max()) > 0
