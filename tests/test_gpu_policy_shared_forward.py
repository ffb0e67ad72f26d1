"""The rollout kernel and the PPO gradient kernel compute the same bits for mu and V (libgpd_policy.so,
csrc/policy/: both take the K order, tile strides and output sums of their forward pass from
gpd_policy_mlp.h).

A deterministic rollout step writes act = mu, logp and V; fed back to the gradient kernel on the same
module as act, old_logp and ret, every row has act - mu == 0 and V - ret == 0 exactly, if and only if
the gradient kernel's forward pass lands on the rollout's bits.  Then dL/dmu and dL/dv are zero in
every row, and with them every gradient of the two networks, and the value loss is 0.  A shifted
act / ret shows that the zeros are not vacuous.

Shapes (n_obs, n_act, rows, max_blocks), the smallest that reach every load path, every obs bucket
and every group pattern: bucket 8 with scalar slice loads and fewer rows than a group; bucket 16 with
a lane group whose slice runs past n_obs and a partial last group; bucket 18 (float2 loads) with
several groups per block in the gradient kernel against one per block in the rollout; buckets 24,
36 (float4) and 48.  Reversed rows put a row in another group and another lane position."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

SHAPES = [(27, 1, 5, 0), (54, 2, 37, 0), (72, 4, 200, 2), (96, 3, 37, 0), (144, 8, 37, 0), (192, 8, 37, 0)]
PI = ("pi_w1", "pi_b1", "pi_w2", "pi_b2", "pi_w3", "pi_b3")
VF = ("vf_w1", "vf_b1", "vf_w2", "vf_b2", "vf_w3", "vf_b3")


def _policy(n_obs, n_act, seed):
    import learn
    torch.manual_seed(seed)
    pol = learn.ActorCritic(n_obs, n_act).cuda()
    with torch.no_grad():             # non-trivial biases and log-std (learn.py initialises them to 0)
        for p in pol.parameters():
            if p.dim() == 1:
                p.copy_(0.1 * torch.randn_like(p))
    return pol


@pytest.mark.parametrize("reverse", [False, True], ids=["rows", "reversed"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_gradient_forward_lands_on_the_rollouts_bits(shape, reverse):
    from gym_pybullet_drones_routing_amd.policy import PARAM_NAMES, MlpPolicyKernel, PpoGradKernel
    n_obs, n_act, rows, max_blocks = shape
    pol = _policy(n_obs, n_act, n_obs)
    g = torch.Generator(device="cuda").manual_seed(rows)
    obs = torch.randn((rows, n_obs), generator=g, device="cuda") * 0.7
    adv = torch.randn(rows, generator=g, device="cuda")
    buf_act, buf_logp, buf_val = torch.zeros((rows, n_act), device="cuda"), torch.zeros(rows, device="cuda"), \
        torch.zeros(rows, device="cuda")
    MlpPolicyKernel(pol).step(obs, buf_act=buf_act, buf_logp=buf_logp, buf_val=buf_val, deterministic=True)
    idx = torch.arange(rows - 1, -1, -1, device="cuda") if reverse else None
    k = PpoGradKernel(pol, max_rows=rows, max_blocks=max_blocks)

    def grads(act, ret):
        k.grad_step(idx, obs, act, buf_logp, adv, ret, 0.2, 0.5, 0.0)
        torch.cuda.synchronize()
        return {n: v.clone() for n, v in zip(PARAM_NAMES, k.views)}, k.stats.clone()

    gr, stats = grads(buf_act, buf_val)
    assert float(stats[1]) == 0.0                       # V - ret == 0 in every row
    for n in VF + PI:                                   # ... and act - mu == 0 (== 0 also accepts -0.0)
        assert bool((gr[n] == 0).all()), f"{n}: {int((gr[n] != 0).sum())} non-zero elements"
    # against vacuity: a shifted action reaches the actor, a shifted return the critic
    gr, _ = grads(buf_act + 0.25, buf_val)
    assert bool((gr["pi_w1"] != 0).any())
    gr, stats = grads(buf_act, buf_val + 1)
    assert float(stats[1]) > 0.0 and bool((gr["vf_w1"] != 0).any())
