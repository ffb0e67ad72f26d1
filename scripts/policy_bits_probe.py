"""Probe: one SHA-256 per output tensor of libgpd_policy.so for a fixed list of seeded calls, to compare
two builds of the library bit for bit (GPD_POLICY_LIB chooses the build; one process per build).

    GPD_POLICY_LIB=/path/to/libgpd_policy.so python scripts/policy_bits_probe.py OUT.json

Per shape (n_obs, n_act, rows, max_blocks) of tests/test_gpu_policy_shared_forward.py: the rollout step
deterministic, sampled twice, forward + bootstrap, bootstrap only and critic only; GAE; the gradient
with and without idx, with max_grad_norm 0 and 0.5.  Two builds agree iff the two files are equal."""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import learn  # noqa: E402
from gym_pybullet_drones_routing_amd.policy import MlpPolicyKernel, PpoGradKernel  # noqa: E402

SHAPES = [(27, 1, 5, 0), (54, 2, 37, 0), (72, 4, 200, 2), (96, 3, 37, 0), (144, 8, 37, 0), (192, 8, 37, 0)]


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def probe(n_obs, n_act, rows, max_blocks):
    dev = "cuda:0"
    torch.manual_seed(n_obs)
    pol = learn.ActorCritic(n_obs, n_act).to(dev)
    with torch.no_grad():
        for p in pol.parameters():
            if p.dim() == 1:
                p.copy_(0.1 * torch.randn_like(p))
    g = torch.Generator(device=dev).manual_seed(rows)

    def randn(*shape):
        return torch.randn(shape, generator=g, device=dev)

    obs, tobs, adv = randn(rows, n_obs) * 0.7, randn(rows, n_obs) * 0.7, randn(rows)
    rew = torch.rand(rows, generator=g, device=dev)
    te = (torch.rand(rows, generator=g, device=dev) < 0.1).to(torch.uint8)
    tr = (torch.rand(rows, generator=g, device=dev) < 0.4).to(torch.uint8)
    out = {}
    k = MlpPolicyKernel(pol, seed=7)

    shapes = {"act_env": (rows, n_act), "buf_obs": (rows, n_obs), "buf_act": (rows, n_act), "buf_logp": (rows,),
              "buf_val": (rows,), "buf_rew": (rows,), "buf_done": (rows,)}

    def step(name, obs_, prev=None, only=None, **kw):
        names = ["act_env", "buf_obs", "buf_act", "buf_logp", "buf_val"] if obs_ is not None else []
        names += ["buf_rew", "buf_done"] if prev is not None else []
        t = {b: torch.full(shapes[b], 7.0, device=dev) for b in only or names}
        k.step(obs_, prev=prev, **t, **kw)
        out.update({f"{name}.{b}": sha(v) for b, v in t.items()})
        return t

    det = step("det", obs, deterministic=True)
    step("sample1", obs)
    step("sample2", obs)
    step("forward_boot", obs, prev=(rew, te, tr, tobs))
    step("boot_only", None, prev=(rew, te, tr, tobs))
    step("critic_only", obs, only=["buf_val"])
    out["rng"] = sha(k.rng)
    T = 8
    E = rows
    r, v, d = torch.rand((T, E), generator=g, device=dev), randn(T, E), \
        (torch.rand((T, E), generator=g, device=dev) < 0.1).float()
    ga, gr = torch.zeros((T, E), device=dev), torch.zeros((T, E), device=dev)
    k.gae(r, v, d, randn(E), 0.99, 0.95, ga, gr)
    out["gae.adv"], out["gae.ret"] = sha(ga), sha(gr)
    gk = PpoGradKernel(pol, max_rows=rows, max_blocks=max_blocks)
    act = det["buf_act"] + 0.3 * randn(rows, n_act)
    logp, ret = det["buf_logp"] + 0.1 * randn(rows), det["buf_val"] + 0.5 * randn(rows)
    for name, idx in (("rows", None), ("idx", torch.randperm(rows, generator=g, device=dev))):
        for mgn in (0.0, 0.5):
            gk.grad_step(idx, obs, act, logp, adv, ret, 0.2, 0.5, mgn)
            out[f"grad.{name}.{mgn}.grad"], out[f"grad.{name}.{mgn}.stats"] = sha(gk.grad), sha(gk.stats)
    return out


if __name__ == "__main__":
    res = {"-".join(map(str, s)): probe(*s) for s in SHAPES}
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(f"{sum(len(v) for v in res.values())} digests -> {sys.argv[1]}")
