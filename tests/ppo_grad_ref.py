"""A plain float64 restatement of the PPO minibatch gradient (include/gpd_policy.h:
gpd_policy_ppo_grad) in numpy: the loss of examples/learn.py's ``GraphedMinibatch._body`` and a
hand-written backward pass.  Shares nothing with the kernel; tests/test_ppo_grad_ref.py pins it to
torch float64 autograd, the GPU tests compare the kernel against both.

Parameters travel as a dict of float64 arrays named like gpd_mlp_policy's fields
(``pi_w1 [64][n_obs]`` ... ``vf_b3 [1]``, ``log_std [n_act]``); the flat gradient is their
gradients concatenated in ``NAMES`` order.
"""
import math

import numpy as np

NAMES = ("pi_w1", "pi_b1", "pi_w2", "pi_b2", "pi_w3", "pi_b3", "vf_w1", "vf_b1", "vf_w2", "vf_b2", "vf_w3", "vf_b3",
         "log_std")
LOG_SQRT_2PI = math.log(math.sqrt(2 * math.pi))


def module_params(module):
    """examples/learn.py's ActorCritic -> the float64 dict."""
    lin = [m for seq in (module.pi, module.vf) for m in seq if hasattr(m, "weight")]
    ts = [t for m in lin for t in (m.weight, m.bias)] + [module.log_std]
    return {n: t.detach().double().cpu().numpy().copy() for n, t in zip(NAMES, ts)}


def _mlp(p, net, x):
    h1 = np.tanh(x @ p[net + "_w1"].T + p[net + "_b1"])
    h2 = np.tanh(h1 @ p[net + "_w2"].T + p[net + "_b2"])
    return h1, h2, h2 @ p[net + "_w3"].T + p[net + "_b3"]


def _mlp_backward(p, net, x, h1, h2, dout, g):
    g[net + "_w3"] = dout.T @ h2
    g[net + "_b3"] = dout.sum(0)
    dz2 = (dout @ p[net + "_w3"]) * (1 - h2 ** 2)
    g[net + "_w2"] = dz2.T @ h1
    g[net + "_b2"] = dz2.sum(0)
    dz1 = (dz2 @ p[net + "_w2"]) * (1 - h1 ** 2)
    g[net + "_w1"] = dz1.T @ x
    g[net + "_b1"] = dz1.sum(0)


def logp_of(p, obs, act):
    """Normal(pi(obs), exp(log_std)).log_prob(act).sum(-1)."""
    mu = _mlp(p, "pi", obs)[2]
    scale = np.exp(p["log_std"])
    return (-((act - mu) ** 2) / (2 * scale ** 2) - p["log_std"] - LOG_SQRT_2PI).sum(-1)


def ppo_grad_ref(p, obs, act, old_logp, adv, ret, clip, vf_coef, max_grad_norm=0.0, idx=None):
    """-> (flat gradient [n_params], stats [4] = policy loss, value loss, gradient norm before
    clipping, clip fraction, per-tensor gradient dict), everything float64."""
    if idx is not None:
        obs, act, old_logp, adv, ret = obs[idx], act[idx], old_logp[idx], adv[idx], ret[idx]
    obs, act = np.asarray(obs, np.float64), np.asarray(act, np.float64)
    n = obs.shape[0]
    h1p, h2p, mu = _mlp(p, "pi", obs)
    h1v, h2v, v = _mlp(p, "vf", obs)
    v = v[:, 0]
    var = np.exp(p["log_std"]) ** 2
    d = act - mu
    logp = (-(d ** 2) / (2 * var) - p["log_std"] - LOG_SQRT_2PI).sum(-1)
    ratio = np.exp(logp - old_logp)
    a = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8)
    s1, s2 = ratio * a, np.clip(ratio, 1 - clip, 1 + clip) * a
    pg = -np.minimum(s1, s2).mean()
    vl = ((v - ret) ** 2).mean()
    # min(s1, s2): ratio receives the gradient through s1, and through s2 inside the clip range
    flow = (s1 < s2) | ((ratio >= 1 - clip) & (ratio <= 1 + clip))
    dlogp = np.where(flow, -a * ratio, 0.0) / n
    g = {}
    _mlp_backward(p, "pi", obs, h1p, h2p, dlogp[:, None] * d / var, g)
    _mlp_backward(p, "vf", obs, h1v, h2v, (vf_coef * 2 * (v - ret) / n)[:, None], g)
    g["log_std"] = (dlogp[:, None] * (d ** 2 / var - 1)).sum(0)
    flat = np.concatenate([g[k].reshape(-1) for k in NAMES])
    norm = math.sqrt(float((flat ** 2).sum()))
    stats = np.array([pg, vl, norm, (np.abs(ratio - 1) > clip).mean()])
    if max_grad_norm > 0:
        scale = min(1.0, max_grad_norm / (norm + 1e-6))
        flat = flat * scale
        g = {k: t * scale for k, t in g.items()}
    return flat, stats, g


RATIOS = (0.7, 0.9, 1.0, 1.1, 1.3)


def make_case(n_obs, n_act, rows, seed, pool=1, clip=0.2):
    """The tests' one input recipe: a seeded ActorCritic, obs ~ N(0, 1), act = mu + scale N(0, 1),
    old_logp = logp_ref - log r with r from RATIOS (every row then >= 0.1 away from a clip boundary of
    clip = 0.2: a float32 evaluation picks the same branch of min), adv ~ N(0, 1), ret ~ N(0, 1).
    ``pool`` > 1: buffers of pool x rows rows and a shuffled int64 ``idx`` of `rows` of them.
    -> (module (float32, CPU), float64 dict of the inputs)."""
    import os
    import sys

    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "examples"))
    from learn import ActorCritic
    torch.manual_seed(seed)
    module = ActorCritic(n_obs, n_act)
    with torch.no_grad():      # away from the zero initialisation: every tensor gets a gradient of its own size
        for prm in module.parameters():
            prm.add_(0.05 * torch.randn_like(prm))
        module.pi[4].weight.mul_(10.0)
    p = module_params(module)
    rng = np.random.default_rng(seed)
    N = rows * pool
    obs = rng.standard_normal((N, n_obs)).astype(np.float32).astype(np.float64)
    mu = _mlp(p, "pi", obs)[2]
    act = (mu + np.exp(p["log_std"]) * rng.standard_normal((N, n_act))).astype(np.float32).astype(np.float64)
    r = np.asarray(RATIOS)[rng.integers(0, len(RATIOS), N)]
    old_logp = (logp_of(p, obs, act) - np.log(r)).astype(np.float32).astype(np.float64)
    adv = rng.standard_normal(N).astype(np.float32).astype(np.float64)
    ret = rng.standard_normal(N).astype(np.float32).astype(np.float64)
    idx = rng.permutation(N)[:rows].astype(np.int64) if pool > 1 else None
    return module, dict(obs=obs, act=act, old_logp=old_logp, adv=adv, ret=ret, idx=idx, clip=clip)


def classes(p, c):
    """The six (sign of A) x (ratio below / inside / above the clip range) classes present in a case."""
    sel = (lambda t: t[c["idx"]]) if c["idx"] is not None else (lambda t: t)
    ratio = np.exp(logp_of(p, sel(c["obs"]), sel(c["act"])) - sel(c["old_logp"]))
    adv = sel(c["adv"])
    a = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8)
    zone = np.where(ratio < 1 - c["clip"], 0, np.where(ratio > 1 + c["clip"], 2, 1))
    return {(bool(s), int(z)) for s, z in zip(a > 0, zone)}, np.abs(np.abs(ratio - 1) - c["clip"]).min()


def covered_case(n_obs, n_act, rows, pool=1, seeds=200):
    """make_case at the first seed whose minibatch holds all six classes (min(6, rows) distinct ones:
    five rows cannot hold six) -> (module, case, classes)."""
    for seed in range(seeds):
        module, c = make_case(n_obs, n_act, rows, seed, pool)
        cls, _ = classes(module_params(module), c)
        if len(cls) == min(6, rows):
            return module, c, cls
    raise AssertionError(f"no seed below {seeds} covers the classes at {rows} rows")


def torch_grad(module, c, dtype, vf_coef, device="cpu"):
    """torch autograd of GraphedMinibatch._body's loss in `dtype` on the case's minibatch ->
    (per-tensor gradient dict of float64 arrays in NAMES order, [policy loss, value loss])."""
    import copy

    import torch
    m = copy.deepcopy(module).to(device=device, dtype=dtype)
    sel = (lambda t: t[c["idx"]]) if c["idx"] is not None else (lambda t: t)
    obs, act, old, adv, ret = (torch.as_tensor(sel(c[k]), dtype=dtype, device=device)
                               for k in ("obs", "act", "old_logp", "adv", "ret"))
    mu = m.pi(obs)
    scale = m.log_std.exp()
    logp = (-((act - mu) ** 2) / (2 * scale ** 2) - scale.log() - math.log(math.sqrt(2 * math.pi))).sum(-1)
    ratio = (logp - old).exp()
    ma = (adv - adv.mean()) / (adv.std() + 1e-8)
    pg = -torch.min(ratio * ma, ratio.clamp(1 - c["clip"], 1 + c["clip"]) * ma).mean()
    vl = ((m.value(obs) - ret) ** 2).mean()
    (pg + vf_coef * vl).backward()
    lin = [x for seq in (m.pi, m.vf) for x in seq if hasattr(x, "weight")]
    ts = [t for x in lin for t in (x.weight, x.bias)] + [m.log_std]
    return ({n: t.grad.detach().double().cpu().numpy() for n, t in zip(NAMES, ts)},
            np.array([float(pg.detach()), float(vl.detach())]))
