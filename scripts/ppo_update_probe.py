"""Per-minibatch PPO update time at the learner's own size: the fused gradient (policy.PpoGradKernel +
torch Adam, learn.py --fused-update) beside learn.py's eager minibatch step and its --graph step, in
one process, alternating between the three in rounds after a warm-up (profiles/ppo_grad/README.md).

    python scripts/ppo_update_probe.py [--rows 262144] [--minibatch 16384] [--rounds 7] [--out FILE]

Every path runs the same work per round: one epoch (rows / minibatch steps) over the same seeded
buffers with a fresh randperm, ending in a device synchronise; the time is per minibatch step.  The
three paths train three copies of the same initial policy (their gradients differ in the last bits,
so their parameters drift apart: timing only).
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import learn  # noqa: E402
from gym_pybullet_drones_routing_amd.policy import PpoGradKernel  # noqa: E402

CLIP, VF_COEF, MAX_NORM, LR = 0.2, 0.5, 0.5, 3e-4


def eager_step(policy, opt, b, idx):
    """learn.py train()'s eager minibatch step."""
    d = policy.dist(b["obs"][idx])
    logp = d.log_prob(b["act"][idx]).sum(-1)
    ratio = (logp - b["logp"][idx]).exp()
    ma = b["adv"][idx]
    ma = (ma - ma.mean()) / (ma.std() + 1e-8)
    pg = -torch.min(ratio * ma, ratio.clamp(1 - CLIP, 1 + CLIP) * ma).mean()
    vl = ((policy.value(b["obs"][idx]) - b["ret"][idx]) ** 2).mean()
    loss = pg + VF_COEF * vl
    opt.zero_grad(set_to_none=True)
    loss.backward()
    nn.utils.clip_grad_norm_(policy.parameters(), MAX_NORM)
    opt.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--minibatch", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--grad-only", type=int, default=0, metavar="N",
                    help="only N gradient calls per shape and nothing else (the run to put under a kernel trace)")
    a = ap.parse_args()
    dev = "cuda:0"
    results = []
    for n_obs, n_act in ((27, 1), (72, 4)):
        torch.manual_seed(0)
        base = learn.ActorCritic(n_obs, n_act).to(dev)
        N, mb = a.rows, a.minibatch
        b = {"obs": torch.randn(N, n_obs, device=dev), "act": torch.randn(N, n_act, device=dev) * 0.5,
             "adv": torch.randn(N, device=dev), "ret": torch.randn(N, device=dev)}
        with torch.no_grad():
            b["logp"] = base.dist(b["obs"]).log_prob(b["act"]).sum(-1) + 0.1 * torch.randn(N, device=dev)
        if a.grad_only:
            gk = PpoGradKernel(base, max_rows=mb)
            idx = torch.randperm(N, device=dev)[:mb]
            for _ in range(a.grad_only):
                gk.grad_step(idx, b["obs"], b["act"], b["logp"], b["adv"], b["ret"], CLIP, VF_COEF, MAX_NORM)
            torch.cuda.synchronize()
            continue
        pols = {k: copy.deepcopy(base) for k in ("fused", "eager", "graph")}
        opts = {k: torch.optim.Adam(p.parameters(), lr=LR, eps=1e-5, capturable=(k == "graph")) for k, p in pols.items()}
        gk = PpoGradKernel(pols["fused"], max_rows=mb)
        gstep = learn.GraphedMinibatch(pols["graph"], opts["graph"], mb, n_obs, n_act, CLIP, VF_COEF, MAX_NORM, dev)

        def epoch(kind):
            perm = torch.randperm(N, device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(0, N, mb):
                idx = perm[s:s + mb]
                if kind == "fused":
                    gk.grad_step(idx, b["obs"], b["act"], b["logp"], b["adv"], b["ret"], CLIP, VF_COEF, MAX_NORM)
                    opts["fused"].step()
                elif kind == "graph":
                    gstep.step(b["obs"][idx], b["act"][idx], b["logp"][idx], b["adv"][idx], b["ret"][idx])
                else:
                    eager_step(pols["eager"], opts["eager"], b, idx)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / (N // mb)

        kinds = ("fused", "eager", "graph")
        for k in kinds:              # warm-up: code objects, the allocator, Adam's state
            epoch(k)
        times = {k: [] for k in kinds}
        for _ in range(a.rounds):    # alternating
            for k in kinds:
                times[k].append(epoch(k))
        # the gradient alone (four launches, no optimizer), by device events
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        idx = torch.randperm(N, device=dev)[:mb]
        reps = 200
        ev[0].record()
        for _ in range(reps):
            gk.grad_step(idx, b["obs"], b["act"], b["logp"], b["adv"], b["ret"], CLIP, VF_COEF, MAX_NORM)
        ev[1].record()
        torch.cuda.synchronize()
        rec = {"n_obs": n_obs, "n_act": n_act, "rows": N, "minibatch": mb, "rounds": a.rounds,
               "grad_only_us": round(ev[0].elapsed_time(ev[1]) * 1e3 / reps, 2)}
        for k in kinds:
            rec[k + "_us"] = {"median": round(statistics.median(times[k]) * 1e6, 1),
                              "min": round(min(times[k]) * 1e6, 1), "max": round(max(times[k]) * 1e6, 1)}
        for k in kinds:
            assert all(bool(torch.isfinite(p).all()) for p in pols[k].parameters()), k
        print(json.dumps(rec), flush=True)
        results.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
