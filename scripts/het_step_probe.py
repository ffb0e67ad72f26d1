"""Step time of a heterogeneous sim (per-env drone parameters, gpd_create_het) under graph replay,
beside the two kernels a plain sim of the same shape runs:

    het      step_kernel_het, rows +-10 % of nominal (assets.randomized_params)
    pool     the same sim with a reset pool (256 rows +-10 %, 16 start poses): the pooled
             instantiation of step_kernel_het, which redraws each env's drone and pose at auto-reset
    nominal  the one-wave step_kernel (tuning step_waves = 1): the code the het kernel restates
    default  whatever gpd_create selects (the three-wave kernel at 4096 single-drone envs, the
             two-wave one at 65536; the one-wave kernel for multi-drone envs)

at 4096 and 65536 single-drone DYN RPM hover envs and at 512 envs x 8 drones with downwash
(MultiHover, staggered start poses so that the downwash acts), f64, 240 / 30.

How often an env resets decides what the pooled tail costs, so the child reports the episodes per
env.  Under the random four-motor actions of the shapes above, replayed in a cycle of 16, a drone
tilts past the truncation bound within 16 to 80 steps: nearly every wave has a reset in nearly
every step.  The shapes 4096x1v and 4096x1v_ep0.5 take collective-thrust actions (one value for
the four motors, zero mean over the cycle): the drones bob in place and only the time limit ends
an episode, every 241st step at the default episode_len_sec = 8 and every 17th at 0.5.

    python scripts/het_step_probe.py [--reps 3] [--out FILE]

Every (shape, repetition) runs in a child process of its own; inside it the three sims replay
their captured graphs in alternated timed windows.  The child first checks that the het sim with
its +-10 % rows really differs from the nominal one (and would equal it on nominal rows: that is
tests/test_gpu_het.py's job).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"4096x1": (4096, 1, ()), "65536x1": (65536, 1, ()), "512x8dw": (512, 8, ("dw",)),
          "4096x1v": (4096, 1, (), {"vertical": True}),
          "4096x1v_ep0.5": (4096, 1, (), {"vertical": True, "episode_len_sec": 0.5})}
VARIANTS = ("het", "pool", "nominal", "default")
POOL_ROWS, POOL_POSES = 256, 16
G, REPLAYS, ROUNDS = 16, 100, 5     # steps per graph, replays per timed window, windows


def child(shape):
    import numpy as np
    import torch
    from gym_pybullet_drones_routing_amd.assets import randomized_params
    from gym_pybullet_drones_routing_amd.sim import BatchedAviarySim

    E, D, aero = SHAPES[shape][:3]
    kw = dict(n_envs=E, drones_per_env=D, task="hover" if D == 1 else "multihover", aero=aero, precision="f64",
              device="cuda:0")
    opts = dict(SHAPES[shape][3]) if len(SHAPES[shape]) > 3 else {}
    vertical = opts.pop("vertical", False)
    kw.update(opts)
    if D > 1:   # drone i at (0.15 cos, 0.15 sin, 0.5 + 0.1 i): the downwash acts
        i = np.arange(D)
        kw["initial_xyzs"] = np.stack([0.15 * np.cos(2 * np.pi * i / D), 0.15 * np.sin(2 * np.pi * i / D),
                                       0.5 + 0.1 * i], 1)
    # pool poses: each env's default start pose moved by up to 5 cm in xy (the stagger of the
    # multi-drone shape, and with it the downwash, stays)
    base = BatchedAviarySim(n_envs=1, drones_per_env=D, task=kw["task"], precision="f64", device="cuda:0",
                            initial_xyzs=kw.get("initial_xyzs"))
    xyz0 = base.raw_state().cpu().numpy()[:, 0:3]
    base.close()
    pxyz = np.tile(xyz0, (POOL_POSES, 1, 1))
    pxyz[:, :, 0:2] += np.random.default_rng(2).uniform(-0.05, 0.05, (POOL_POSES, 1, 2))
    pool = dict(env_params=randomized_params(POOL_ROWS, 0.1, seed=1), initial_xyzs=pxyz, seed=0)
    sims = {"het": BatchedAviarySim(env_params=randomized_params(E, 0.1, seed=0), **kw),
            "pool": BatchedAviarySim(env_params=randomized_params(E, 0.1, seed=0), reset_pool=pool, **kw),
            "nominal": BatchedAviarySim(tuning={"step_waves": 1}, **kw),
            "default": BatchedAviarySim(**kw)}
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(0)
    acts = [(0.2 * (2 * torch.rand((E, D, 4), generator=gen, device="cuda:0") - 1)).contiguous() for _ in range(G)]
    if vertical:
        u = torch.stack(acts)[..., :1]
        acts = list((u - u.mean(0, keepdim=True)).expand(-1, -1, -1, 4).contiguous())
    graphs = {k: s.capture_graph(acts) for k, s in sims.items()}

    def window(graph):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPLAYS):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1000 / (REPLAYS * G)

    for g in graphs.values():   # warm-up
        g.replay()
    torch.cuda.synchronize()
    diff = float((sims["het"].obs[..., :12] - sims["nominal"].obs[..., :12]).abs().max())
    # (collective thrust around each env's own hover RPM accelerates every drone alike, whatever
    # its mass and kf: the vertical shapes leave this check to the others)
    assert vertical or diff > 1e-6, "the het sim's rows do not act"
    t = {k: [] for k in VARIANTS}
    for _ in range(ROUNDS):      # alternated windows
        for k in VARIANTS:
            t[k].append(window(graphs[k]))
    draws = sims["pool"].reset_draws().cpu().numpy()
    out = {"us_per_step": t, "het_vs_nominal_obs_diff": diff,
           "steps": (1 + ROUNDS * REPLAYS) * G,
           "pool_episodes_per_env": [int(draws[:, 0].min()), int(draws[:, 0].max())],
           "pool_rows_in_force": int(len(set(draws[:, 1].tolist()))),
           "lanes_per_block": {k: int(s.constants.lanes_per_block) for k, s in sims.items()},
           "drones_per_block": {k: int(s.constants.drones_per_block) for k, s in sims.items()}}
    for s in sims.values():
        s.close()
    print("PROBE " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    runs = {}
    for rep in range(args.reps):
        for shape in args.shapes.split(","):
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape], capture_output=True,
                                 text=True, timeout=240)
            if res.returncode != 0:       # a failed child ends the probe: nothing more is started
                sys.stderr.write(res.stdout + res.stderr)
                raise SystemExit(f"child for {shape} failed with status {res.returncode}")
            line = [ln for ln in res.stdout.splitlines() if ln.startswith("PROBE ")][-1]
            runs.setdefault(shape, []).append(json.loads(line[6:]))
            print(f"rep {rep} {shape}: {line[6:]}", flush=True)
    summary = {}
    for shape, reps in runs.items():
        for k in VARIANTS:
            vals = [v for r in reps for v in r["us_per_step"][k]]
            per_child = [statistics.median(r["us_per_step"][k]) for r in reps]
            summary[f"{shape} {k}"] = {"median": round(statistics.median(vals), 3), "min": round(min(vals), 3),
                                       "max": round(max(vals), 3), "n": len(vals),
                                       "child_medians": [round(v, 3) for v in per_child],
                                       "lanes_per_block": reps[0]["lanes_per_block"][k]}
    for k, v in summary.items():
        print(f"{k}: median {v['median']} us per step (min {v['min']}, max {v['max']}, n {v['n']}; per child "
              f"{v['child_medians']}; {v['lanes_per_block']} lanes per block)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"graph_steps": G, "replays_per_window": REPLAYS, "runs": runs, "summary": summary}, f, indent=1)


if __name__ == "__main__":
    main()
