"""Time per control step of the closed-loop rollout (gpd_cmd_rollout) beside the path that gives
the same result without it: the same T command steps as capture_cmd_graph launches.

    python scripts/cmd_rollout_probe.py [--reps 3] [--out FILE]

Configurations: 4096 and 65536 single-drone DYN envs at 240 / 30 in RPM mode, and 4096
single-drone Physics.PYB envs at 240 / 48 in waypoint mode, T = 192 each (the examples/pid.py
flight); beside them 1024 PYB envs of 3 drones (the pair-contact instantiation).  Each is timed
three ways, as graph replays in alternated windows:
  rollout_norec  cmd_rollout(record=False)
  rollout_rec    cmd_rollout(record_every=1)
  stepwise       T cmd_step launches in one graph (capture_cmd_graph)
--reps child processes, one after the other; each first checks that the rollout and the stepwise
path end in the same state (to 1e-9; the figure is printed) before it times them.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T, REPLAYS, ROUNDS = 192, 12, 5     # steps per flight, flights per timed window, windows
# name -> (mode, envs, drones per env); the last one is beside the three gated sizes: multi-drone PYB
# envs run the pair-contact code, the instantiation with the most registers
CONFIGS = {"rpm_4096": ("rpm", 4096, 1), "rpm_65536": ("rpm", 65536, 1), "waypoint_4096": ("waypoint", 4096, 1),
           "waypoint_1024x3": ("waypoint", 1024, 3)}
VARIANTS = ("rollout_norec", "rollout_rec", "stepwise")


def child():
    import numpy as np
    import torch
    from gym_pybullet_drones_routing_amd.enums import ActionType, Physics
    from gym_pybullet_drones_routing_amd.sim import BatchedAviarySim, graph_capture

    def window(graph):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPLAYS):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1000 / (REPLAYS * T)

    def make(cfg):
        mode, E, D = CONFIGS[cfg]
        if mode == "rpm":
            return E, D, mode, BatchedAviarySim(n_envs=E, task="none", ctrl_freq=30, device="cuda:0")
        # the start of examples/pid.py: on a circle of 0.3 m, a sixth of a turn and 5 cm of height apart
        ph0 = np.arange(D) * (2 * np.pi / 6) + np.pi / 2
        xyz = np.stack([0.3 * np.cos(ph0), 0.3 * np.sin(ph0) - 0.3, 0.1 + 0.05 * np.arange(D)], 1)
        return E, D, mode, BatchedAviarySim(n_envs=E, drones_per_env=D, task="none", ctrl_freq=48, act=ActionType.VEL,
                                            physics=Physics.PYB, autoreset=False, initial_xyzs=xyz, device="cuda:0")

    out = {}
    for cfg in CONFIGS:
        sims = {}
        for var in VARIANTS:
            E, D, mode, sims[var] = make(cfg)
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(0)
        if mode == "rpm":
            hover = 14468.429183500699
            acts = hover * (1 + 0.05 * (2 * torch.rand((T, E, 1, 4), generator=gen, device="cuda:0",
                                                       dtype=torch.float64) - 1))
        else:   # a slow circle around the start position, the drones of an env in formation (one phase per
            # env).  (The multi-drone controller instantiations of the two paths round integral_rpy_e
            # differently in the last bit; this closed loop is chaotic on some flights, where
            # that grows past the gate below within the 192 steps.  On this one the states stay equal.)
            t = torch.arange(T, device="cuda:0", dtype=torch.float64).reshape(T, 1, 1) / 48
            ph = 2 * torch.pi * (t / 10.0 + torch.rand((1, E, 1), generator=gen, device="cuda:0", dtype=torch.float64))
            pos0 = sims["stepwise"].state20()[:, 0:3].reshape(1, E, D, 3)
            acts = torch.zeros((T, E, D, 7), dtype=torch.float64, device="cuda:0")
            acts[..., 0:3] = pos0
            acts[..., 0] += 0.3 * (torch.cos(ph) - torch.cos(ph[0:1]))
            acts[..., 1] += 0.3 * (torch.sin(ph) - torch.sin(ph[0:1]))
            acts[..., 2] += 0.5
        acts = acts.contiguous()
        graphs = {"stepwise": sims["stepwise"].capture_cmd_graph([acts[k] for k in range(T)], mode)}
        keep = []
        warm = make(cfg)[3]       # the kernel's first launch stays out of the captures
        warm.cmd_rollout(acts[:2], mode)
        warm.close()
        for var, kw in (("rollout_norec", dict(record=False)), ("rollout_rec", dict(record_every=1))):
            sims[var]._cmd_rows()
            g = torch.cuda.CUDAGraph()
            with graph_capture(g, sims[var].device):
                keep.append(sims[var].cmd_rollout(acts, mode, **kw))
            graphs[var] = g
        for var in VARIANTS:      # one flight each from the same start: the paths agree
            graphs[var].replay()
        torch.cuda.synchronize()
        ref = sims["stepwise"].raw_state()
        diff = max(float((sims[var].raw_state() - ref).abs().max()) for var in VARIANTS)
        assert bool(torch.isfinite(ref).all()), f"{cfg}: the flight diverged"
        assert diff <= 1e-9, f"{cfg}: cmd_rollout != {T} cmd_step calls: max abs difference {diff}"
        times = {var: [] for var in VARIANTS}
        for var in VARIANTS:      # warm-up window
            window(graphs[var])
        for _ in range(ROUNDS):   # alternated windows
            for var in VARIANTS:
                times[var].append(window(graphs[var]))
        out[cfg] = dict(times, max_abs_diff=diff)
        del graphs, keep
        for s in sims.values():
            s.close()
    print("PROBE " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child()
    runs = []
    for rep in range(args.reps):
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True,
                             timeout=300)
        if res.returncode != 0:       # a failed child ends the probe: nothing more is started
            sys.stderr.write(res.stdout + res.stderr)
            raise SystemExit(f"child {rep} failed with status {res.returncode}")
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("PROBE ")][-1]
        runs.append(json.loads(line[6:]))
        print(f"rep {rep}: {line[6:]}", flush=True)
    summary = {}
    for cfg in CONFIGS:
        for var in VARIANTS:
            vals = [v for r in runs for v in r[cfg][var]]
            summary[f"{cfg} {var}"] = {"median": round(statistics.median(vals), 3), "min": round(min(vals), 3),
                                       "max": round(max(vals), 3), "n": len(vals)}
    for k, v in summary.items():
        print(f"{k}: median {v['median']} us per step (min {v['min']}, max {v['max']}, n {v['n']})")
    for cfg in CONFIGS:
        r, b = summary[f"{cfg} rollout_norec"], summary[f"{cfg} stepwise"]
        print(f"{cfg}: rollout median below stepwise: {r['median'] < b['median']}; "
              f"windows apart (rollout max < stepwise min): {r['max'] < b['min']}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"steps_per_flight": T, "flights_per_window": REPLAYS, "runs": runs, "summary": summary}, f,
                      indent=1)


if __name__ == "__main__":
    main()
