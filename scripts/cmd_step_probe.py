"""Time of the command step (gpd_cmd_step, RPM mode) under graph replay, at 4096 and 65536
single-drone DYN envs, 240 / 30, beside the path that gives the same result without it:
gpd_integrate of the eight repeated RPM rows followed by gpd_get_state20 (two launches, a
caller-made [8][N][4] tensor, no clip).

    python scripts/cmd_step_probe.py [--libs main,x] [--reps 3] [--out FILE]

--libs: library builds to time, alternated --reps times, each in a child process of its own
(`main` = libgpd.so, else the A/B build libgpd_<name>.so of `_build.build(variant=...)`; the
retired -DGPD_CMD_ROWS_PER_LANE build, whose lanes stored their state20 rows themselves instead of
through the LDS-staged copy-out, was timed this way: DESIGN.md §8.1, profiles/cmd_step/).  Each
child checks that both paths end in the same state (to 1e-9; the figure is printed) before it
times them.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (4096, 65536)
G, REPLAYS, ROUNDS = 16, 200, 5     # steps per graph, replays per timed window, windows


def child():
    import torch
    from gym_pybullet_drones_routing_amd.sim import BatchedAviarySim

    def window(graph):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPLAYS):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1000 / (REPLAYS * G)

    out = {}
    for E in SIZES:
        gen = torch.Generator(device="cuda:0")
        gen.manual_seed(0)
        hover = 14468.429183500699
        rpm = [(hover * (1 + 0.05 * (2 * torch.rand((E, 1, 4), generator=gen, device="cuda:0", dtype=torch.float64) - 1)))
               .contiguous() for _ in range(G)]
        rows8 = [r.reshape(1, E, 4).repeat(8, 1, 1).contiguous() for r in rpm]
        fused = BatchedAviarySim(n_envs=E, task="none", ctrl_freq=30, device="cuda:0")
        split = BatchedAviarySim(n_envs=E, task="none", ctrl_freq=30, device="cuda:0")
        s20 = torch.empty((E, 20), dtype=torch.float64, device="cuda:0")
        g_fused = fused.capture_cmd_graph(rpm, "rpm")
        g_split = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_split):
            for r in rows8:
                split._call("gpd_integrate", r.data_ptr(), 8, None, torch.cuda.current_stream().cuda_stream)
                split._call("gpd_get_state20", s20.data_ptr(), torch.cuda.current_stream().cuda_stream)
        for _ in range(3):      # warm-up, and the two paths agree
            g_fused.replay()
            g_split.replay()
        torch.cuda.synchronize()
        diff = float((fused._obs20.reshape(E, 20) - s20).abs().max())
        assert diff <= 1e-9, f"cmd_step != integrate + state20: max abs difference {diff}"
        t_f, t_s = [], []
        for _ in range(ROUNDS):  # alternated windows
            t_f.append(window(g_fused))
            t_s.append(window(g_split))
        out[str(E)] = {"cmd_step_us": t_f, "integrate_state20_us": t_s, "max_abs_diff": diff}
        fused.close()
        split.close()
    print("PROBE " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", default="main")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child()
    pkg = os.path.join(ROOT, "gym_pybullet_drones_routing_amd")
    runs = {}
    for rep in range(args.reps):
        for lib in args.libs.split(","):
            env = dict(os.environ)
            env["GPD_LIB"] = os.path.join(pkg, "libgpd.so" if lib == "main" else f"libgpd_{lib}.so")
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True,
                                 text=True, timeout=240)
            if res.returncode != 0:       # a failed child ends the probe: nothing more is started
                sys.stderr.write(res.stdout + res.stderr)
                raise SystemExit(f"child for {lib} failed with status {res.returncode}")
            line = [ln for ln in res.stdout.splitlines() if ln.startswith("PROBE ")][-1]
            runs.setdefault(lib, []).append(json.loads(line[6:]))
            print(f"rep {rep} {lib}: {line[6:]}", flush=True)
    summary = {}
    for lib, reps in runs.items():
        for E in map(str, SIZES):
            for key in ("cmd_step_us", "integrate_state20_us"):
                vals = [v for r in reps for v in r[E][key]]
                summary[f"{lib} E={E} {key}"] = {"median": round(statistics.median(vals), 3),
                                                 "min": round(min(vals), 3), "max": round(max(vals), 3), "n": len(vals)}
    for k, v in summary.items():
        print(f"{k}: median {v['median']} us per step (min {v['min']}, max {v['max']}, n {v['n']})")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"graph_steps": G, "replays_per_window": REPLAYS, "runs": runs, "summary": summary}, f, indent=1)


if __name__ == "__main__":
    main()
