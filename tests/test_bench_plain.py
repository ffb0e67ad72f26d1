"""bench.py's plain run and its options: a plain run times the requested steps and prints the
headline line only, --full adds the other legs, --dump-outputs writes the last timed step's
outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("kernel_us", "roofline", "eager", "other_launch_form", "strong", "handoff", "rollout", "sweep",
             "other_configs", "raw_integrator", "cpu_baseline", "parity")


def test_options_default_to_a_plain_run():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    """One plain run (64 envs, 3 timed steps of 12 in all: an upload replay of the 3-step graph,
    one warm-up step, the timed replay): the line holds the headline fields and none of the --full
    legs, and the dumped arrays are what the same launches leave in the sim's output tensors."""
    import torch

    from gym_pybullet_drones_routing_amd.shard import rank_seed
    from gym_pybullet_drones_routing_amd.sim import BatchedAviarySim

    E, K, W = 64, 3, 1
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup",
                        str(W), "--envs", str(E), "--dump-outputs", str(out)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    for k in HEADLINE:
        assert k in line, k
    assert not [k for k in FULL_ONLY if k in line]
    assert line["steps"] == K and line["warmup"] == W and line["full"] is False
    assert line["unit"] == "drone*dt/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["value"] == pytest.approx(E * 8 / (line["ms_per_step"] * 1e-3))
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(got) == {"obs", "reward", "terminated", "truncated", "terminal_obs"}
    assert set(line["outputs"]["files"]) == {k + ".npy" for k in got}
    assert all(a.dtype == np.float32 for a in got.values())

    sim = BatchedAviarySim(n_envs=E, task="hover", precision="f64", autoreset=True, device="cuda:0")
    pool = bench.make_pool(E, 4, sim.device, seed=rank_seed(1000, 0))
    bench.time_graph(sim, pool, K, W, kernel_time=False)
    torch.cuda.synchronize()
    assert got["obs"].shape == (E, 1, sim.obs_width)
    np.testing.assert_array_equal(got["obs"], sim.obs.cpu().numpy())
    np.testing.assert_array_equal(got["reward"], sim.reward.cpu().numpy())
    np.testing.assert_array_equal(got["terminated"], sim.terminated.cpu().numpy().astype(np.float32))
    np.testing.assert_array_equal(got["truncated"], sim.truncated.cpu().numpy().astype(np.float32))
    done = (sim.terminated | sim.truncated).bool().cpu().numpy()
    np.testing.assert_array_equal(got["terminal_obs"][done], sim.terminal_obs.cpu().numpy()[done])
    assert not got["terminal_obs"][~done].any()
    sim.close()


@pytest.mark.gpu
def test_large_batch_dump_is_a_fixed_sample():
    """Past the 64 MB budget the snapshot keeps a seeded, sorted sample of the envs, the same in
    every run, and its files stay within the budget."""
    from gym_pybullet_drones_routing_amd.sim import BatchedAviarySim

    E = 1 << 18
    sim = BatchedAviarySim(n_envs=E, task="hover", precision="f64", autoreset=True, device="cuda:0")
    a, b = bench.OutputSnapshot(sim, 1), bench.OutputSnapshot(sim, 1)
    assert a.index is not None and np.array_equal(a.index, b.index)
    assert np.all(np.diff(a.index) > 0) and 0 <= a.index[0] and a.index[-1] < E
    a.take()
    n = a.index.size
    assert a.fields["obs"].shape == (n, 1, sim.obs_width)
    assert np.array_equal(a.fields["obs"].cpu().numpy(), sim.obs.cpu().numpy()[a.index])
    total = sum(v.numel() * 4 for v in a.fields.values()) + 8 * n
    assert 0.9 * bench.DUMP_BUDGET_BYTES < total <= bench.DUMP_BUDGET_BYTES
    sim.close()
