"""bench.py --dump-outputs: what the last timed vector step computed, as .npy files that two builds can be compared by.
CPU: the size limit and the seeded env sample.  GPU (-m gpu): the files of both workloads, and the same files from two runs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from conftest import ROOT


def _files(d):
    return {f[:-4]: np.load(os.path.join(d, f), allow_pickle=False) for f in sorted(os.listdir(d))}


def test_write_outputs_keeps_one_seeded_env_sample_under_the_limit(tmp_path, monkeypatch):
    n = 1000
    g = torch.Generator().manual_seed(0)
    outputs = {"obs": (torch.randn(n, 23, generator=g), True), "reward": (torch.randn(n, generator=g), True),
               "done": ((torch.rand(n, generator=g) < 0.1).to(torch.uint8), True),
               "w": (torch.randn(500_000, generator=g), False), "s": (torch.randn(10, generator=g, dtype=torch.float64), False)}
    bench.write_outputs(str(tmp_path / "full"), outputs, n)
    full = _files(tmp_path / "full")
    assert full["obs"].shape == (n, 23) and full["done"].dtype == np.float32 and full["s"].dtype == np.float64
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 2_060_000)
    for d in ("a", "b"):
        bench.write_outputs(str(tmp_path / d), outputs, n)
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= 2_060_000
    a, b = _files(tmp_path / "a"), _files(tmp_path / "b")
    assert all(np.array_equal(a[k], b[k]) for k in a)                       # the same sample every time
    assert 0 < len(a["obs"]) < n and np.array_equal(a["w"], full["w"])      # the per-env arrays shrink, nothing else does
    rows = [int(np.flatnonzero((full["obs"] == r).all(1))[0]) for r in a["obs"]]
    assert rows == sorted(set(rows))                                        # distinct envs, in env order ...
    assert np.array_equal(full["reward"][rows], a["reward"]) and np.array_equal(full["done"][rows], a["done"])   # ... in every array


def _bench_dump(out_dir, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "20", "--warmup", "5", "--no-cpu-baseline",
                        "--repeats", "1", "--dump-outputs", str(out_dir)] + list(extra),
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads([x for x in r.stdout.splitlines() if x.strip()][-1])["steps"] == 20
    files = _files(out_dir)
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir)) <= 64 * 10 ** 6
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in files.values())
    assert files["obs"].shape == (65536, 23) and files["reward"].shape == files["done"].shape == (65536,)
    assert set(np.unique(files["done"])) <= {0.0, 1.0}
    return files


@pytest.mark.gpu
def test_ddpg_outputs_are_the_same_in_two_runs(tmp_path, gpu_device):
    a = _bench_dump(tmp_path / "a")
    b = _bench_dump(tmp_path / "b")
    nets = {f"{net}.{k}" for net in ("actor", "critic", "target_actor", "target_critic") for k in
            (("fc1", "bn1", "fc2", "bn2", "mu") if "actor" in net else ("fc1", "bn1", "fc2", "bn2", "action_value", "q"))}
    assert set(a) == {"obs", "action", "reward", "done"} | {f"{p}.{w}" for p in nets for w in ("weight", "bias")}
    assert a["action"].shape == (65536,) and a["actor.fc1.weight"].shape == (400, 23)
    assert not np.array_equal(a["actor.fc1.weight"], a["target_actor.fc1.weight"])     # learn() ran: the target trails
    different = [k for k in a if not np.array_equal(a[k], b[k])]
    assert not different, different


@pytest.mark.gpu
def test_env_workload_outputs(tmp_path, gpu_device):
    assert set(_bench_dump(tmp_path, "--workload", "env")) == {"obs", "reward", "done"}
