"""bench.py's command line without a GPU: --steps is validated before anything starts, and --dump-outputs writes float32
arrays within its size cap, sampling the same pairs on every run."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_refuses_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr, (r.returncode, r.stderr[-300:])


def test_dump_outputs_caps_and_samples_pairs(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "torch", torch)
    flow = torch.arange(10 * 2 * 4 * 8, dtype=torch.float64).reshape(10, 2, 4, 8)
    bench.dump_outputs(str(tmp_path / "whole"), flow)
    whole = np.load(tmp_path / "whole" / "flow.npy")
    assert whole.dtype == np.float32 and np.array_equal(whole, flow.float().numpy())
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 3 * flow[0].numel() * 4)
    bench.dump_outputs(str(tmp_path / "a"), flow)
    bench.dump_outputs(str(tmp_path / "b"), flow)
    a, b = np.load(tmp_path / "a" / "flow.npy"), np.load(tmp_path / "b" / "flow.npy")
    assert a.dtype == np.float32 and a.shape == (3, 2, 4, 8) and np.array_equal(a, b)
    picked = [int(p[0, 0, 0]) // flow[0].numel() for p in a]
    assert picked == sorted(set(picked)) and all(np.array_equal(a[i], whole[k]) for i, k in enumerate(picked))
