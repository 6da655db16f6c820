"""CPU: `python bench.py --gpus N` must start its own N ranks (the driver's command shape)."""
import json
import os
import subprocess
import sys

from conftest import ROOT


def test_bench_self_launches_two_ranks_dry_run():
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        env.pop(k, None)
    for mode in ("denoise", "train"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run", "--mode", mode],
                             capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, out.stdout                  # rank 0 only
        rec = json.loads(lines[0])
        assert rec == {"dry_run": True, "n_gpus": 2, "ranks_seen": 2, "mode": mode}


def test_bench_single_rank_dry_run_needs_no_launcher():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-run"], capture_output=True, text=True,
                         timeout=120, cwd=ROOT)
    assert out.returncode == 0 and json.loads(out.stdout.strip().splitlines()[-1])["ranks_seen"] == 1


def test_dump_outputs_writes_float32_npy_and_a_fixed_parameter_sample(tmp_path):
    """`--dump-outputs DIR`: every array lands as DIR/<name>.npy in float32; the training line's parameter sample is the same
    elements of the same parameters on every run."""
    import numpy as np
    import torch
    import bench
    bench.dump_outputs(str(tmp_path / "out"), {"latents": torch.arange(6, dtype=torch.bfloat16).view(2, 3)})
    a = np.load(tmp_path / "out" / "latents.npy")
    assert a.dtype == np.float32 and a.tolist() == [[0, 1, 2], [3, 4, 5]]
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(300, 40), torch.nn.Linear(40, 3))
    s1, s2 = bench.param_sample(m), bench.param_sample(m)
    assert s1.dtype == torch.float32 and s1.numel() == 256 + 40 + 120 + 3 and torch.equal(s1, s2)
