"""bench.py end to end on the GPU at a small size: a plain run prints the headline line and nothing that takes runs of its
own, and `--full` adds those reports, each of them working."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

SMALL = ["--gpus", "1", "--steps", "1", "--warmup", "1", "--res", "128", "--frames", "16", "--ddim-steps", "2"]
FULL_ONLY = ("flow_decode", "shard_sim", "other_configs", "max_clip_frames", "cpu_baseline")


def run_bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *args], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(tmp_path):
    d = run_bench("--dump-outputs", str(tmp_path))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert k in d, k
    assert d["unit"] == "frames/s" and d["dtype"] == "f32" and d["higher_is_better"] is True and d["config"]["full"] is False
    assert d["value"] == pytest.approx(16 / (d["ms_per_step"] * 1e-3), rel=1e-6)
    assert [k for k in FULL_ONLY if k in d] == [] and "power_ceiling" not in d["roofline"]
    sample = np.load(tmp_path / "sample.npy")
    assert sample.shape == (1, 3, 16, 32, 32) and np.isfinite(sample).all()


@pytest.mark.gpu
def test_full_run_adds_every_report():
    d = run_bench("--full", "--cpu-sample-frames", "2")
    assert d["config"]["full"] is True
    # other_configs belongs to the headline workload (256x256, 200 frames, 50 DDIM steps) only
    for k in ("flow_decode", "shard_sim", "max_clip_frames", "cpu_baseline"):
        assert k in d and "error" not in d[k], (k, d.get(k))
    assert "error" not in d["roofline"]["power_ceiling"] and d["roofline"]["power_ceiling"]["mfma_lds_tflops"] > 0
    assert d["cpu_baseline"]["sample_frames"] == 2 and d["max_clip_frames"]["per_gpu"] > 0
