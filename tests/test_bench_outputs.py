"""bench.py --dump-outputs and the plain / --full split: the dump helper writes
float32 .npy files, a fixed sample of an array above its cap (the same positions
in every run); a plain run prints the headline line without the legs that take
runs of their own and writes the last timed step's results."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_outputs_float32_and_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_VALUES", 1000)
    big = torch.arange(5000, dtype=torch.float64).reshape(50, 100)
    small = torch.tensor([[1, -1], [2, 3]], dtype=torch.int64)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.shape == (1000,)
    np.testing.assert_array_equal(a, b)
    assert len(set(a.tolist())) == 1000 and (np.diff(a) > 0).all()     # distinct positions, ascending
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.tolist() == [[1, -1], [2, 3]]


def test_dump_cap_keeps_a_run_under_64_mb():
    # C3 writes loss, params, bn_stats, adam_m: at most 3 large arrays + a scalar
    assert 4 * bench.DUMP_MAX_VALUES * 4 <= 64 * 1024 * 1024


@pytest.mark.gpu
def test_plain_run_prints_the_headline_line_and_dumps(cuda, tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert line["unit"] == "line-crops/sec" and line["dtype"] == "bf16"
    assert abs(line["value"] - 256 * 1e3 / line["ms_per_step"]) <= 0.01 * line["value"]
    for leg in ("cpu_baseline", "c1_latency", "cer_vs_ref", "cer_vs_ref_trained"):
        assert leg not in line                                   # --full's legs
    files = sorted(os.listdir(out))
    assert files == ["adam_m.npy", "bn_stats.npy", "loss.npy", "params.npy"]
    arrays = {f: np.load(out / f) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 1024 * 1024
    assert abs(float(arrays["loss.npy"][0]) - line["loss"]) <= 1e-3 * abs(line["loss"]) + 1e-4
    assert np.abs(arrays["adam_m.npy"]).max() > 0
