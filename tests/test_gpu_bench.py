"""bench.py on the GPU at a small size: the plain run's line and what --dump-outputs writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_dump_outputs(tmp_path):
    """--dump-outputs writes the last timed step's decoded bytes: a seeded sample of frames as float32 and a float64 checksum of
    every frame that agrees with the sample; the plain line carries the headline fields and the steps asked for."""
    frames = 20000
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--frames", str(frames), "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    rec = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in rec, k
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["value"] > 0
    assert "roofline" not in rec and "cpu_baseline" not in rec and "configs" not in rec   # --full only

    sample = np.load(tmp_path / "rx_bytes_sample.npy")
    rows = np.load(tmp_path / "rx_bytes_sample_frames.npy")
    chk = np.load(tmp_path / "rx_bytes_frame_checksum.npy")
    assert sample.dtype == np.float32 and rows.dtype == np.float64 and chk.dtype == np.float64
    assert sample.shape == (16384, 576) and rows.shape == (16384,) and chk.shape == (frames,)
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < frames
    assert np.all((sample >= 0) & (sample <= 255) & (sample == np.round(sample)))
    w = np.arange(1, 577, dtype=np.float64)
    assert np.array_equal(sample.astype(np.float64) @ w, chk[rows.astype(np.int64)])
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64 << 20
