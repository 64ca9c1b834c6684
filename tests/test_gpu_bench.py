"""bench.py on one GPU at a small size: a plain run carries the headline only, --full adds the checks and extra
measurements, and --dump-outputs writes the timed path's poses -- the same poses with and without --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "2", "--width", "640",
                        "--height", "384", "--steps", "3", "--warmup", "1", "--no-secondary"] + extra,
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.timeout(900)
def test_plain_and_full_runs_dump_the_same_poses(tmp_path):
    plain = _bench(["--dump-outputs", str(tmp_path / "plain")])
    full = _bench(["--full", "--cpu-seconds", "0.2", "--dump-outputs", str(tmp_path / "full")])
    for out in (plain, full):
        assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0
        assert out["value"] > 0 and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert "roofline" not in plain and plain["cpu_baseline"] is None and plain["pose_err_vs_cpu"] is None
    assert "roofline" in full and full["cpu_baseline"] is not None and full["pose_err_vs_cpu"] <= 1e-4
    a, b = np.load(tmp_path / "plain" / "poses.npy"), np.load(tmp_path / "full" / "poses.npy")
    assert a.dtype == np.float64 and a.shape == (2, 6) and np.isfinite(a).all()
    assert np.array_equal(a, b)   # seeded inputs, same timed path
