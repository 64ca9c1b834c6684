"""Camera fit timings: one JSON line, also written to profiles/camfit_bench.json.

  python tools/camfit_bench.py [--window 0.5] [--out profiles/camfit_bench.json]

Per shape (N points, F frames, 0.3 px noise, the default schedule from the identity): wall_ms_*, fit_cameras with the
data starting in host memory (create, upload, every launch, read-back; the host clock stops after the results are back):
after a warm-up run, as many runs as fill --window seconds (at least 20), reported as minimum, median and maximum;
kernel_ms, the device time of the pass and the step launches from events around them (runs of their own with set_timing,
so the events do not sit in the wall time; minimum and median over the same number of runs), launches = 2 + 2 noiter;
host_ms, fit_cameras_host in the same process, one run. The device result is checked against the host's.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from invcompcamtrack_amd import camfit as F  # noqa: E402

SHAPES = [(2000, 10), (100000, 10)]
CAM = ((1000.0, 1000.0), (640.0, 360.0))
NOISE = 0.3


def scene(n, nframes, seed):
    """X (3, n) at depths 4 .. 12 and xy (F, 2, n): per frame a first-order rotation of 0.05 (f + 1) rad and a translation
    of that length, Gaussian pixel noise."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(4.0, 12.0, n)
    X = np.stack([rng.uniform(-0.5, 0.5, n) * z, rng.uniform(-0.3, 0.3, n) * z, z])
    xy = np.empty((nframes, 2, n))
    for f in range(nframes):
        w, t = rng.normal(size=3), rng.normal(size=3)
        w, t = w / np.linalg.norm(w) * 0.05 * (f + 1), t / np.linalg.norm(t) * 0.05 * (f + 1)
        W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        Xc = (np.eye(3) + W + 0.5 * W @ W) @ X + t[:, None]
        xy[f] = np.stack([CAM[0][0] * Xc[0] / Xc[2] + CAM[1][0], CAM[0][1] * Xc[1] / Xc[2] + CAM[1][1]])
        xy[f] += rng.normal(0, NOISE, (2, n))
    return X, xy


def one(n, nframes, window):
    X, xy = scene(n, nframes, seed=n + nframes)
    dev = F.fit_cameras(X, xy, CAM)  # warm-up; wait() returns after the read-back
    t0 = time.perf_counter()
    dev = F.fit_cameras(X, xy, CAM)
    reps = max(20, min(2000, int(window / max(time.perf_counter() - t0, 1e-6))))
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        dev = F.fit_cameras(X, xy, CAM)
        ts.append(time.perf_counter() - t0)
    f = F.CameraFitter(n, nframes)
    f.set_points(X)
    f.set_observations(xy)
    f.set_camera(CAM)
    f.set_timing(True)
    ks, run_only = [], []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        f.run_async()
        f.wait()
        run_only.append(time.perf_counter() - t0)
        ks.append(f.kernel_times())
    kern = {k: round(min(r[k] for r in ks[1:]), 4) for k in ks[0]}
    kern_med = {k: round(statistics.median(r[k] for r in ks[1:]), 4) for k in ks[0]}
    t0 = time.perf_counter()
    host = F.fit_cameras_host(X, xy, CAM)
    host_s = time.perf_counter() - t0
    same = bool(all(dev[k].tobytes() == host[k].tobytes() for k in ("G", "cost", "damp", "iters", "status", "n")))
    wall = sorted(ts)
    launches = 2 + 2 * F.DEFAULTS["noiter"]
    return dict(n=n, frames=nframes, reps=reps, launches=launches, iters=[int(v) for v in dev["iters"]],
                status=[int(v) for v in dev["status"]], wall_ms_min=round(wall[0] * 1e3, 3),
                wall_ms_median=round(statistics.median(wall) * 1e3, 3), wall_ms_max=round(wall[-1] * 1e3, 3),
                run_wait_ms_median=round(statistics.median(run_only[1:]) * 1e3, 3),
                kernel_ms=kern, kernel_ms_median=kern_med, kernel_ms_sum=round(sum(kern.values()), 4),
                bytes_read_per_pass=40 * n * nframes, host_ms=round(host_s * 1e3, 1),
                speedup_wall_median=round(host_s / statistics.median(wall), 1), same_as_host=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camfit_bench.json"))
    a = ap.parse_args()
    import invcompcamtrack_amd as ic
    if ic.device_count() < 1:
        raise SystemExit("camfit_bench: no HIP device (timings are only taken on the GPU)")
    out = dict(bench="camfit", noise_px=NOISE, schedule=F.DEFAULTS, scene="F frames of growing motion from the identity",
               shapes=[one(n, f, a.window) for n, f in SHAPES])
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
