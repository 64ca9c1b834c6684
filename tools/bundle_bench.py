"""Window bundle adjustment timings: one JSON line, also written to profiles/bundle_bench.json.

  python tools/bundle_bench.py [--window 0.5] [--out profiles/bundle_bench.json]

Per shape (N points, F frames, two sides, 0.3 px noise, points with 3 % depth error, the default schedule started from
fit_cameras' poses): wall_ms_*, adjust_window with the data starting in host memory (create, upload, every launch,
read-back of poses and points; the host clock stops after the results are back): after a warm-up run, as many runs as
fill --window seconds (at least 10), reported as minimum, median and maximum; run_wait_ms, run + wait on an object that
exists; kernel_ms, the device time per kernel kind from events around every launch (runs of their own with set_timing, so
the events do not sit in the wall time; minimum and median), launches = 2 + 7 (noiter + 1); host_ms, adjust_window_host
in the same process, one run. The device result is checked against the host's.
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

from invcompcamtrack_amd import bundle as B  # noqa: E402
from invcompcamtrack_amd import camfit as F  # noqa: E402

SHAPES = [(2000, 10), (100000, 10)]
CAM = ((1000.0, 1000.0), (640.0, 360.0))
OFFSET = (-0.5, 0.0, 0.0)
NOISE, DEPTH_ERR = 0.3, 0.03


def scene(n, nframes, seed):
    """X0 (3, n): points at depths 4 .. 12 with a relative depth error; xy (2, F, 2, n): a camera path that starts at the
    identity and moves by a first-order rotation of 0.01 f rad and (0.06, -0.02, 0.12) f per frame, the second side beside
    the first by OFFSET, Gaussian pixel noise."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(4.0, 12.0, n)
    X = np.stack([rng.uniform(-0.5, 0.5, n) * z, rng.uniform(-0.3, 0.3, n) * z, z])
    w0 = rng.normal(0, 0.01, 3)
    xy = np.empty((2, nframes, 2, n))
    for f in range(nframes):
        w, t = w0 * f, np.array([0.06, -0.02, 0.12]) * f
        W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        for s in range(2):
            Xc = (np.eye(3) + W + 0.5 * W @ W) @ X + (t + np.array(OFFSET) * s)[:, None]
            xy[s, f] = np.stack([CAM[0][0] * Xc[0] / Xc[2] + CAM[1][0], CAM[0][1] * Xc[1] / Xc[2] + CAM[1][1]])
            xy[s, f] += rng.normal(0, NOISE, (2, n))
    return X * (1.0 + rng.normal(0, DEPTH_ERR, n)), xy


def one(n, nframes, window):
    X, xy = scene(n, nframes, seed=n + nframes)
    init = F.fit_cameras(X, xy[0], CAM)["G"]
    kw = dict(offset=OFFSET, init=init)
    dev = B.adjust_window(X, xy, CAM, **kw)  # warm-up; wait() returns after the read-back
    t0 = time.perf_counter()
    dev = B.adjust_window(X, xy, CAM, **kw)
    reps = max(10, min(1000, int(window / max(time.perf_counter() - t0, 1e-6))))
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        dev = B.adjust_window(X, xy, CAM, **kw)
        ts.append(time.perf_counter() - t0)
    b = B.BundleAdjuster(n, nframes, 2)
    b.set_points(X)
    b.set_observations(xy)
    b.set_camera(CAM)
    b.set_offset(OFFSET)
    run_only = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        b.run_async(init)
        b.wait()
        run_only.append(time.perf_counter() - t0)
    b.set_timing(True)
    ks = []
    for _ in range(reps + 1):
        b.run_async(init)
        b.wait()
        ks.append(b.kernel_times())
    kern = {k: round(min(r[k] for r in ks[1:]), 4) for k in ks[0]}
    kern_med = {k: round(statistics.median(r[k] for r in ks[1:]), 4) for k in ks[0]}
    t0 = time.perf_counter()
    host = B.adjust_window_host(X, xy, CAM, **kw)
    host_s = time.perf_counter() - t0
    same = bool(all(np.asarray(dev[k]).tobytes() == np.asarray(host[k]).tobytes()
                    for k in ("G", "X", "cost", "damp", "iters", "status", "n")))
    wall = sorted(ts)
    rounds = B.DEFAULTS["noiter"] + 1
    npairs = (nframes - 1) * nframes // 2
    return dict(n=n, frames=nframes, sides=2, reps=reps, launches=2 + 7 * rounds, iters=int(dev["iters"]),
                status=int(dev["status"]), cost=float(dev["cost"]), wall_ms_min=round(wall[0] * 1e3, 3),
                wall_ms_median=round(statistics.median(wall) * 1e3, 3), wall_ms_max=round(wall[-1] * 1e3, 3),
                run_wait_ms_median=round(statistics.median(run_only[1:]) * 1e3, 3),
                kernel_ms=kern, kernel_ms_median=kern_med, kernel_ms_sum=round(sum(kern.values()), 4),
                schur_bytes_per_pass_model=n * npairs * (8 * (3 + 9) + 2 * 2 * 16) + n * npairs // 8,
                schur_pairs=npairs, host_ms=round(host_s * 1e3, 1),
                speedup_wall_median=round(host_s / statistics.median(wall), 1), same_as_host=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bundle_bench.json"))
    a = ap.parse_args()
    import invcompcamtrack_amd as ic
    if ic.device_count() < 1:
        raise SystemExit("bundle_bench: no HIP device (timings are only taken on the GPU)")
    out = dict(bench="bundle", noise_px=NOISE, depth_err=DEPTH_ERR, schedule=B.DEFAULTS,
               scene="two sides, F frames of a camera path from the identity, started from fit_cameras' poses",
               shapes=[one(n, f, a.window) for n, f in SHAPES])
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
