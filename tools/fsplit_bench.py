"""Static split timings: one JSON line, also written to profiles/fsplit_bench.json.

  python tools/fsplit_bench.py [--window 0.5] [--out profiles/fsplit_bench.json] [--host-trials 100]

Per shape (N points, P view pairs, trials): wall_ms_*, split_static with the pairs starting in host memory (create,
upload, every kernel, read-back; the host clock stops after the results are back): after a warm-up run, as many runs as
fill --window seconds (at least 20), reported as minimum, median and maximum; kernel_ms, the stages' device time from
events between them (fit, score, select, mask; runs of their own with set_timing, so the events do not sit in the wall
time; minimum and median over the same number of runs); host_ms, split_static_host in the same process, RUN over
--host-trials rounds and SCALED to the shape's round count where that is larger (host_scaled says so; its cost per round
does not depend on the count). The device result is checked against the host's on the rounds both ran.
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

from invcompcamtrack_amd import fsplit as S  # noqa: E402

SHAPES = [(2000, 10, 100), (100000, 10, 100), (100000, 10, 2000)]
THRESH = 2.0


def scene(n, npairs, static, noise, seed):
    """pairs (npairs, 4, n): camera a at the origin, one camera b per pair, points in front of both; the last share of
    the points, shuffled, displaced by 30 px in image b; Gaussian pixel noise."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(4.0, 20.0, n)
    X = np.stack([rng.uniform(-0.55, 0.55, n) * z, rng.uniform(-0.3, 0.3, n) * z, z])
    moving = np.zeros(n, bool)
    moving[rng.permutation(n)[:int(round((1.0 - static) * n))]] = True
    proj = lambda Xc: np.stack([1000.0 * Xc[0] / Xc[2] + 640.0, 1000.0 * Xc[1] / Xc[2] + 360.0])  # noqa: E731
    pairs = np.empty((npairs, 4, n))
    for p in range(npairs):
        w = rng.normal(0, 0.03, 3)
        W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        t = rng.normal(0, 0.4, 3) + np.array([0.6 if p % 2 == 0 else -0.6, 0.0, 0.0])
        ang = rng.uniform(0, 2 * np.pi, n)
        xb = proj((np.eye(3) + W + 0.5 * W @ W) @ X + t[:, None]) + moving * 30.0 * np.stack([np.cos(ang), np.sin(ang)])
        pairs[p, 0:2] = proj(X) + rng.normal(0, noise, (2, n))
        pairs[p, 2:4] = xb + rng.normal(0, noise, (2, n))
    return pairs


def one(n, p, trials, window, host_trials):
    pairs = scene(n, p, 0.7, 0.3, seed=n + trials)
    t0 = time.perf_counter()
    dev = S.split_static(pairs, trials, THRESH, 0)  # warm-up; wait() returns after the read-back
    t0 = time.perf_counter()
    dev = S.split_static(pairs, trials, THRESH, 0)
    reps = max(20, min(2000, int(window / max(time.perf_counter() - t0, 1e-6))))
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        dev = S.split_static(pairs, trials, THRESH, 0)
        ts.append(time.perf_counter() - t0)
    s = S.StaticSplitter(n, p)
    s.set_pairs(pairs)
    s.set_timing(True)
    ks = []
    for _ in range(reps + 1):
        s.run_async(trials, THRESH, 0)
        s.wait()
        ks.append(s.kernel_times())
    kern = {k: round(min(r[k] for r in ks[1:]), 4) for k in ks[0]}
    kern_med = {k: round(statistics.median(r[k] for r in ks[1:]), 4) for k in ks[0]}
    ht = min(host_trials, trials)
    t0 = time.perf_counter()
    host = S.split_static_host(pairs, ht, THRESH, 0)
    host_s = (time.perf_counter() - t0) * trials / ht
    same = None
    if ht == trials:
        same = bool(dev["best_trial"] == host["best_trial"] and dev["dd"].tobytes() == host["dd"].tobytes()
                    and np.array_equal(dev["words"], host["words"]))
    else:
        d2 = S.split_static(pairs, ht, THRESH, 0)
        same = bool(d2["best_trial"] == host["best_trial"] and d2["dd"].tobytes() == host["dd"].tobytes()
                    and np.array_equal(d2["words"], host["words"]))
    wall = sorted(ts)
    return dict(n=n, pairs=p, trials=trials, reps=reps, wall_ms_min=round(wall[0] * 1e3, 3),
                wall_ms_median=round(statistics.median(wall) * 1e3, 3), wall_ms_max=round(wall[-1] * 1e3, 3),
                kernel_ms=kern, kernel_ms_median=kern_med, kernel_ms_sum=round(sum(kern.values()), 4),
                host_ms=round(host_s * 1e3, 1), host_trials_run=ht, host_scaled=ht != trials,
                speedup_wall_median=round(host_s / statistics.median(wall), 1), best_count=dev["best_count"],
                same_as_host=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fsplit_bench.json"))
    ap.add_argument("--host-trials", type=int, default=100)
    a = ap.parse_args()
    import invcompcamtrack_amd as ic
    if ic.device_count() < 1:
        raise SystemExit("fsplit_bench: no HIP device (timings are only taken on the GPU)")
    out = dict(bench="fsplit", thresh=THRESH, scene="two-camera scenes, 70 % static, 0.3 px noise",
               shapes=[one(n, p, t, a.window, a.host_trials) for n, p, t in SHAPES])
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
