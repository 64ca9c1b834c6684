"""Window camera RANSAC timings: one JSON line, also written to profiles/camransac_bench.json.

  python tools/camransac_bench.py [--window 0.5] [--out profiles/camransac_bench.json] [--host-trials 100] [--no-pipeline]

Per shape (N points, F frames, S sides, trials): wall_ms_*, window_ransac with the points and observations starting in
host memory (create, upload, every kernel, read-back; the host clock stops after the results are back): after a warm-up
run, as many runs as fill --window seconds (at least 20), reported as minimum, median and maximum; kernel_ms, the stages'
device time from events between them (hyp, score, select, flags + mask; runs of their own with set_timing, so the events do
not sit in the wall time; minimum and median over the same number of runs); host_ms, window_ransac_host in the same process,
RUN over --host-trials trials and SCALED to the shape's trial count where that is larger (host_scaled says so; its cost per
trial does not depend on the count). The device result is checked against the host's, in the bits, on the trials both ran.
distances_per_s: N F S trials over the score kernel's median time.

pipeline: at the shape of tools/windowcams_bench.py (1242 x 375, bsize 14, every pixel, fields in device memory),
windowcams.ransac_cameras_from_window against windowcams.cameras_from_window on the same counted window, objects reused,
taken in turn; the fit's iterations per frame of both are reported beside the wall times.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from invcompcamtrack_amd import camransac as R  # noqa: E402

SHAPES = [(2000, 10, 2, 100), (100000, 10, 2, 100), (100000, 10, 2, 2000)]
THRESH = 2.0
CAM = ((1000.0, 1000.0), (640.0, 360.0))
OFFSET = (-0.5, 0.0, 0.0)


def scene(n, nframes, static, noise, seed):
    """X (3, n) from the first view's disparity, xy (2, F, 2, n): a camera path that moves on every frame, the right camera
    OFFSET beside the left one, the last share of the points, shuffled, displaced by 30 px in every later frame."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(4.0, 12.0, n)
    Xt = np.stack([rng.uniform(-0.5, 0.5, n) * z, rng.uniform(-0.3, 0.3, n) * z, z])
    moving = np.zeros(n, bool)
    moving[rng.permutation(n)[:int(round((1.0 - static) * n))]] = True
    (fx, fy), (cx, cy) = CAM
    proj = lambda Xc: np.stack([fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy])  # noqa: E731
    xy = np.empty((2, nframes, 2, n))
    step_w, step_t = rng.normal(0, 0.01, 3), np.array([0.06, -0.02, 0.12])
    for f in range(nframes):
        w = step_w * f
        W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        Rm = np.eye(3) + W + 0.5 * W @ W
        for s in range(2):
            p = proj(Rm @ Xt + (step_t * f + s * np.array(OFFSET))[:, None])
            if f > 0:
                ang = rng.uniform(0, 2 * np.pi, n)
                p = p + moving * 30.0 * np.stack([np.cos(ang), np.sin(ang)])
            xy[s, f] = p + rng.normal(0, noise, (2, n))
    d = OFFSET[0] * fx / (xy[1, 0, 0] - xy[0, 0, 0])
    X = np.stack([(xy[0, 0, 0] - cx) / fx * d, (xy[0, 0, 1] - cy) / fy * d, d])
    return X, xy


def same(a, b):
    return bool(a["best_trial"] == b["best_trial"] and a["best_count"] == b["best_count"]
                and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("draws", "G", "p", "words", "dd")))


def one(n, nframes, nsides, trials, window, host_trials):
    X, xy = scene(n, nframes, 0.7, 0.3, seed=n + trials)
    run = lambda nt: R.window_ransac(X, xy, CAM, OFFSET, None, nt, THRESH, 0)  # noqa: E731
    run(trials)  # warm-up; wait() returns after the read-back
    t0 = time.perf_counter()
    dev = run(trials)
    reps = max(20, min(2000, int(window / max(time.perf_counter() - t0, 1e-6))))
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        dev = run(trials)
        ts.append(time.perf_counter() - t0)
    r = R.CameraRansac(n, nframes, nsides)
    r.set_points(X)
    r.set_observations(xy)
    r.set_camera(CAM)
    r.set_offset(OFFSET)
    r.set_timing(True)
    ks = []
    for _ in range(reps + 1):
        r.run_async(trials, THRESH, 0)
        r.wait()
        ks.append(r.kernel_times())
    kern = {k: round(min(q[k] for q in ks[1:]), 4) for k in ks[0]}
    kern_med = {k: round(statistics.median(q[k] for q in ks[1:]), 4) for k in ks[0]}
    ht = min(host_trials, trials)
    t0 = time.perf_counter()
    host = R.window_ransac_host(X, xy, CAM, OFFSET, None, ht, THRESH, 0)
    host_s = (time.perf_counter() - t0) * trials / ht
    ok = same(dev if ht == trials else run(ht), host)
    wall = sorted(ts)
    return dict(n=n, frames=nframes, sides=nsides, trials=trials, reps=reps, chunk=r.chunk,
                wall_ms_min=round(wall[0] * 1e3, 3), wall_ms_median=round(statistics.median(wall) * 1e3, 3),
                wall_ms_max=round(wall[-1] * 1e3, 3), kernel_ms=kern, kernel_ms_median=kern_med,
                kernel_ms_sum=round(sum(kern.values()), 4),
                distances_per_s=round(n * nframes * nsides * trials / (kern_med["score"] * 1e-3), 0),
                host_ms=round(host_s * 1e3, 1), host_trials_run=ht, host_scaled=ht != trials,
                speedup_wall_median=round(host_s / statistics.median(wall), 1), best_trial=dev["best_trial"],
                best_count=dev["best_count"], same_as_host=ok)


def spread(ts):
    ts = sorted(ts)
    return dict(min=round(ts[0] * 1e3, 3), median=round(statistics.median(ts) * 1e3, 3), max=round(ts[-1] * 1e3, 3))


def pipeline(reps):
    import torch

    import stereotrack_bench as SB
    import windowcams_bench as WB
    from invcompcamtrack_amd import stereotrack as S
    from invcompcamtrack_amd import windowcams as W
    dev_args = [torch.from_numpy(x).cuda() for x in SB.scene()]
    torch.cuda.synchronize()
    lr, rl, fl, fr = dev_args
    win = S.StereoTrackWindow(SB.W, SB.H, SB.BSIZE)
    win.open(S.field(lr[0], -1), rl[0])
    for k in range(1, SB.BSIZE):
        win.advance(fl[k - 1][0], fl[k - 1][1], fr[k - 1][0], fr[k - 1][1], S.field(lr[k], -1), rl[k])
    win.count()
    obj_a, obj_b = {}, {}
    ways = (("cameras_from_window", lambda: W.cameras_from_window(win, WB.CAM, WB.BASELINE, objects=obj_a)),
            ("ransac_cameras_from_window", lambda: W.ransac_cameras_from_window(win, WB.CAM, WB.BASELINE, objects=obj_b)))
    res = {name: fn() for name, fn in ways}  # warm-up
    ts = {name: [] for name, _ in ways}
    for _ in range(reps):
        for name, fn in ways:
            t0 = time.perf_counter()
            fn()
            ts[name].append(time.perf_counter() - t0)
    out = dict(w=SB.W, h=SB.H, bsize=SB.BSIZE, kept=res["cameras_from_window"]["m"], ntrials=100, reps=reps)
    for name, _ in ways:
        q = res[name]
        out[name] = dict(wall_ms=spread(ts[name]), inliers=int(q["best_count"]), fit_iters=[int(v) for v in q["iters"]],
                         fit_status=[int(v) for v in q["status"]],
                         err_left_last=float(q["err_left"][-1]), err_right_last=float(q["err_right"][-1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camransac_bench.json"))
    ap.add_argument("--host-trials", type=int, default=100)
    ap.add_argument("--no-pipeline", action="store_true")
    a = ap.parse_args()
    import invcompcamtrack_amd as ic
    if ic.device_count() < 1:
        raise SystemExit("camransac_bench: no HIP device (timings are only taken on the GPU)")
    out = dict(bench="camransac", thresh=THRESH, scene="stereo windows, 70 % static, 0.3 px noise", shapes=[])
    for n, f, s, t in SHAPES:
        out["shapes"].append(one(n, f, s, t, a.window, a.host_trials))
        print("[camransac_bench]", json.dumps(out["shapes"][-1]), flush=True)
    if not a.no_pipeline:
        out["pipeline"] = pipeline(7)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
