"""RANSAC pose sampling timings: one JSON line.

  python tools/ransac_bench.py [--reps 3] [--no-e2e] [--sweep profiles/ransac_sweep.json]

hyp_*: the hypothesis stage (sample_poses: create, upload, every chunk, read-back; the host clock stops after the
results are back) against sample_poses_host, nsamples 500, maxtrials 50 000 (run_ransac_test.m:67,84), at N = 300
with 80 % inliers and N = 2000 with 35 % inliers. e2e_*: fit_cameras_odom with 5 + 5 frames (run_ransac_test.m:76),
hypotheses and verification, at 640x480 and 1920x1080. --sweep: device times over chunk sizes (ICTR_RANSAC_CHUNK) and
score tiles (ICTR_RANSAC_TILE) at both N, written as JSON.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from invcompcamtrack_amd import ransac as R  # noqa: E402
from invcompcamtrack_amd import synth  # noqa: E402

FC, CC, WH = [800.0, 780.0], [320.0, 240.0], (640, 480)
NS, MT = 500, 50000


def matches(n, ratio, seed):
    rng = np.random.default_rng(seed)
    Xc = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 9, n)], 0)
    x = np.stack([FC[0] * Xc[0] / Xc[2] + CC[0], FC[1] * Xc[1] / Xc[2] + CC[1]], 0) + rng.normal(0, 0.3, (2, n))
    nout = n - int(round(ratio * n))
    out = rng.permutation(n)[:nout]
    x[:, out] = np.stack([rng.uniform(0, WH[0], nout), rng.uniform(0, WH[1], nout)], 0)
    return x, Xc


def time_device(x, X, thr, reps):
    import torch
    ts = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        r = R.sample_poses(x, X, FC, CC, NS, MT, thr)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts[1:]), r


def hyp(n, ratio, reps):
    x, X = matches(n, ratio, seed=n)
    thr = float(np.hypot(*WH)) / 100.0
    dev_s, d = time_device(x, X, thr, reps)
    t0 = time.perf_counter()
    h = R.sample_poses_host(x, X, FC, CC, NS, MT, thr)
    host_s = time.perf_counter() - t0
    same = bool(np.array_equal(d["trials"], h["trials"]) and d["trials_used"] == h["trials_used"])
    return dict(n=n, inlier_ratio=ratio, device_ms=round(dev_s * 1e3, 3), host_ms=round(host_s * 1e3, 1),
                speedup=round(host_s / dev_s, 1), samples=len(d["p"]), accepted=d["accepted"],
                trials_used=d["trials_used"], same_as_host=same)


def e2e(w, h, reps):
    pref = np.array([0.02, -0.03, 0.05, 0.01, -0.02, 0.015])
    step = np.array([0.02, 0.01, 0.0, 0.002, -0.002, 0.0])
    poses = [pref + (k - 5) * step for k in range(11)]
    sq = synth.make_sequence(w, h, poses, 5, 300, seed=5)
    rng = np.random.default_rng(6)
    pt2d = np.concatenate([sq["px_ref"], np.stack([rng.uniform(0, w, 300), rng.uniform(0, h, 300)], 1)], 0)
    pt3d = np.concatenate([sq["pts3d"], sq["pts3d"][rng.permutation(300)] + rng.normal(0, 0.5, (300, 3))], 0)
    op = dict(lv_f=4, lv_l=0, psz=8, maxiter=10, normdp_ratio=0.01, donorm=1, dopatchnorm=0, maxpttrack=0, verbosity=0)
    cam = dict(fc=sq["fc"], cc=sq["cc"], wh=sq["wh"])
    thr = float(np.hypot(w, h)) / 100.0
    ts = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        res = R.fit_cameras_odom(pt2d, pt3d, cam, NS, MT, thr, op, (5, 5), sq["frames"])
        ts.append(time.perf_counter() - t0)
    err = float(np.abs(res["p_best"][5] - poses[5]).max()) if res["best"] is not None else None
    return dict(wh=[w, h], frames=11, matches=600, ms=round(min(ts[1:]) * 1e3, 1), samples=len(res["res_corr"]),
                best=res["best"], ref_pose_err=err)


def sweep(path, reps):
    import torch
    rows = []
    for n, ratio in ((300, 0.8), (2000, 0.35)):
        x, X = matches(n, ratio, seed=n)
        thr = float(np.hypot(*WH)) / 100.0
        for chunk in (1024, 2048, 4096, 8192, 16384):
            for tile in (16, 32, 64):
                os.environ["ICTR_RANSAC_CHUNK"], os.environ["ICTR_RANSAC_TILE"] = str(chunk), str(tile)
                ts = []
                for _ in range(reps + 1):
                    t0 = time.perf_counter()
                    R.sample_poses(x, X, FC, CC, NS, MT, thr)
                    torch.cuda.synchronize()
                    ts.append(time.perf_counter() - t0)
                rows.append(dict(n=n, inlier_ratio=ratio, chunk=chunk, tile=tile, ms=round(min(ts[1:]) * 1e3, 3)))
    os.environ.pop("ICTR_RANSAC_CHUNK")
    os.environ.pop("ICTR_RANSAC_TILE")
    with open(path, "w") as f:
        json.dump(dict(what="sample_poses wall time (min of reps), nsamples 500, maxtrials 50000", rows=rows), f,
                  indent=1)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--sweep", default=None)
    a = ap.parse_args()
    import invcompcamtrack_amd as ic
    if ic.device_count() < 1:
        raise SystemExit("ransac_bench: no HIP device (timings are only taken on the GPU)")
    out = dict(bench="ransac", hyp=[hyp(300, 0.8, a.reps), hyp(2000, 0.35, a.reps)])
    if not a.no_e2e:
        out["e2e"] = [e2e(640, 480, a.reps), e2e(1920, 1080, a.reps)]
    if a.sweep:
        rows = sweep(a.sweep, a.reps)
        best = {}
        for r in rows:
            if r["n"] not in best or r["ms"] < best[r["n"]]["ms"]:
                best[r["n"]] = r
        out["sweep_best"] = list(best.values())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
