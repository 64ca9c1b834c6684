"""Window hand-over timings: one JSON line, also written to profiles/windowcams_bench.json.

  python tools/windowcams_bench.py [--reps 7] [--no-host] [--out profiles/windowcams_bench.json]

The workload of tools/stereotrack_bench.py (KITTI size 1242 x 375, bsize 14, every pixel) carried on to one camera per
frame, at ntrials 100 and 2000, with the fields starting in host and in device memory. Per combination, after a warm-up of
each, --reps runs of each taken in turn in the same process, wall clock around the whole call (each ends in a device wait),
as minimum, median and maximum:
  a        windowcams.window_cameras with its window, splitter and fitter reused (the hand-over);
  a_fresh  the same with a new splitter and fitter per call, as b makes them;
  b        the same result through the host-array functions: stereo_track_window -> pairs_from_stereo_tracks ->
           split_static -> depth_from_disparity, points_from_first_view, observations_from_stereo_tracks -> fit_cameras ->
           two reprojection_errors (windowcams.cameras_from_tracks), its window reused;
stages_ms_median_*: one pass of each way with the host clock read between its stages; handover_kernels: device time of the
three kernels from events around their launches in runs of their own, the bytes each moves and the rate; host_ms: c,
windowcams.window_cameras_host once at ntrials 100, not scaled. a, b (and c) are compared byte for byte.
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

import stereotrack_bench as SB  # noqa: E402
from invcompcamtrack_amd import camfit as F  # noqa: E402
from invcompcamtrack_amd import fsplit  # noqa: E402
from invcompcamtrack_amd import stereotrack as S  # noqa: E402
from invcompcamtrack_amd import windowcams as WCAM  # noqa: E402

CAM = ((718.856, 718.856), (607.1928, 185.2157))
BASELINE = -0.54
KEYS = ("m", "words", "best_trial", "best_count", "draws", "F", "dd", "G", "cost", "damp", "iters", "status", "n", "err_left",
        "err_right")


def spread(ts):
    ts = sorted(ts)
    return dict(min=round(ts[0] * 1e3, 3), median=round(statistics.median(ts) * 1e3, 3), max=round(ts[-1] * 1e3, 3))


def same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in KEYS)


def way_b(fields, win, nt):
    xy_t, _ = S.stereo_track_window(*fields, window=win)
    return WCAM.cameras_from_tracks(xy_t, CAM, BASELINE, ntrials=nt)


def stages_b(fields, win, nt):
    """way b with the host clock read between its stages (seconds)."""
    t = [time.perf_counter()]
    xy_t, _ = S.stereo_track_window(*fields, window=win)
    t.append(time.perf_counter())
    pairs, rows = fsplit.pairs_from_stereo_tracks(xy_t)
    t.append(time.perf_counter())
    split = fsplit.split_static(pairs, nt)
    t.append(time.perf_counter())
    xy = xy_t[rows]
    X = F.points_from_first_view(xy, CAM, F.depth_from_disparity(xy, CAM[0][0], BASELINE))
    left, right = F.observations_from_stereo_tracks(xy)
    t.append(time.perf_counter())
    fit = F.fit_cameras(X, left, CAM, mask=split["words"])
    t.append(time.perf_counter())
    F.reprojection_errors(X, left, CAM, fit["G"], mask=split["words"])
    F.reprojection_errors(X, right, CAM, fit["G"], mask=split["words"], offset=[BASELINE, 0.0, 0.0])
    t.append(time.perf_counter())
    names = ("window_and_read", "pairs_numpy", "split_static", "points_obs_numpy", "fit_cameras", "two_reprojections")
    return dict(zip(names, np.diff(t)))


def stages_a(fields, win, objects, nt):
    """way a with the host clock read between its stages (seconds); the calls of window_cameras and cameras_from_window."""
    lr, rl, fl, fr = fields
    t = [time.perf_counter()]
    win.open(S.field(lr[0], -1), rl[0])
    for k in range(1, SB.BSIZE):
        win.advance(fl[k - 1][0], fl[k - 1][1], fr[k - 1][0], fr[k - 1][1], S.field(lr[k], -1), rl[k])
    win.count()
    t.append(time.perf_counter())
    split, fit = objects["split"], objects["fit"]
    split.set_pairs_from_window(win)
    split.run_async(nt, 2.0, 0)
    fit.set_camera(CAM)
    fit.set_points_from_window(win, BASELINE)
    fit.set_observations_from_window(win, right=False)
    fit.set_mask_from_fsplit(split)
    fit.run_async()
    t.append(time.perf_counter())
    split.wait()
    t.append(time.perf_counter())
    f = fit.wait()
    t.append(time.perf_counter())
    fit.reprojection_errors(f["G"])
    fit.set_observations_from_window(win, right=True)
    fit.reprojection_errors(f["G"], [BASELINE, 0.0, 0.0])
    t.append(time.perf_counter())
    names = ("window_and_count", "handover_and_enqueue", "wait_split", "wait_fit", "two_reprojections")
    return dict(zip(names, np.diff(t)))


def median_stages(runs):
    return {k: round(statistics.median(r[k] for r in runs) * 1e3, 3) for k in runs[0]}


def handover_kernels(win, objects, reps):
    """Device ms of the three kernels from events on the null stream, min and median, with the bytes they move."""
    import torch
    split, fit = objects["split"], objects["fit"]
    m, b = win.survivors, win.bsize
    npairs = b // 2
    calls = (("k_ho_pairs", lambda: split.set_pairs_from_window(win)),
             ("k_ho_points", lambda: fit.set_points_from_window(win, BASELINE)),
             ("k_ho_obs_left", lambda: fit.set_observations_from_window(win, right=False)),
             ("k_ho_obs_right", lambda: fit.set_observations_from_window(win, right=True)))
    moved = dict(k_ho_pairs=(32 * m * 2 * npairs + 8 * m * 2 * npairs, 32 * m * 2 * npairs),
                 k_ho_points=(24 * m + 8 * m, 24 * m),
                 k_ho_obs_left=(16 * m * b + 8 * m * b, 16 * m * b), k_ho_obs_right=(16 * m * b + 8 * m * b, 16 * m * b))
    ms = {name: [] for name, _ in calls}
    for _ in range(reps + 1):  # the first is the warm-up
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)]
        ev[0].record()
        for k, (_, fn) in enumerate(calls):
            fn()
            ev[k + 1].record()
        torch.cuda.synchronize()
        for k, (name, _) in enumerate(calls):
            ms[name].append(ev[k].elapsed_time(ev[k + 1]))
    out = {}
    for name, v in ms.items():
        v = v[1:]
        rd, wr = moved[name]
        med = statistics.median(v)
        out[name] = dict(ms_min=round(min(v), 4), ms_median=round(med, 4), bytes_read=rd, bytes_written=wr,
                         tb_per_s_at_median=round((rd + wr) / (med * 1e-3) / 1e12, 3))
    total = sum(statistics.median(v[1:]) for v in ms.values())
    model = (32 * m * b + 8 * m) + (32 * m * 2 * npairs + 2 * 16 * m * b + 24 * m)
    out["all"] = dict(ms_median_sum=round(total, 4), bytes_moved=sum(sum(x) for x in moved.values()),
                      fused_model_bytes=model, fused_model_tb_per_s=round(model / (total * 1e-3) / 1e12, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "windowcams_bench.json"))
    a = ap.parse_args()
    import invcompcamtrack_amd as ic
    if ic.device_count() < 1:
        raise SystemExit("windowcams_bench: no HIP device (timings are only taken on the GPU)")
    import torch
    args = SB.scene()
    dev_args = [torch.from_numpy(x).cuda() for x in args]
    torch.cuda.synchronize()
    win_a, win_b, objects = S.StereoTrackWindow(SB.W, SB.H, SB.BSIZE), S.StereoTrackWindow(SB.W, SB.H, SB.BSIZE), {}
    out, results = {}, {}
    for nt in (100, 2000):
        for where, fields in (("host_fields", args), ("device_fields", dev_args)):
            ways = (("a", lambda: WCAM.window_cameras(*fields, CAM, BASELINE, ntrials=nt, window=win_a, objects=objects)),
                    ("a_fresh", lambda: WCAM.window_cameras(*fields, CAM, BASELINE, ntrials=nt, window=win_a)),
                    ("b", lambda: way_b(fields, win_b, nt)))
            ts = {name: [] for name, _ in ways}
            for name, fn in ways:  # warm-up
                results[(nt, name)] = fn()
            for _ in range(a.reps):
                for name, fn in ways:
                    t0 = time.perf_counter()
                    fn()
                    ts[name].append(time.perf_counter() - t0)
            tag = "ntrials_%d_%s" % (nt, where)
            out["wall_ms_" + tag] = {name: spread(v) for name, v in ts.items()}
            out["wall_ms_" + tag]["b_over_a_median"] = round(statistics.median(ts["b"]) / statistics.median(ts["a"]), 3)
            out["stages_ms_median_a_" + tag] = median_stages([stages_a(fields, win_a, objects, nt) for _ in range(a.reps)])
            out["stages_ms_median_b_" + tag] = median_stages([stages_b(fields, win_b, nt) for _ in range(a.reps)])
            print("[windowcams_bench]", tag, json.dumps(out["wall_ms_" + tag]), flush=True)
        out["a_same_as_b_ntrials_%d" % nt] = bool(same(results[(nt, "a")], results[(nt, "b")])
                                                  and same(results[(nt, "a_fresh")], results[(nt, "b")]))
    kernels = handover_kernels(win_a, objects, a.reps)
    r = results[(100, "a")]
    head = dict(bench="windowcams", w=SB.W, h=SB.H, bsize=SB.BSIZE, points=SB.W * SB.H, kept=r["m"], reps=a.reps,
                static_ntrials_100=r["best_count"], fit_status=[int(v) for v in r["status"]],
                fit_iters=[int(v) for v in r["iters"]],
                xy_t_bytes=32 * r["m"] * SB.BSIZE, pairs_bytes=32 * r["m"] * 2 * (SB.BSIZE // 2),
                observations_bytes_per_side=16 * r["m"] * SB.BSIZE)
    def write(res):
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        return res

    res = write(dict(**head, **out, handover_kernels=kernels))
    if not a.no_host:  # last: the slow part; what was measured is on disk already
        print("[windowcams_bench] the host definition, once ...", flush=True)
        t0 = time.perf_counter()
        host = WCAM.window_cameras_host(*args, CAM, BASELINE, ntrials=100)
        head.update(host_ms=round((time.perf_counter() - t0) * 1e3, 1), host_ntrials=100, host_scaled=False,
                    a_same_as_host=bool(same(r, host)))
        res = write(dict(**head, **out, handover_kernels=kernels))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
