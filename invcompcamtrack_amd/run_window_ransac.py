"""Dense fields of a stereo sequence to one camera per frame through the window camera RANSAC (run_test_OF_track.py:170-223,
360-411 and the script's TODO 1):

  python -m invcompcamtrack_amd.run_window_ransac in.npz out.npz [--host] [--ntrials 100] [--thresh 2.0] [--seed 0]
         [--bundle] [--tracks] [--th_ratio 0.2] [--th_abs 1.0]

in.npz holds the keys of run_window_cameras: ``disp_lr``, ``disp_rl`` (bsize, H, W), ``flow_l``, ``flow_r`` (>= bsize-1,
2 = fwd / bwd, H, W, 2), optionally ``xy0`` (N, 2); and ``fc`` (2,), ``cc`` (2,), ``baseline`` (P1[0, 3] of the script). The
checked window, the RANSAC over both cameras, the camera fit from its poses on its inliers and both reprojection means run
on the GPU and the window stays there (windowcams.ransac_cameras); --host runs the host definition instead (same bits).
out.npz holds ``m``, the RANSAC's ``words``, ``mask``, ``inliers``, ``best_trial``, ``best_count``, ``draws``, ``dd``,
``G_ransac``, ``p_ransac``, the fit's ``G``, ``p``, ``cost``, ``damp``, ``iters``, ``status``, ``n``, ``err_left``,
``err_right``; with --bundle the adjustment's result as ``ba_G``, ``ba_p``, ``ba_X``, ``ba_cost``, ``ba_damp``,
``ba_iters``, ``ba_status``, ``ba_n`` (absent when no trial succeeded) and ``err_left_ba``, ``err_right_ba``; with --tracks
``xy_t`` and ``rows``. The two means are printed per frame as the script prints them.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from . import windowcams as W


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m invcompcamtrack_amd.run_window_ransac", description=__doc__.split("\n")[0])
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--ntrials", type=int, default=100)
    ap.add_argument("--thresh", type=float, default=2.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--bundle", action="store_true")
    ap.add_argument("--tracks", action="store_true")
    ap.add_argument("--th_ratio", type=float, default=0.2)
    ap.add_argument("--th_abs", type=float, default=1.0)
    a = ap.parse_args(sys.argv[1:] if argv is None else list(argv))
    with np.load(a.input) as z:
        lr, rl, fl, fr = z["disp_lr"], z["disp_rl"], z["flow_l"], z["flow_r"]
        xy0 = z["xy0"] if "xy0" in z else None
        cam = (np.asarray(z["fc"], np.float64), np.asarray(z["cc"], np.float64))
        baseline = float(z["baseline"])
    fn = W.window_ransac_cameras_host if a.host else W.ransac_cameras
    try:
        res = fn(lr, rl, fl, fr, cam, baseline, xy0=xy0, th_ratio=a.th_ratio, th_abs=a.th_abs, ntrials=a.ntrials,
                 thresh=a.thresh, seed=a.seed, bundle=a.bundle, tracks=a.tracks)
    except ValueError as exc:
        print(exc, file=sys.stderr)
        return 2
    ba = res.pop("ba", None)
    if ba is not None:
        res.update({"ba_" + k: v for k, v in ba.items()})
    np.savez(a.output, **res)
    print("kept %d points in %d frames, %d inliers of trial %d" % (res["m"], len(res["status"]), res["best_count"],
                                                                   res["best_trial"]))
    for f in range(len(res["err_left"])):
        print("[%.17g, %.17g]" % (res["err_left"][f], res["err_right"][f]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
