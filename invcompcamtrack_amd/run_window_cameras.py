"""Dense fields of a stereo sequence to one camera per frame (run_test_OF_track.py:170-223, 309-343, 360-411):

  python -m invcompcamtrack_amd.run_window_cameras in.npz out.npz [--host] [--ntrials 100] [--thresh 2.0] [--seed 0]
         [--tracks] [--th_ratio 0.2] [--th_abs 1.0]

in.npz holds the keys of run_stereo_track --fields: ``disp_lr``, ``disp_rl`` (bsize, H, W), ``flow_l``, ``flow_r``
(>= bsize-1, 2 = fwd / bwd, H, W, 2), optionally ``xy0`` (N, 2); and ``fc`` (2,), ``cc`` (2,), ``baseline`` (P1[0, 3] of the
script). The checked window, the static split, the camera fit and both reprojection means run on the GPU and the window
stays there (windowcams.window_cameras); --host runs the host definition instead (same bits). out.npz holds the result
dict of windowcams: ``m``, ``words``, ``mask``, ``inliers``, ``best_trial``, ``best_count``, ``draws``, ``F``, ``dd``,
``G``, ``p``, ``cost``, ``damp``, ``iters``, ``status``, ``n``, ``err_left``, ``err_right``, and with --tracks ``xy_t`` and
``rows``. The two means are printed per frame as the script prints them.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from . import windowcams as W


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m invcompcamtrack_amd.run_window_cameras", description=__doc__.split("\n")[0])
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--ntrials", type=int, default=100)
    ap.add_argument("--thresh", type=float, default=2.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tracks", action="store_true")
    ap.add_argument("--th_ratio", type=float, default=0.2)
    ap.add_argument("--th_abs", type=float, default=1.0)
    a = ap.parse_args(sys.argv[1:] if argv is None else list(argv))
    with np.load(a.input) as z:
        lr, rl, fl, fr = z["disp_lr"], z["disp_rl"], z["flow_l"], z["flow_r"]
        xy0 = z["xy0"] if "xy0" in z else None
        cam = (np.asarray(z["fc"], np.float64), np.asarray(z["cc"], np.float64))
        baseline = float(z["baseline"])
    fn = W.window_cameras_host if a.host else W.window_cameras
    try:
        res = fn(lr, rl, fl, fr, cam, baseline, xy0=xy0, th_ratio=a.th_ratio, th_abs=a.th_abs, ntrials=a.ntrials,
                 thresh=a.thresh, seed=a.seed, tracks=a.tracks)
    except ValueError as exc:
        print(exc, file=sys.stderr)
        return 2
    np.savez(a.output, **res)
    print("kept %d points in %d frames, %d static" % (res["m"], len(res["status"]), res["best_count"]))
    for f in range(len(res["err_left"])):
        print("[%.17g, %.17g]" % (res["err_left"][f], res["err_right"][f]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
