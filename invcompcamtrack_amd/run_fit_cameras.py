"""One camera per frame of a track window (run_test_OF_track.py:360-411):

  python -m invcompcamtrack_amd.run_fit_cameras in.npz out.npz [--host] [--stereo] [--noiter 20] [--minres 1e-5]
                                                [--ntrials 100] [--thresh 2.0] [--seed 0]

in.npz holds ``X`` (3, N), ``xy`` (F, 2, N), ``fc`` (2,), ``cc`` (2,) and optionally ``mask`` (bool (N,) or the inlier
words of the static split) and ``init`` (F, 3, 4). With --stereo it holds the script's block ``xy_t`` (N, 4, bsize) = left
x, y, right x, y per frame, ``fc``, ``cc`` and ``baseline`` (P1[0, 3] of the script), and the chain of the script runs:
static split -> depth from the first frame's disparity -> fit on the inliers in the left camera -> the mean reprojection
error per frame in the left and in the right camera, printed as the script prints them. out.npz: ``G`` (F, 3, 4), ``p``
(F, 6), ``cost``, ``damp``, ``iters``, ``status``, ``n``, ``reproj`` (F,) (with --stereo also ``reproj_right``, ``inliers``,
``rows``). The fit and the reprojection run on the GPU; --host runs the host restatements instead (same bits).
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from . import camfit as F
from .fsplit import pairs_from_stereo_tracks, split_static, split_static_host


def frame_lines(res, reproj):
    """One line per frame, as tests/cxx/camfit_driver.cpp prints them."""
    out = []
    for f in range(len(res["status"])):
        out.append("frame %d: status %d iters %d n %d cost %.17g damp %.17g reproj %.17g G %s"
                   % (f, res["status"][f], res["iters"][f], res["n"][f], res["cost"][f], res["damp"][f], reproj[f],
                      " ".join("%.17g" % v for v in res["G"][f].reshape(12))))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m invcompcamtrack_amd.run_fit_cameras", description=__doc__.split("\n")[0])
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--stereo", action="store_true")
    ap.add_argument("--noiter", type=int, default=F.DEFAULTS["noiter"])
    ap.add_argument("--minres", type=float, default=F.DEFAULTS["minres"])
    ap.add_argument("--ntrials", type=int, default=100)
    ap.add_argument("--thresh", type=float, default=2.0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(sys.argv[1:] if argv is None else list(argv))
    fit = F.fit_cameras_host if a.host else F.fit_cameras
    reproj = F.reprojection_errors_host if a.host else F.reprojection_errors
    sched = dict(noiter=a.noiter, minres=a.minres)
    with np.load(a.input) as z:
        cam = (np.asarray(z["fc"], np.float64), np.asarray(z["cc"], np.float64))
        if a.stereo:
            xy_t = np.asarray(z["xy_t"], np.float64)
            pairs, rows = pairs_from_stereo_tracks(xy_t)
            split = (split_static_host if a.host else split_static)(pairs, a.ntrials, a.thresh, a.seed)
            xy_t = xy_t[rows]
            baseline = float(z["baseline"])
            X = F.points_from_first_view(xy_t, cam, F.depth_from_disparity(xy_t, cam[0][0], baseline))
            left, right = F.observations_from_stereo_tracks(xy_t)
            res = fit(X, left, cam, mask=split["words"], **sched)
            err_l, _ = reproj(X, left, cam, res["G"], mask=split["words"])
            err_r, _ = reproj(X, right, cam, res["G"], mask=split["words"], offset=[baseline, 0.0, 0.0])
            np.savez(a.output, reproj=err_l, reproj_right=err_r, inliers=rows[split["inliers"]], rows=rows,
                     **{k: res[k] for k in ("G", "p", "cost", "damp", "iters", "status", "n")})
            for f in range(len(err_l)):
                print("[%.17g, %.17g]" % (err_l[f], err_r[f]))
            return 0
        X, xy = z["X"], z["xy"]
        mask = z["mask"] if "mask" in z else None
        init = z["init"] if "init" in z else None
    res = fit(X, xy, cam, mask=mask, init=init, **sched)
    err, _ = reproj(X, xy, cam, res["G"], mask=mask)
    np.savez(a.output, reproj=err, **{k: res[k] for k in ("G", "p", "cost", "damp", "iters", "status", "n")})
    print("\n".join(frame_lines(res, err)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
