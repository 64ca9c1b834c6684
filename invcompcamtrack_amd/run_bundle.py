"""Window bundle adjustment (item 3 of the list that ends run_test_OF_track.py):

  python -m invcompcamtrack_amd.run_bundle in.npz out.npz [--host] [--stereo] [--noiter 20] [--minres 1e-5]
                                           [--ntrials 100] [--thresh 2.0] [--seed 0]

in.npz holds ``X`` (3, N), ``xy`` (S, F, 2, N) or (F, 2, N), ``fc`` (2,), ``cc`` (2,) and optionally ``offset`` (3,),
``mask`` (bool (N,) or the inlier words of the static split) and ``init`` (F, 3, 4). With --stereo it holds the script's
block ``xy_t`` (N, 4, bsize), ``fc``, ``cc`` and ``baseline`` (P1[0, 3] of the script), and the chain runs: static split ->
depth from the first frame's disparity -> one camera per frame on the inliers -> the adjustment of those poses and the
inliers' points over both cameras, with offset (baseline, 0, 0). out.npz: ``G`` (F, 3, 4), ``p`` (F, 6), ``X`` (3, N),
``cost``, ``damp``, ``iters``, ``status``, ``n`` (with --stereo also ``fit_G``, ``inliers``, ``rows``). The printed lines
carry every number as a hexadecimal float. Everything runs on the GPU; --host runs the host restatements instead (same bits).
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from . import bundle as B
from . import camfit as F
from .fsplit import pairs_from_stereo_tracks, split_static, split_static_host

KEYS = ("G", "p", "X", "cost", "damp", "iters", "status", "n")


def hexf(v):
    """printf("%a") of a double."""
    s = float(v).hex()
    if "p" not in s:
        return s
    mant, exp = s.split("p")
    if "." in mant:
        mant = mant.rstrip("0").rstrip(".")
    return mant + "p" + exp


def result_lines(res):
    """The lines of tests/cxx/bundle_driver.cpp: the run, one line per frame, one per point."""
    out = ["status %d iters %d n %d cost %s damp %s" % (res["status"], res["iters"], res["n"], hexf(res["cost"]),
                                                        hexf(res["damp"]))]
    for f, g in enumerate(res["G"]):
        out.append("G %d: %s" % (f, " ".join(hexf(v) for v in g.reshape(12))))
    for m in range(res["X"].shape[1]):
        out.append("X %d: %s" % (m, " ".join(hexf(v) for v in res["X"][:, m])))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m invcompcamtrack_amd.run_bundle", description=__doc__.split("\n")[0])
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--stereo", action="store_true")
    ap.add_argument("--noiter", type=int, default=B.DEFAULTS["noiter"])
    ap.add_argument("--minres", type=float, default=B.DEFAULTS["minres"])
    ap.add_argument("--ntrials", type=int, default=100)
    ap.add_argument("--thresh", type=float, default=2.0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(sys.argv[1:] if argv is None else list(argv))
    adjust = B.adjust_window_host if a.host else B.adjust_window
    sched = dict(noiter=a.noiter, minres=a.minres)
    extra = {}
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
            fit = (F.fit_cameras_host if a.host else F.fit_cameras)(X, left, cam, mask=split["words"])
            xy, mask, init, offset = np.stack([left, right]), split["words"], fit["G"], [baseline, 0.0, 0.0]
            extra = dict(fit_G=fit["G"], inliers=rows[split["inliers"]], rows=rows)
        else:
            X, xy = z["X"], z["xy"]
            offset = z["offset"] if "offset" in z else None
            mask = z["mask"] if "mask" in z else None
            init = z["init"] if "init" in z else None
    res = adjust(X, xy, cam, offset=offset, mask=mask, init=init, **sched)
    np.savez(a.output, **{k: res[k] for k in KEYS}, **extra)
    print("\n".join(result_lines(res)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
