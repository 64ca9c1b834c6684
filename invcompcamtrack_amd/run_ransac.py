"""RANSAC pose samples for a run_track_nposes input file (the first half of func_ransac_fitcameras_odom.m):

  python -m invcompcamtrack_amd.run_ransac in.txt out.txt [--track result.txt] [--nsamples 500] [--maxtrials M]
                                           [--inlthresh T] [--kc 0] [--seed 0]

Reads the parameters, camera, frames and 2-D/3-D matches of in.txt (its sample section is ignored and may be `0`),
draws the pose samples on the GPU (ransac.sample_poses) and writes out.txt: the same file with the samples filled in
(poses p = se3_log([R | -R t]), 1-based sorted inlier ids). Defaults as run_ransac_test.m:67,84-85: maxtrials = 100 x
nsamples, inlthresh = image diagonal / 100. With --track the samples are also verified (run_track_nposes.run): the
nposes result goes to result.txt and the best sample (largest mean correlation) is printed.
"""
from __future__ import annotations

import argparse
import math
import sys

import numpy as np

from . import io_formats as iof
from . import run_track_nposes
from .ransac import best_sample, sample_poses


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m invcompcamtrack_amd.run_ransac", description=__doc__.split("\n")[0])
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--track", default=None)
    ap.add_argument("--nsamples", type=int, default=500)
    ap.add_argument("--maxtrials", type=int, default=None)
    ap.add_argument("--inlthresh", type=float, default=None)
    ap.add_argument("--kc", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(sys.argv[1:] if argv is None else list(argv))
    inp = iof.read_nposes_input(a.input)
    maxtrials = 100 * a.nsamples if a.maxtrials is None else a.maxtrials
    wh = inp["wh"]
    thr = math.sqrt(float(wh[0]) ** 2 + float(wh[1]) ** 2) / 100.0 if a.inlthresh is None else a.inlthresh
    smp = sample_poses(inp["pt2d"], inp["pt3d"], inp["fc"], inp["cc"], a.nsamples, maxtrials, thr, a.kc, a.seed)
    inp["poses"] = smp["p"]
    inp["inlids"] = [np.sort(i) + 1 for i in smp["inl"]]
    iof.write_nposes_input(a.output, inp["op"], inp["fc"], inp["cc"], inp["wh"], inp["fbframes"], inp["filenames"],
                           inp["pt2d"], inp["pt3d"], inp["poses"], inp["inlids"])
    print(f"[run_ransac] {len(smp['p'])} samples ({smp['accepted']} accepted, {smp['trials_used']} trials)")
    if a.track is not None:
        out_corr, out_pose = run_track_nposes.run(inp) if len(inp["poses"]) else ([], [])
        iof.write_nposes_result(a.track, out_corr, out_pose)
        best, means = best_sample(out_corr)
        if best is None:
            print("[run_ransac] no sample to verify")
        else:
            print(f"[run_ransac] best sample {best}: mean correlation {means[best]:.6g}, "
                  f"{len(inp['inlids'][best])} inliers")
    return 0


if __name__ == "__main__":
    sys.exit(main())
