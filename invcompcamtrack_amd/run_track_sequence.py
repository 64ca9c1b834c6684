"""Sequence driver: the loop of run_odometer_test.m:172-250 (frame t -> t+1 from the pose tracked for frame t, every
10th visible point by default) with the step between pairs on the device:

  python -m invcompcamtrack_amd.run_track_sequence listfile infile outfile lv_f lv_l psz maxiter normdp_ratio \\
         donorm dopatchnorm maxpttrack stride

listfile = one PGM path per line (the frames, in order); infile = the binary point/cam file of
run_io_reprojection_test (p_init = pose of frame 0, then the world points; no 10 000-point cap here);
outfile = N x 6 f64, the tracked pose of every frame (the script's pose_tr{3,:}). maxpttrack caps the points of one pair
(and picks the launch form), stride is the subsampling of the visible points.
"""
from __future__ import annotations

import sys

import numpy as np

from . import io_formats as iof
from .sequence import SequenceTracker
from .tracker import CamClass, optparam


def main(argv=None):
    a = sys.argv[1:] if argv is None else list(argv)
    if len(a) != 12:
        print(__doc__)
        return 2
    listfile, infile, outfile = a[0:3]
    lv_f, lv_l, psz, maxiter = int(a[3]), int(a[4]), int(a[5]), int(a[6])
    ratio, donorm, dpn, maxpt, stride = float(a[7]), int(a[8]), int(a[9]), int(a[10]), int(a[11])
    op = optparam(lv_f, lv_l, psz, maxiter, ratio, donorm, dpn, maxpt)
    frames = np.stack([iof.read_image_gray(fn) for fn in iof.read_image_list(listfile)]).astype(np.float32)
    d = iof.read_pointcam_file_uncapped(infile)
    cam = CamClass(lv_f + 1, d["fc"], d["cc"], d["wh"], psz)
    st = SequenceTracker(cam, op, d["pts3d"], stride)
    st.track_async(frames, d["pose"])
    np.asarray(st.wait()["poses"], "<f8").tofile(outfile)
    return 0


if __name__ == "__main__":
    sys.exit(main())
