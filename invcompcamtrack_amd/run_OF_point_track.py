"""Point-track driver: the loop of misc_src/run_OF_point_track.py.ipynb cell 2 on the device.

  python -m invcompcamtrack_amd.run_OF_point_track listfile out.npz [--bsize 10] [--psz 15] [--lv_f 3] [--step 4]
         [--maxcorners 1000] [--th_ratio 0.2] [--th_abs 1.0]

listfile = one PGM path per line (the frames, in order); out.npz = what ``oftrack.savetofile`` writes (``x``: the ragged
list of track blocks).
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from . import io_formats as iof
from .patchflow import run_OF_point_track_hip


def main(argv=None):
    ap = argparse.ArgumentParser(prog="invcompcamtrack_amd.run_OF_point_track", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listfile")
    ap.add_argument("out")
    ap.add_argument("--bsize", type=int, default=10)
    ap.add_argument("--psz", type=int, default=15)
    ap.add_argument("--lv_f", type=int, default=3)
    ap.add_argument("--step", type=int, default=4)
    ap.add_argument("--maxcorners", type=int, default=1000)
    ap.add_argument("--th_ratio", type=float, default=0.2)
    ap.add_argument("--th_abs", type=float, default=1.0)
    a = ap.parse_args(argv)
    frames = [np.asarray(iof.read_image_gray(fn), np.float32) for fn in iof.read_image_list(a.listfile)]
    if len(frames) < 2:
        print("the list needs at least two frames", file=sys.stderr)
        return 2
    run_OF_point_track_hip(frames, a.bsize, a.psz, a.lv_f, a.step, a.maxcorners, a.th_ratio, a.th_abs, savefile=a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
