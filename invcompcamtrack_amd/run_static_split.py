"""Static / moving split of a track window (run_test_OF_track.py:309-343):

  python -m invcompcamtrack_amd.run_static_split in.npz out.npz [--ntrials 100] [--thresh 2.0] [--seed 0] [--stereo]
                                                 [--host]

in.npz holds one of: ``pairs`` (P, 4, N), the view pairs themselves; ``tracks`` (M, 2, bsize), one block of
PointTracker.tracks(); with --stereo ``xy_t`` (N, 4, bsize), the script's left / right layout (also read from
``tracks``). out.npz: ``inliers`` (indices into the input rows), ``dd`` (per kept row), ``F`` (P, 3, 3), ``best_trial``,
``best_count``, ``draws`` (8, into the kept rows), ``rows`` (the input rows without NaN that took part). The rounds run on
the GPU (fsplit.split_static); --host runs the host restatement instead (same bits).
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from .fsplit import pairs_from_stereo_tracks, pairs_from_tracks, split_static, split_static_host


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m invcompcamtrack_amd.run_static_split",
                                 description=__doc__.split("\n")[0])
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--ntrials", type=int, default=100)
    ap.add_argument("--thresh", type=float, default=2.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--stereo", action="store_true")
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args(sys.argv[1:] if argv is None else list(argv))
    with np.load(a.input) as z:
        if a.stereo:
            pairs, rows = pairs_from_stereo_tracks(z["xy_t"] if "xy_t" in z else z["tracks"])
        elif "pairs" in z:
            pairs = np.asarray(z["pairs"], np.float64)
            rows = np.arange(pairs.shape[2])
        else:
            pairs, rows = pairs_from_tracks(z["tracks"])
    res = (split_static_host if a.host else split_static)(pairs, a.ntrials, a.thresh, a.seed)
    np.savez(a.output, inliers=rows[res["inliers"]], dd=res["dd"], F=res["F"], best_trial=res["best_trial"],
             best_count=res["best_count"], draws=res["draws"], rows=rows)
    print(f"[run_static_split] {res['best_count']} of {pairs.shape[2]} points static (trial {res['best_trial']} of "
          f"{a.ntrials}, {pairs.shape[0]} view pairs)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
