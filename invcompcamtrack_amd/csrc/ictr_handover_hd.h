// ictr_handover_hd.h -- the arithmetic of the window hand-over (DESIGN.md §4 "Window hand-over"), stated once: where a
// frame stands among the static split's view pairs (fsplit.pairs_from_stereo_tracks) and the point of the first view
// (camfit.depth_from_disparity, camfit.points_from_first_view; misc_src/run_test_OF_track.py:361-371). Compiled from the
// same text for the device (k_ho_pairs, k_ho_points of ictr_handover.hip) and, as plain C++, for the host
// (tests/cxx/handover_hd_host.cpp, built with sanitizers by tests/test_windowcams_cpu.py). Only - / * occur, in f64, one
// rounding each, in the order written (the library builds with -ffp-contract=off); a zero disparity gives an infinite or
// NaN point as it does in NumPy, which the fit leaves out.
#pragma once

#include "se3_math.h"

namespace ictr {

ICTR_HD int ho_npairs(int bsize) { return bsize / 2; }     // frame pairs of a window; the split sees two view pairs each
ICTR_HD int ho_offset(int bsize) { return (bsize + 1) / 2; }  // frame fr is paired with frame fr + ho_offset

struct HoCam {
  double fx, fy, cx, cy;
};

// xl, yl, xr: left x, y and right x of frame 0; bf = baseline * fx, formed by the caller in f64. X[3]
ICTR_HD void ho_point(double xl, double yl, double xr, double bf, const HoCam &cam, double *X) {
  const double d = bf / (xr - xl);
  X[0] = (xl - cam.cx) / cam.fx * d;
  X[1] = (yl - cam.cy) / cam.fy * d;
  X[2] = d;
}

}  // namespace ictr
