// ictr_stereotrack_hd.h -- the per-point step of the stereo track window (misc_src/run_test_OF_track.py:170-223), stated
// once: the gather over a field accessor (func_get_transf_position), the frame-0 open, the per-frame advance with its eight
// tests. Compiled from the same text for the device (k_st_open, k_st_advance of ictr_stereotrack.hip) and, as plain C++, for
// the host (tests/cxx/stereotrack_hd_host.cpp, built with sanitizers by tests/test_stereotrack_cpu.py);
// invcompcamtrack_amd/stereotrack.py restates it operation by operation. Only + - * / sqrt floor occur, in f64, in the
// order written (the library builds with -ffp-contract=off); NaN and x / 0 compare false, so a point with zero motion or
// zero disparity is dropped, as in the script.
//
// A field accessor F gives width(), height(), xonly() and taps(x0, y0, u, v): the field's two components at the pixels
// (x0+1, y0+1), (x0, y0+1), (x0+1, y0), (x0, y0) -- the script's tap order w0..w3 -- widened to f64 and multiplied by the
// field's exact sign. v is not read when xonly().
#pragma once

#include <math.h>
#include <stddef.h>

#include "se3_math.h"

namespace ictr {

ICTR_HD double st_nan() { return __builtin_nan(""); }  // the one NaN that outputs carry (0x7ff8000000000000)

// a field in plain memory (host or device): comps = 1 a plane [h][w], used x only; comps = 2 an interleaved flow [h][w][2]
struct StMem {
  const float *p;
  int w, h, comps, x_only;
  double sign;  // +1 or -1
  ICTR_HD int width() const { return w; }
  ICTR_HD int height() const { return h; }
  ICTR_HD bool xonly() const { return comps == 1 || x_only != 0; }
  ICTR_HD void taps(int x0, int y0, double *u, double *v) const {
    const size_t c = (size_t)comps, r0 = (size_t)y0 * (size_t)w + (size_t)x0, r1 = r0 + (size_t)w;
    u[0] = sign * (double)p[(r1 + 1) * c];
    u[1] = sign * (double)p[r1 * c];
    u[2] = sign * (double)p[(r0 + 1) * c];
    u[3] = sign * (double)p[r0 * c];
    if (!xonly()) {
      v[0] = sign * (double)p[(r1 + 1) * c + 1];
      v[1] = sign * (double)p[r1 * c + 1];
      v[2] = sign * (double)p[(r0 + 1) * c + 1];
      v[3] = sign * (double)p[r0 * c + 1];
    }
  }
};

// func_get_transf_position for one point: NaN and out-of-range coordinates fail the four-tap range test (written
// positively, like the INT_MIN cast in NumPy) and give (NaN, NaN); an x-only field leaves y as it is
template <class F>
ICTR_HD void st_gather(const F &f, double x, double y, double *ox, double *oy) {
  const double flx = floor(x), fly = floor(y);
  *ox = st_nan();
  *oy = st_nan();
  if (flx >= 0.0 && fly >= 0.0 && flx + 1.0 < (double)f.width() && fly + 1.0 < (double)f.height()) {
    const int x0 = (int)flx, y0 = (int)fly;
    const double fx = x - flx, fy = y - fly;
    const double w0 = fx * fy, w1 = (1 - fx) * fy, w2 = fx * (1 - fy), w3 = (1 - fx) * (1 - fy);
    double u[4], v[4] = {0.0, 0.0, 0.0, 0.0};
    f.taps(x0, y0, u, v);
    *ox = x + (u[0] * w0 + u[1] * w1 + u[2] * w2 + u[3] * w3);
    *oy = f.xonly() ? y : y + (v[0] * w0 + v[1] * w1 + v[2] * w2 + v[3] * w3);
  }
}

ICTR_HD double st_norm(double dx, double dy) { return sqrt(dx * dx + dy * dy); }  // np.linalg.norm of a pair

// frame 0 (:180-187): p[4] = left x, y, right x, y of the start point (xl, yl); false: the point is dropped
template <class F>
ICTR_HD bool st_open(const F &lr, const F &rl, double xl, double yl, double th_ratio, double th_abs, double *p) {
  double xr, yr, xb, yb;
  st_gather(lr, xl, yl, &xr, &yr);
  st_gather(rl, xr, yr, &xb, &yb);
  const double err = st_norm(xl - xb, yl - yb), base = st_norm(xr - xl, yr - yl);
  p[0] = xl;
  p[1] = yl;
  p[2] = xr;
  p[3] = yr;
  return (err / base < th_ratio) & (err < th_abs);
}

// frame fr >= 1 (:190-215): p[4] of frame fr - 1 -> q[4] of frame fr through the flows of the pair (l_fwd, l_bwd, r_fwd,
// r_bwd) and the disparities of frame fr (lr, rl); false: one of the eight tests failed
template <class F>
ICTR_HD bool st_advance(const F &l_fwd, const F &l_bwd, const F &r_fwd, const F &r_bwd, const F &lr, const F &rl,
                        const double *p, double th_ratio, double th_abs, double *q) {
  const double xl = p[0], yl = p[1], xr = p[2], yr = p[3];
  double xlf, ylf, xrf, yrf, xrd, yrd, xld, yld, xlv, ylv, xrv, yrv;
  st_gather(l_fwd, xl, yl, &xlf, &ylf);
  st_gather(r_fwd, xr, yr, &xrf, &yrf);
  st_gather(lr, xlf, ylf, &xrd, &yrd);    // xy_rf_verif_d
  st_gather(rl, xrf, yrf, &xld, &yld);    // xy_lf_verif_d
  st_gather(l_bwd, xlf, ylf, &xlv, &ylv);  // xy_l_verif_f
  st_gather(r_bwd, xrf, yrf, &xrv, &yrv);  // xy_r_verif_f
  const double e1 = st_norm(xrf - xrd, yrf - yrd), e2 = st_norm(xlf - xld, ylf - yld);
  const double e3 = st_norm(xl - xlv, yl - ylv), e4 = st_norm(xr - xrv, yr - yrv);
  const double d12 = st_norm(xrf - xlf, yrf - ylf), d3 = st_norm(xl - xlf, yl - ylf), d4 = st_norm(xr - xrf, yr - yrf);
  q[0] = xlf;
  q[1] = ylf;
  q[2] = xrf;
  q[3] = yrf;
  return (e1 / d12 < th_ratio) & (e2 / d12 < th_ratio) & (e3 / d3 < th_ratio) & (e4 / d4 < th_ratio) & (e1 < th_abs) &
         (e2 < th_abs) & (e3 < th_abs) & (e4 < th_abs);
}

// the whole window of one start point on the host (the test program's loop): row[4][bsize]; false: dropped
template <class F>
inline bool st_track_host(const F *lr, const F *rl, const F *l_fwd, const F *l_bwd, const F *r_fwd, const F *r_bwd,
                          int bsize, double x, double y, double th_ratio, double th_abs, double *row) {
  double p[4], q[4];
  if (!st_open(lr[0], rl[0], x, y, th_ratio, th_abs, p)) return false;
  for (int c = 0; c < 4; ++c) row[c * bsize] = p[c];
  for (int fr = 1; fr < bsize; ++fr) {
    if (!st_advance(l_fwd[fr - 1], l_bwd[fr - 1], r_fwd[fr - 1], r_bwd[fr - 1], lr[fr], rl[fr], p, th_ratio, th_abs, q))
      return false;
    for (int c = 0; c < 4; ++c) row[c * bsize + fr] = p[c] = q[c];
  }
  return true;
}

}  // namespace ictr
