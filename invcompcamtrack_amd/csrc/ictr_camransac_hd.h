// ictr_camransac_hd.h -- the bit-pinned steps of the window camera RANSAC (ictr_camransac.hip), each stated once: which
// points count, the hypothesis of one frame of one trial and its pose, the squared reprojection residual of one
// observation, the running maximum and the inlier test. Compiled from the same text for the device (k_cr_flags, k_cr_hyp,
// k_cr_score, k_cr_mask) and, as plain C++, for the host (tests/cxx/camransac_hd_host.cpp, built with sanitizers by
// tests/test_camransac_cpu.py); invcompcamtrack_amd/camransac.py restates them operation by operation. Only + - * / sqrt
// occur, in f64, in the order written (the library builds with -ffp-contract=off).
//
// The rule: trial g draws ran_draw<4>(mix(seed), g, N) once for the whole window. It fails with fewer than 4 distinct
// indices or a drawn point that does not count. Frame f's hypothesis is p3p_hypothesis (ictr_p3p_hd.h) on the drawn
// points and their left pixels of frame f at kc = 0; its pose is G = [R | -R c]; twelve NaN without one, and the trial
// fails. Point i's distance is the maximum over the frames (outer) and sides (inner) of cf_reproj_point at t_f + o_s; a
// correctly rounded sqrt is monotone, so the maximum is kept on rx^2 + ry^2 and one root is taken. Point i is an inlier iff
// it counts and that distance is < thresh. The largest count wins, the lowest trial on ties.
#pragma once

#include <math.h>

#include "ictr_camfit_hd.h"
#include "ictr_draw_hd.h"
#include "ictr_p3p_hd.h"

namespace ictr {

constexpr int kCrHypBlock = 64;      // one lane per (trial, frame)
constexpr int kCrScoreBlock = 256;   // four waves, one 64-point block each
constexpr int kCrSelBlock = 1024;    // the one-workgroup select
constexpr int kCrTilePoses = 240;    // poses of a score workgroup's LDS tile (23040 B): 240 / T frames of T trials
constexpr int kCrMaxFrames = 64;

struct CrState {
  long long best_trial, best_count;  // -1, 0: no trial has succeeded
  int draws[4];
  int found, pad_;
};

ICTR_HD bool cr_bit(const unsigned long long *w, long long m) { return ((w[m >> 6] >> (m & 63)) & 1ull) != 0; }

// does point m count: its mask bit, its three coordinates and all its 2 S F observation coordinates; xy [S][F][2][n]
ICTR_HD bool cr_counts(bool bit, const double *X, const double *xy, long long n, int nframes, int nsides, long long m) {
  bool ok = bit && cf_finite(X[m]) && cf_finite(X[n + m]) && cf_finite(X[2 * n + m]);
  for (int q = 0; q < 2 * nsides * nframes; ++q) ok = ok && cf_finite(xy[(long long)q * n + m]);
  return ok;
}

// the draws of trial g and whether every drawn point counts (cw: the counts words)
ICTR_HD bool cr_draw(unsigned long long seedmix, long long g, int n, const unsigned long long *cw, int *idx) {
  bool ok = ran_draw<4>(seedmix, g, n, idx) == 4;
#pragma unroll
  for (int q = 0; q < 4; ++q) ok = ok && idx[q] >= 0 && cr_bit(cw, idx[q]);
  return ok;
}

// G = [R | t], t[r] = -R[r][0] c[0] - R[r][1] c[1] - R[r][2] c[2], left to right
ICTR_HD void cr_pose(const double *R, const double *c, double *G) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int k = 0; k < 3; ++k) G[4 * r + k] = R[3 * r + k];
    G[4 * r + 3] = -R[3 * r + 0] * c[0] - R[3 * r + 1] * c[1] - R[3 * r + 2] * c[2];
  }
}

// one frame's hypothesis from the drawn points; xyl: the frame's left observations [2][n]. Twelve NaN without one.
ICTR_HD bool cr_hyp(const int *idx, const double *X, const double *xyl, long long n, const CfCam &k, double *G) {
  double P[4][3], u[4], v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const long long i = idx[q];
    P[q][0] = X[i];
    P[q][1] = X[n + i];
    P[q][2] = X[2 * n + i];
    u[q] = xyl[i];
    v[q] = xyl[n + i];
  }
  double R[9], c[3];
  const bool ok = p3p_hypothesis(P, u, v, k.fx, k.fy, k.cx, k.cy, 0.0, R, c) != 0;
  if (ok) {
    cr_pose(R, c, G);
  } else {
#pragma unroll
    for (int q = 0; q < 12; ++q) G[q] = cf_nan();
  }
  return ok;
}

// rx^2 + ry^2 of one observation at pose G with the side offset o on the translation: what cf_reproj_point takes the
// root of
ICTR_HD double cr_sq(const double *G, const double *o, const CfCam &k, double X, double Y, double Z, double xo,
                     double yo) {
  double iz, xz, yz, rx, ry;
  cf_project(G, G[3] + o[0], G[7] + o[1], G[11] + o[2], k, X, Y, Z, xo, yo, iz, xz, yz, rx, ry);
  return rx * rx + ry * ry;
}

// the running maximum; a NaN stays (as cf_nan()). Start from -1.
ICTR_HD double cr_max(double mx, double d) { return d != d ? cf_nan() : (d > mx ? d : mx); }

// the distance of a point from its running maximum of squares
ICTR_HD double cr_dist(double mx) { return cf_canon(sqrt(mx)); }

#if !defined(__HIP_DEVICE_COMPILE__)
// One trial on the host, serially. X [3][n], xy [S][F][2][n], cw the counts words, off [3] the offset of side 1.
// idx [4], G [F][12]; dd [n] and words [ceil(n / 64)] may be NULL. Returns the status; *cnt the inlier count.
inline int cr_trial_host(unsigned long long seedmix, long long g, const double *X, const double *xy,
                         const unsigned long long *cw, long long n, int F, int S, const CfCam &k, const double *off,
                         double thr, int *idx, double *G, long long *cnt, double *dd, unsigned long long *words) {
  const bool drawn = cr_draw(seedmix, g, (int)n, cw, idx);  // failed: no hypothesis in any frame
  int status = drawn ? 1 : 0;
  for (int f = 0; f < F; ++f) {
    bool ok = false;
    if (drawn) {
      ok = cr_hyp(idx, X, xy + (long long)f * 2 * n, n, k, G + 12 * f);
    } else {
      for (int q = 0; q < 12; ++q) G[12 * f + q] = cf_nan();
    }
    if (!ok) status = 0;
  }
  const double o[2][3] = {{0.0, 0.0, 0.0}, {off ? off[0] : 0.0, off ? off[1] : 0.0, off ? off[2] : 0.0}};
  long long c = 0;
  for (long long w = 0; words && w < (n + 63) / 64; ++w) words[w] = 0ull;
  for (long long m = 0; m < n; ++m) {
    double mx = -1.0;
    for (int f = 0; f < F; ++f)
      for (int s = 0; s < S; ++s) {
        const double *b = xy + ((long long)s * F + f) * 2 * n;
        mx = cr_max(mx, cr_sq(G + 12 * f, o[s], k, X[m], X[n + m], X[2 * n + m], b[m], b[n + m]));
      }
    const double d = cr_dist(mx);
    const bool inl = cr_bit(cw, m) && d < thr;
    if (dd) dd[m] = d;
    if (inl) {
      ++c;
      if (words) words[m >> 6] |= 1ull << (m & 63);
    }
  }
  *cnt = c;
  return status;
}
#endif

}  // namespace ictr
