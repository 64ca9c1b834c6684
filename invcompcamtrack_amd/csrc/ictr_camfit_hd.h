// ictr_camfit_hd.h -- the bit-pinned steps of the per-frame camera fit (ictr_camfit.hip), each stated once: the terms one
// observation adds to the normal equations, the order in which they are summed, the damped 6x6 solve, the pose update and
// the Levenberg-Marquardt bookkeeping of one frame. Compiled from the same text for the device (k_camfit_pass,
// k_camfit_step, k_camfit_reproj) and, as plain C++, for the host (tests/cxx/camfit_hd_host.cpp, built with sanitizers by
// tests/test_camfit_cpu.py); invcompcamtrack_amd/camfit.py restates them operation by operation. Only + - * / sqrt occur,
// in f64, in the order written (the library builds with -ffp-contract=off). Every array below is indexed by constants of
// fully unrolled loops.
//
// Reduction order, a function of N alone: the points go in chunks of C = kCfChunk = 1024. Inside a chunk lane l of 256
// adds its kCfPerLane = 4 points base + l, base + 256 + l, base + 512 + l, base + 768 + l to +0.0 in that order; the 256
// lane values are then added by the pairwise tree v[i] <- v[i] + v[i + s], i a multiple of 2 s, s = 1, 2, 4 .. 128. The
// chunk values are added to +0.0 serially in chunk order, and a NaN result is replaced by cf_nan(). Points past N and
// observations that do not count add exact zeros.
#pragma once

#include <math.h>

#include "se3_math.h"

namespace ictr {

constexpr int kCfBlock = 256;                      // lanes of a pass workgroup
constexpr int kCfPerLane = 4;                      // points per lane, serial
constexpr int kCfChunk = kCfBlock * kCfPerLane;    // C
constexpr int kCfTerms = 28;                       // H (21, upper triangle, row-major), b (6), s
constexpr int kCfSlots = 32;                       // doubles per chunk partial: the terms, [28] the count, 3 unused
constexpr int kCfCountSlot = 28;

// status of a frame (ICTR_CAMFIT_* of include/ictr.h); kCfRunning is never read back from a finished run
constexpr int kCfRunning = -1, kCfConverged = 0, kCfNoiter = 1, kCfMaxdamp = 2, kCfFewObs = 3, kCfStartNotFinite = 4;

struct CfCam {
  double fx, fy, cx, cy;
};
struct CfParams {
  int noiter;
  double damp_init, damp_fct, minres, maxdamp;
};
struct CfState {
  double G[12];   // the accepted pose, row-major [R | t]
  double Gt[12];  // the pose the next pass is taken at
  double c, damp;
  double H[21], b[6];      // the system at G
  double sums[kCfSlots];   // inspection: the ordered sums of the last pass
  long long n;
  int it, status, phase, pad_;
};

ICTR_HD double cf_nan() { return __builtin_nan(""); }  // the one NaN that outputs carry (0x7ff8000000000000)
ICTR_HD bool cf_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }
ICTR_HD double cf_canon(double v) { return v != v ? cf_nan() : v; }
ICTR_HD constexpr int cf_hidx(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }  // i <= j

// an observation counts iff its mask bit is set and its five coordinates are finite
ICTR_HD bool cf_counted(bool bit, double X, double Y, double Z, double xo, double yo) {
  return bit && cf_finite(X) && cf_finite(Y) && cf_finite(Z) && cf_finite(xo) && cf_finite(yo);
}

// the camera-frame point over its depth and the two residuals; tz: G[11], or G[11] + dt[2] for the reprojection
ICTR_HD void cf_project(const double *G, double tx, double ty, double tz, const CfCam &k, double X, double Y, double Z,
                        double xo, double yo, double &iz, double &xz, double &yz, double &rx, double &ry) {
  const double Xc = ((G[0] * X + G[1] * Y) + G[2] * Z) + tx;
  const double Yc = ((G[4] * X + G[5] * Y) + G[6] * Z) + ty;
  const double Zc = ((G[8] * X + G[9] * Y) + G[10] * Z) + tz;
  iz = 1.0 / Zc;
  xz = Xc * iz;
  yz = Yc * iz;
  rx = xo - (k.fx * xz + k.cx);
  ry = yo - (k.fy * yz + k.cy);
}

// the 28 terms of one observation at pose G (odometer.cpp:313-326 for the Jacobian of a left perturbation (dt, dw))
ICTR_HD void cf_point(const double *G, const CfCam &k, double X, double Y, double Z, double xo, double yo, bool counted,
                      double *t) {
  double iz, xz, yz, rx, ry;
  cf_project(G, G[3], G[7], G[11], k, X, Y, Z, xo, yo, iz, xz, yz, rx, ry);
  double jx[6], jy[6];
  jx[0] = k.fx * iz;
  jx[1] = 0.0;
  jx[2] = k.fx * (-(xz * iz));
  jx[3] = k.fx * (-(xz * yz));
  jx[4] = k.fx * (1.0 + xz * xz);
  jx[5] = k.fx * (-yz);
  jy[0] = 0.0;
  jy[1] = k.fy * iz;
  jy[2] = k.fy * (-(yz * iz));
  jy[3] = k.fy * (-(1.0 + yz * yz));
  jy[4] = k.fy * (xz * yz);
  jy[5] = k.fy * xz;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) t[cf_hidx(i, j)] = counted ? jx[i] * jx[j] + jy[i] * jy[j] : 0.0;
    t[21 + i] = counted ? jx[i] * rx + jy[i] * ry : 0.0;
  }
  t[27] = counted ? rx * rx + ry * ry : 0.0;
}

// the reprojection distance of one observation at pose G with the camera-frame offset dt on the translation
ICTR_HD double cf_reproj_point(const double *G, const double *dt, const CfCam &k, double X, double Y, double Z, double xo,
                               double yo, bool counted) {
  double iz, xz, yz, rx, ry;
  cf_project(G, G[3] + dt[0], G[7] + dt[1], G[11] + dt[2], k, X, Y, Z, xo, yo, iz, xz, yz, rx, ry);
  return counted ? sqrt(rx * rx + ry * ry) : 0.0;
}

// (H + damp diag(H)) x = b by LDL^T without pivoting; H: 21 entries (cf_hidx). False when a pivot is not finite or not > 0.
ICTR_HD bool cf_solve(const double *H, const double *b, double damp, double *x) {
  double L[6][6], D[6];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = H[cf_hidx(j, j)] + damp * H[cf_hidx(j, j)];
#pragma unroll
    for (int q = 0; q < j; ++q) d = d - L[j][q] * (L[j][q] * D[q]);
    if (!(d > 0.0) || !cf_finite(d)) ok = false;
    D[j] = d;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = H[cf_hidx(j, i)];
#pragma unroll
      for (int q = 0; q < j; ++q) s = s - L[i][q] * (L[j][q] * D[q]);
      L[i][j] = s / d;
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = b[i];
#pragma unroll
    for (int q = 0; q < i; ++q) s = s - L[i][q] * y[q];
    y[i] = s;
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = y[i] / D[i];
#pragma unroll
    for (int q = i + 1; q < 6; ++q) s = s - L[q][i] * x[q];
    x[i] = s;
  }
  return ok;
}

// Go = Cayley(dw) G with dt added: Rd = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a), a = dw / 2; R <- Rd R, t <- Rd t + dt.
// d = (dt, dw). Go must not alias G.
ICTR_HD void cf_update(const double *G, const double *d, double *Go) {
  const double a0 = d[3] * 0.5, a1 = d[4] * 0.5, a2 = d[5] * 0.5;
  const double aa = (a0 * a0 + a1 * a1) + a2 * a2;
  const double den = 1.0 + aa, kk = 1.0 - aa;
  double r[9];
  r[0] = (kk + 2.0 * (a0 * a0)) / den;
  r[1] = (2.0 * (a0 * a1) - 2.0 * a2) / den;
  r[2] = (2.0 * (a0 * a2) + 2.0 * a1) / den;
  r[3] = (2.0 * (a1 * a0) + 2.0 * a2) / den;
  r[4] = (kk + 2.0 * (a1 * a1)) / den;
  r[5] = (2.0 * (a1 * a2) - 2.0 * a0) / den;
  r[6] = (2.0 * (a2 * a0) - 2.0 * a1) / den;
  r[7] = (2.0 * (a2 * a1) + 2.0 * a0) / den;
  r[8] = (kk + 2.0 * (a2 * a2)) / den;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) Go[4 * i + j] = (r[3 * i] * G[j] + r[3 * i + 1] * G[4 + j]) + r[3 * i + 2] * G[8 + j];
    Go[4 * i + 3] = ((r[3 * i] * G[3] + r[3 * i + 1] * G[7]) + r[3 * i + 2] * G[11]) + d[i];
  }
}

// a frame before its first pass: both poses G0, damp_init, nothing counted yet
ICTR_HD void cf_init(CfState &s, const double *G0, const CfParams &p) {
#pragma unroll
  for (int q = 0; q < 12; ++q) s.G[q] = s.Gt[q] = G0[q];
  s.c = 0.0;
  s.damp = p.damp_init;
#pragma unroll
  for (int q = 0; q < 21; ++q) s.H[q] = 0.0;
#pragma unroll
  for (int q = 0; q < 6; ++q) s.b[q] = 0.0;
#pragma unroll
  for (int q = 0; q < kCfSlots; ++q) s.sums[q] = 0.0;
  s.n = 0;
  s.it = 0;
  s.status = kCfRunning;
  s.phase = 0;
  s.pad_ = 0;
}

// The bookkeeping between two passes. sums: the ordered sums of the pass at s.Gt. First (phase 0) the start: n, the cost,
// fewer than 3 observations or a cost that is not finite end the frame with G = G0. Later the accept test of the trial
// pose. Then the loop of the schedule up to the next trial pose: the stops are tested in the order cost <= minres
// (converged), it >= noiter, damp >= maxdamp; a failed solve raises the damping, counts an iteration and tries again
// without a pass, since the pose has not moved.
ICTR_HD void cf_step(CfState &s, const double *sums, const CfParams &p) {
  if (s.status != kCfRunning) return;
  const double n = sums[kCfCountSlot];
  const double c = cf_canon(sums[27] / n);
  bool take = false;
  if (s.phase == 0) {
    s.phase = 1;
    s.n = (long long)n;
    s.c = c;  // 0 / 0 without an observation: cf_nan()
    if (n < 3.0) {
      s.status = kCfFewObs;
      return;
    }
    if (!cf_finite(c)) {
      s.status = kCfStartNotFinite;
      return;
    }
    take = true;
  } else {
    s.it = s.it + 1;
    if (cf_finite(c) && c < s.c) {
      const double imp = s.c - c;
#pragma unroll
      for (int q = 0; q < 12; ++q) s.G[q] = s.Gt[q];
      s.c = c;
      s.damp = s.damp / p.damp_fct;
      take = true;
      if (imp <= p.minres) s.status = kCfConverged;
    } else {
      s.damp = s.damp * p.damp_fct;
    }
  }
  if (take) {
#pragma unroll
    for (int q = 0; q < 21; ++q) s.H[q] = sums[q];
#pragma unroll
    for (int q = 0; q < 6; ++q) s.b[q] = sums[21 + q];
  }
  if (s.status != kCfRunning) return;
  for (;;) {
    if (!(s.c > p.minres)) {
      s.status = kCfConverged;
      return;
    }
    if (!(s.it < p.noiter)) {
      s.status = kCfNoiter;
      return;
    }
    if (!(s.damp < p.maxdamp)) {
      s.status = kCfMaxdamp;
      return;
    }
    double d[6];
    if (cf_solve(s.H, s.b, s.damp, d)) {
      cf_update(s.G, d, s.Gt);
      return;
    }
    s.damp = s.damp * p.damp_fct;
    s.it = s.it + 1;
  }
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The pass in the stated order, serially (the device's k_camfit_pass / k_camfit_reproj and the ordered sum of
// k_camfit_step). X: [3][n], xy: [2][n] of one frame, words: inlier words or NULL. dt == NULL: the 28 terms of cf_point
// at G; otherwise slot 0 holds the sum of cf_reproj_point and the other terms are 0. out: kCfSlots doubles.
inline void cf_pass_host(const double *G, const double *dt, const CfCam &k, const double *X, const double *xy,
                         const unsigned long long *words, long long n, double *out) {
  double v[kCfTerms][kCfBlock];
  double tot[kCfTerms];
  for (int q = 0; q < kCfTerms; ++q) tot[q] = 0.0;
  long long cnt = 0;
  const long long nchunks = (n + kCfChunk - 1) / kCfChunk;
  for (long long ch = 0; ch < nchunks; ++ch) {
    for (int l = 0; l < kCfBlock; ++l) {
      double acc[kCfTerms];
      for (int q = 0; q < kCfTerms; ++q) acc[q] = 0.0;
      for (int r = 0; r < kCfPerLane; ++r) {
        const long long m = ch * kCfChunk + (long long)r * kCfBlock + l;
        if (m >= n) continue;  // exact zeros
        const bool bit = words ? ((words[m >> 6] >> (m & 63)) & 1ull) != 0 : true;
        const bool counted = cf_counted(bit, X[m], X[n + m], X[2 * n + m], xy[m], xy[n + m]);
        cnt += counted ? 1 : 0;
        double t[kCfTerms];
        if (dt) {
          for (int q = 0; q < kCfTerms; ++q) t[q] = 0.0;
          t[0] = cf_reproj_point(G, dt, k, X[m], X[n + m], X[2 * n + m], xy[m], xy[n + m], counted);
        } else {
          cf_point(G, k, X[m], X[n + m], X[2 * n + m], xy[m], xy[n + m], counted, t);
        }
        for (int q = 0; q < kCfTerms; ++q) acc[q] = acc[q] + t[q];
      }
      for (int q = 0; q < kCfTerms; ++q) v[q][l] = acc[q];
    }
    for (int s = 1; s < kCfBlock; s *= 2)
      for (int i = 0; i < kCfBlock; i += 2 * s)
        for (int q = 0; q < kCfTerms; ++q) v[q][i] = v[q][i] + v[q][i + s];
    for (int q = 0; q < kCfTerms; ++q) tot[q] = tot[q] + v[q][0];
  }
  for (int q = 0; q < kCfSlots; ++q) out[q] = 0.0;
  for (int q = 0; q < kCfTerms; ++q) out[q] = cf_canon(tot[q]);
  out[kCfCountSlot] = (double)cnt;
}

// one frame's whole fit on the host: passes and steps until the frame stops
inline void cf_fit_host(const double *G0, const CfCam &k, const CfParams &p, const double *X, const double *xy,
                        const unsigned long long *words, long long n, CfState &s) {
  cf_init(s, G0, p);
  while (s.status == kCfRunning) {
    cf_pass_host(s.Gt, nullptr, k, X, xy, words, n, s.sums);
    cf_step(s, s.sums, p);
  }
}
#endif

}  // namespace ictr
