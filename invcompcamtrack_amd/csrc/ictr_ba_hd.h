// ictr_ba_hd.h -- the bit-pinned steps of the window bundle adjustment (ictr_ba.hip), each stated once: what one
// observation adds to a point's and a frame's normal equations, the damped 3x3 point solve, the terms of the reduced
// (Schur) system of the cameras, its LDL^T, the back-substitution and the Levenberg-Marquardt bookkeeping. Compiled from
// the same text for the device and, as plain C++, for the host (tests/cxx/bundle_hd_host.cpp, built with sanitizers by
// tests/test_bundle_cpu.py); invcompcamtrack_amd/bundle.py restates it operation by operation and is the statement of
// record. Only + - * / occur, in f64, in the order written (the library builds with -ffp-contract=off).
//
// Unknowns: the poses of frames 1 .. F - 1 (frame 0 keeps its start pose) and every adjusted point. Side s of frame f
// sees x_cam = R_f X + (t_f + o_s), o_0 = 0, o_1 = the offset. A point is adjusted iff its mask bit is set and its three
// coordinates and all its 2 S F observation coordinates are finite; any other point adds exact zeros and is not moved.
//
// Every sum over points is taken in ictr_camfit_hd.h's order, a function of N alone. Every sum over observations of one
// point goes over the frames f = 0 .. F - 1 outer and the sides s = 0 .. S - 1 inner, added to +0.0 in that order.
#pragma once

#include <vector>

#include "ictr_camfit_hd.h"

namespace ictr {

constexpr int kBaMaxFrames = 32;
constexpr int kBaMaxDim = 6 * (kBaMaxFrames - 1);  // unknowns of the largest reduced system
constexpr int kBaLdsDim = 78;                      // reduced systems up to F = 14 are factored in LDS
constexpr int kBaPairTerms = 42;                   // of a block pair (f, g): T_fg (36, [a][b]) and Y_f gp (6)
constexpr int kBaPairSlots = 48;                   // doubles per partial: the terms, [42] the failed point solves
constexpr int kBaFailSlot = 42;
constexpr int kBaStart = 0, kBaTrial = 1, kBaRetry = 2;  // BaState::phase: what the next pass finds at the trial set

struct BaState {
  double G[kBaMaxFrames * 12];   // the accepted poses
  double Gt[kBaMaxFrames * 12];  // the trial poses
  double U[kBaMaxFrames * 21], gc[kBaMaxFrames * 6];  // the frames' blocks at the accepted poses and points
  double dc[kBaMaxDim];          // the camera part of the last solved step
  double c, damp;
  long long n;
  int it, status, phase;
  int cur, tset;  // which of the two point sets holds the accepted points, and which the trial points
  int pad_;
};

ICTR_HD constexpr int ba_vidx(int i, int j) { return i * 3 - i * (i - 1) / 2 + (j - i); }  // i <= j < 3
// the place of entry (I, J), I <= J, in the packed upper triangle (row-major) of the reduced system of size n
ICTR_HD int ba_ridx(int n, int I, int J) { return I * n - I * (I - 1) / 2 + (J - I); }
ICTR_HD constexpr int ba_npairs(int nframes) { return (nframes - 1) * nframes / 2; }  // block pairs 1 <= f <= g < F
// pair p = 0, 1, .. counts (1, 1), (1, 2) .. (1, F - 1), (2, 2), ..
ICTR_HD void ba_pair(int nframes, int p, int &f, int &g) {
  f = 1;
  int row = nframes - 1;
  while (p >= row) {
    p -= row;
    row -= 1;
    f += 1;
  }
  g = f + p;
}

// One observation: the residual, the camera Jacobian rows and the point Jacobian rows. With o = 0 the camera rows are
// cf_point's jx, jy bit for bit; with an offset their rotation columns take the turning part x_cam - o, which is what
// cf_update moves (cf_point's formula on x_cam itself is the Jacobian of another update and stalls above the minimum).
struct BaObs {
  double rx, ry, jx[6], jy[6], px[3], py[3];
};
ICTR_HD void ba_obs(const double *G, const double *o, const CfCam &k, double X, double Y, double Z, double xo, double yo,
                    BaObs &b) {
  double iz, xz, yz;
  cf_project(G, G[3] + o[0], G[7] + o[1], G[11] + o[2], k, X, Y, Z, xo, yo, iz, xz, yz, b.rx, b.ry);
  // cf_update turns R X + t and leaves o where it is: the part of x_cam that turns, over the depth
  const double qx = xz - o[0] * iz, qy = yz - o[1] * iz, qz = 1.0 - o[2] * iz;
  b.jx[0] = k.fx * iz;
  b.jx[1] = 0.0;
  b.jx[2] = k.fx * (-(xz * iz));
  b.jx[3] = k.fx * (-(xz * qy));
  b.jx[4] = k.fx * (qz + xz * qx);
  b.jx[5] = k.fx * (-qy);
  b.jy[0] = 0.0;
  b.jy[1] = k.fy * iz;
  b.jy[2] = k.fy * (-(yz * iz));
  b.jy[3] = k.fy * (-(qz + yz * qy));
  b.jy[4] = k.fy * (yz * qx);
  b.jy[5] = k.fy * qx;
  const double ax = k.fx * iz, ay = k.fy * iz;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    b.px[q] = ax * (G[q] - xz * G[8 + q]);
    b.py[q] = ay * (G[4 + q] - yz * G[8 + q]);
  }
}

// V (6, ba_vidx) and gp (3) of a point take one observation
ICTR_HD void ba_add_point(const BaObs &b, double *V, double *gp) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = i; j < 3; ++j) V[ba_vidx(i, j)] = V[ba_vidx(i, j)] + (b.px[i] * b.px[j] + b.py[i] * b.py[j]);
    gp[i] = gp[i] + (b.px[i] * b.rx + b.py[i] * b.ry);
  }
}
// W (6 x 3, [a][k]) of a point in one frame takes one side
ICTR_HD void ba_add_w(const BaObs &b, double *W) {
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int q = 0; q < 3; ++q) W[3 * a + q] = W[3 * a + q] + (b.jx[a] * b.px[q] + b.jy[a] * b.py[q]);
}
// the 28 terms of a point in one frame (U: 21, cf_hidx; gc: 6; the squared residual) take one side
ICTR_HD void ba_add_cam(const BaObs &b, double *t) {
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) t[cf_hidx(i, j)] = t[cf_hidx(i, j)] + (b.jx[i] * b.jx[j] + b.jy[i] * b.jy[j]);
    t[21 + i] = t[21 + i] + (b.jx[i] * b.rx + b.jy[i] * b.ry);
  }
  t[27] = t[27] + (b.rx * b.rx + b.ry * b.ry);
}

// V + damp diag(V) = L D L^T without pivoting, cf_solve's shape for 3; L: [1][0], [2][0], [2][1]. False when a pivot is
// not finite or not > 0.
ICTR_HD bool ba_factor3(const double *V, double damp, double *L, double *D) {
  bool ok = true;
  double l[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    double d = V[ba_vidx(j, j)] + damp * V[ba_vidx(j, j)];
#pragma unroll
    for (int q = 0; q < j; ++q) d = d - l[j][q] * (l[j][q] * D[q]);
    if (!(d > 0.0) || !cf_finite(d)) ok = false;
    D[j] = d;
#pragma unroll
    for (int i = j + 1; i < 3; ++i) {
      double s = V[ba_vidx(j, i)];
#pragma unroll
      for (int q = 0; q < j; ++q) s = s - l[i][q] * (l[j][q] * D[q]);
      l[i][j] = s / d;
    }
  }
  L[0] = l[1][0];
  L[1] = l[2][0];
  L[2] = l[2][1];
  return ok;
}
// x = (L D L^T)^-1 b through the factors of ba_factor3
ICTR_HD void ba_solve3(const double *L, const double *D, const double *b, double *x) {
  const double y0 = b[0];
  const double y1 = b[1] - L[0] * y0;
  const double y2 = (b[2] - L[1] * y0) - L[2] * y1;
  x[2] = y2 / D[2];
  x[1] = y1 / D[1] - L[2] * x[2];
  x[0] = (y0 / D[0] - L[0] * x[1]) - L[1] * x[2];
}

// the 42 terms one point adds to block pair (f, g): Y_f = W_f V*^-1 row by row, T[a][b] = sum_k Y_f[a][k] W_g[b][k] and
// Y_f gp, with k in order
ICTR_HD void ba_pair_terms(const double *Wf, const double *Wg, const double *L, const double *D, const double *gp,
                           double *t) {
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    double y[3];
    ba_solve3(L, D, Wf + 3 * a, y);
#pragma unroll
    for (int b = 0; b < 6; ++b) t[6 * a + b] = (y[0] * Wg[3 * b] + y[1] * Wg[3 * b + 1]) + y[2] * Wg[3 * b + 2];
    t[36 + a] = (y[0] * gp[0] + y[1] * gp[1]) + y[2] * gp[2];
  }
}

// Entry (I, J), I <= J, of the reduced system: delta_fg U*_f - T_fg. U: the frames' blocks [F][21]; T: the ordered sums
// of the pairs [npairs][kBaPairSlots]. Only this upper triangle in global indices is ever formed or read: of a diagonal
// block T_ff the entries a <= b.
ICTR_HD double ba_reduced_entry(const double *U, const double *T, int nframes, double damp, int I, int J) {
  const int f = I / 6 + 1, a = I % 6, g = J / 6 + 1, b = J % 6;
  const int p = (f - 1) * (nframes - 1) - (f - 1) * (f - 2) / 2 + (g - f);
  double u = 0.0;
  if (f == g) {
    u = U[21 * f + cf_hidx(a, b)];
    if (a == b) u = u + damp * u;
  }
  return cf_canon(u - T[(size_t)p * kBaPairSlots + 6 * a + b]);
}
// entry I of the right-hand side: gc_f - sum over points of Y_f gp
ICTR_HD double ba_reduced_rhs(const double *gc, const double *T, int nframes, int I) {
  const int f = I / 6 + 1, a = I % 6;
  const int p = (f - 1) * (nframes - 1) - (f - 1) * (f - 2) / 2;
  return cf_canon(gc[6 * f + a] - T[(size_t)p * kBaPairSlots + 36 + a]);
}

// LDL^T of the packed upper triangle A in place, columns left to right: after column j, A(j, j) = D[j] and A(j, i) =
// L[i][j]. ba_ldl_sum is the entry of column j, row i >= j, before its division: every inner sum subtracted in index
// order q = 0 .. j - 1, cf_solve written for n. The entries of one column do not depend on each other.
ICTR_HD double ba_ldl_sum(const double *A, int n, int j, int i) {
  double s = A[ba_ridx(n, j, i)];
  for (int q = 0; q < j; ++q) s = s - A[ba_ridx(n, q, i)] * (A[ba_ridx(n, q, j)] * A[ba_ridx(n, q, q)]);
  return s;
}
ICTR_HD bool ba_pivot_ok(double d) { return d > 0.0 && cf_finite(d); }
// x = (L D L^T)^-1 b through the factored A
ICTR_HD void ba_ldl_solve(const double *A, int n, const double *b, double *x) {
  for (int i = 0; i < n; ++i) {
    double s = b[i];
    for (int q = 0; q < i; ++q) s = s - A[ba_ridx(n, q, i)] * x[q];
    x[i] = s;
  }
  for (int i = n - 1; i >= 0; --i) {
    double s = x[i] / A[ba_ridx(n, i, i)];
    for (int q = i + 1; q < n; ++q) s = s - A[ba_ridx(n, i, q)] * x[q];
    x[i] = s;
  }
}

// dX = V*^-1 (gp - sum_{f = 1 .. F - 1} W_f^T dc_f), f in order; W: the point's [F][18] (frame 0 unused)
ICTR_HD void ba_back_rhs(const double *W, const double *dc, double *b) {
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    double t = W[q] * dc[0];
#pragma unroll
    for (int a = 1; a < 6; ++a) t = t + W[3 * a + q] * dc[a];
    b[q] = b[q] - t;
  }
}

// a run before its first pass
ICTR_HD void ba_init(BaState &s, const double *G0, int nframes, const CfParams &p) {
  for (int q = 0; q < kBaMaxFrames * 12; ++q) s.G[q] = s.Gt[q] = q < 12 * nframes ? G0[q] : 0.0;
  for (int q = 0; q < kBaMaxFrames * 21; ++q) s.U[q] = 0.0;
  for (int q = 0; q < kBaMaxFrames * 6; ++q) s.gc[q] = 0.0;
  for (int q = 0; q < kBaMaxDim; ++q) s.dc[q] = 0.0;
  s.c = 0.0;
  s.damp = p.damp_init;
  s.n = 0;
  s.it = 0;
  s.status = kCfRunning;
  s.phase = kBaStart;
  s.cur = s.tset = 0;
  s.pad_ = 0;
}

// the stops, tested in cf_step's order
ICTR_HD void ba_stops(BaState &s, const CfParams &p) {
  if (!(s.c > p.minres))
    s.status = kCfConverged;
  else if (!(s.it < p.noiter))
    s.status = kCfNoiter;
  else if (!(s.damp < p.maxdamp))
    s.status = kCfMaxdamp;
}

// the cost from the frames' ordered sums [F][kCfSlots]: the squared residuals added to +0.0 in frame order over n S F
ICTR_HD double ba_cost(const double *sums, int nframes, int nsides) {
  double tot = 0.0;
  for (int f = 0; f < nframes; ++f) tot = tot + sums[kCfSlots * f + 27];
  return cf_canon(cf_canon(tot) / (sums[kCfCountSlot] * (double)(nsides * nframes)));
}

// The bookkeeping behind a pass at the trial set, cf_step's first half. sums: the frames' ordered sums [F][kCfSlots] of
// that pass; n is frame 0's count.
ICTR_HD void ba_decide(BaState &s, const double *sums, int nframes, int nsides, const CfParams &p) {
  if (s.status != kCfRunning || s.phase == kBaRetry) return;
  const double n = sums[kCfCountSlot];
  const double c = ba_cost(sums, nframes, nsides);
  bool take = false;
  if (s.phase == kBaStart) {
    s.n = (long long)n;
    s.c = c;
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
      for (int q = 0; q < 12 * nframes; ++q) s.G[q] = s.Gt[q];
      s.cur = s.tset;
      s.c = c;
      s.damp = s.damp / p.damp_fct;
      take = true;
      if (imp <= p.minres) s.status = kCfConverged;
    } else {
      s.damp = s.damp * p.damp_fct;
    }
  }
  if (take)
    for (int f = 0; f < nframes; ++f) {
      for (int q = 0; q < 21; ++q) s.U[21 * f + q] = sums[kCfSlots * f + q];
      for (int q = 0; q < 6; ++q) s.gc[6 * f + q] = sums[kCfSlots * f + 21 + q];
    }
  s.phase = kBaRetry;  // no trial stands until a solve succeeds
  if (s.status == kCfRunning) ba_stops(s, p);
}

// behind the reduced solve: a step dc (6 (F - 1)) moves the trial poses, a failed solve raises the damping, counts an
// iteration and meets the stops again
ICTR_HD void ba_solved(BaState &s, bool ok, const double *dc, int nframes, const CfParams &p) {
  if (ok) {
    for (int q = 0; q < 12; ++q) s.Gt[q] = s.G[q];
    for (int f = 1; f < nframes; ++f) {
      for (int q = 0; q < 6; ++q) s.dc[6 * (f - 1) + q] = dc[6 * (f - 1) + q];
      cf_update(s.G + 12 * f, dc + 6 * (f - 1), s.Gt + 12 * f);
    }
    s.tset = s.cur ^ 1;
    s.phase = kBaTrial;
  } else {
    s.damp = s.damp * p.damp_fct;
    s.it = s.it + 1;
    s.phase = kBaRetry;
    ba_stops(s, p);
  }
}

// is point m adjusted: xy [S][F][2][n]
ICTR_HD bool ba_adjusted(bool bit, const double *X, const double *xy, long long n, int nframes, int nsides, long long m) {
  bool ok = bit && cf_finite(X[m]) && cf_finite(X[n + m]) && cf_finite(X[2 * n + m]);
  for (int q = 0; q < 2 * nsides * nframes; ++q) ok = ok && cf_finite(xy[(long long)q * n + m]);
  return ok;
}

#if !defined(__HIP_DEVICE_COMPILE__)

// The whole adjustment on the host, serially, in the stated order.
struct BaHost {
  long long n = 0;
  int nframes = 0, nsides = 0;
  CfCam cam = {0, 0, 0, 0};
  double off[2][3] = {{0, 0, 0}, {0, 0, 0}};
  const double *xy = nullptr;   // [S][F][2][n]
  std::vector<unsigned char> adj;
  std::vector<double> X[2], V[2], gp[2];  // the two point sets: [3][n], [6][n], [3][n]
  std::vector<double> fsums, T, A, rhs;   // [F][32], [npairs][48], packed triangle, right-hand side
  long long nfail = 0;
  BaState st;

  void setup(const double *X0, const double *xy_, const unsigned long long *words, long long n_, int F, int S,
             const CfCam &k, const double *offset) {
    n = n_, nframes = F, nsides = S, cam = k, xy = xy_;
    for (int q = 0; q < 3; ++q) off[1][q] = offset ? offset[q] : 0.0;
    adj.assign((size_t)n, 0);
    for (int e = 0; e < 2; ++e) {
      X[e].assign(X0, X0 + 3 * n);
      V[e].assign((size_t)(6 * n), 0.0);
      gp[e].assign((size_t)(3 * n), 0.0);
    }
    for (long long m = 0; m < n; ++m) {
      const bool bit = words ? ((words[m >> 6] >> (m & 63)) & 1ull) != 0 : true;
      adj[(size_t)m] = ba_adjusted(bit, X0, xy, n, F, S, m) ? 1 : 0;
    }
    fsums.assign((size_t)(kCfSlots * F), 0.0);
    T.assign((size_t)(kBaPairSlots * (ba_npairs(F) > 0 ? ba_npairs(F) : 1)), 0.0);
    const int dim = 6 * (F - 1);
    A.assign((size_t)(dim * (dim + 1) / 2), 0.0);
    rhs.assign((size_t)dim, 0.0);
  }
  void obs(const double *G, int f, int s, int e, long long m, BaObs &b) const {
    const double *o = xy + ((long long)s * nframes + f) * 2 * n;
    ba_obs(G + 12 * f, off[s], cam, X[e][m], X[e][n + m], X[e][2 * n + m], o[m], o[n + m], b);
  }
  // V, gp of every point of set e at the poses G
  void point_pass(const double *G, int e) {
    for (long long m = 0; m < n; ++m) {
      double v[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
      if (adj[(size_t)m])
        for (int f = 0; f < nframes; ++f)
          for (int s = 0; s < nsides; ++s) {
            BaObs b;
            obs(G, f, s, e, m, b);
            ba_add_point(b, v, g);
          }
      for (int q = 0; q < 6; ++q) V[e][q * n + m] = v[q];
      for (int q = 0; q < 3; ++q) gp[e][q * n + m] = g[q];
    }
  }
  // the ordered sum over the points of nt terms; term(m, t) fills the terms of point m
  template <class Fn>
  void ordered(int nt, double *out, Fn term) const {
    std::vector<double> v((size_t)nt * kCfBlock), tot((size_t)nt, 0.0), acc((size_t)nt), t((size_t)nt);
    const long long nchunks = (n + kCfChunk - 1) / kCfChunk;
    for (long long ch = 0; ch < nchunks; ++ch) {
      for (int l = 0; l < kCfBlock; ++l) {
        for (int q = 0; q < nt; ++q) acc[q] = 0.0;
        for (int r = 0; r < kCfPerLane; ++r) {
          const long long m = ch * kCfChunk + (long long)r * kCfBlock + l;
          if (m >= n) continue;
          for (int q = 0; q < nt; ++q) t[q] = 0.0;
          if (adj[(size_t)m]) term(m, t.data());
          for (int q = 0; q < nt; ++q) acc[q] = acc[q] + t[q];
        }
        for (int q = 0; q < nt; ++q) v[(size_t)q * kCfBlock + l] = acc[q];
      }
      for (int s = 1; s < kCfBlock; s *= 2)
        for (int i = 0; i < kCfBlock; i += 2 * s)
          for (int q = 0; q < nt; ++q) v[(size_t)q * kCfBlock + i] = v[(size_t)q * kCfBlock + i] + v[(size_t)q * kCfBlock + i + s];
      for (int q = 0; q < nt; ++q) tot[q] = tot[q] + v[(size_t)q * kCfBlock];
    }
    for (int q = 0; q < nt; ++q) out[q] = cf_canon(tot[q]);
  }
  // the frames' sums of set e at the poses G
  void frame_pass(const double *G, int e) {
    long long cnt = 0;
    for (long long m = 0; m < n; ++m) cnt += adj[(size_t)m];
    for (int f = 0; f < nframes; ++f) {
      double *o = fsums.data() + kCfSlots * f;
      for (int q = 0; q < kCfSlots; ++q) o[q] = 0.0;
      ordered(kCfTerms, o, [&](long long m, double *t) {
        for (int s = 0; s < nsides; ++s) {
          BaObs b;
          obs(G, f, s, e, m, b);
          ba_add_cam(b, t);
        }
      });
      o[kCfCountSlot] = (double)cnt;
    }
  }
  void w_of(const double *G, int f, int e, long long m, double *W) const {
    for (int q = 0; q < 18; ++q) W[q] = 0.0;
    for (int s = 0; s < nsides; ++s) {
      BaObs b;
      obs(G, f, s, e, m, b);
      ba_add_w(b, W);
    }
  }
  // the pairs' sums of set e at the poses G, and the points whose factorisation failed
  void schur_pass(const double *G, int e, double damp) {
    nfail = 0;
    for (long long m = 0; m < n; ++m)
      if (adj[(size_t)m]) {
        double v[6], L[3], D[3];
        for (int q = 0; q < 6; ++q) v[q] = V[e][q * n + m];
        nfail += ba_factor3(v, damp, L, D) ? 0 : 1;
      }
    for (int p = 0; p < ba_npairs(nframes); ++p) {
      int f, g;
      ba_pair(nframes, p, f, g);
      double *o = T.data() + (size_t)kBaPairSlots * p;
      for (int q = 0; q < kBaPairSlots; ++q) o[q] = 0.0;
      ordered(kBaPairTerms, o, [&](long long m, double *t) {
        double v[6], gq[3], L[3], D[3], Wf[18], Wg[18];
        for (int q = 0; q < 6; ++q) v[q] = V[e][q * n + m];
        for (int q = 0; q < 3; ++q) gq[q] = gp[e][q * n + m];
        ba_factor3(v, damp, L, D);
        w_of(G, f, e, m, Wf);
        w_of(G, g, e, m, Wg);
        ba_pair_terms(Wf, Wg, L, D, gq, t);
      });
      o[kBaFailSlot] = (double)nfail;
    }
  }
  void assemble(const double *U, const double *gc, double damp) {
    const int dim = 6 * (nframes - 1);
    for (int I = 0; I < dim; ++I) {
      for (int J = I; J < dim; ++J) A[(size_t)ba_ridx(dim, I, J)] = ba_reduced_entry(U, T.data(), nframes, damp, I, J);
      rhs[(size_t)I] = ba_reduced_rhs(gc, T.data(), nframes, I);
    }
  }
  // the reduced solve in place of A; false on a bad pivot
  bool reduced_solve(double *dc) {
    const int dim = 6 * (nframes - 1);
    std::vector<double> col((size_t)dim);
    bool ok = nfail == 0;
    for (int j = 0; j < dim && ok; ++j) {
      for (int i = j; i < dim; ++i) col[(size_t)i] = ba_ldl_sum(A.data(), dim, j, i);
      const double d = col[(size_t)j];
      if (!ba_pivot_ok(d)) ok = false;
      A[(size_t)ba_ridx(dim, j, j)] = d;
      for (int i = j + 1; i < dim; ++i) A[(size_t)ba_ridx(dim, j, i)] = col[(size_t)i] / d;
    }
    if (ok) ba_ldl_solve(A.data(), dim, rhs.data(), dc);
    return ok;
  }
  // the points of set `to` from set `from` moved by the step dc at the poses G
  void back_pass(const double *G, int from, int to, double damp, const double *dc) {
    for (long long m = 0; m < n; ++m) {
      double x[3] = {X[from][m], X[from][n + m], X[from][2 * n + m]};
      if (adj[(size_t)m]) {
        double v[6], b[3], L[3], D[3], W[18], d[3];
        for (int q = 0; q < 6; ++q) v[q] = V[from][q * n + m];
        for (int q = 0; q < 3; ++q) b[q] = gp[from][q * n + m];
        ba_factor3(v, damp, L, D);
        for (int f = 1; f < nframes; ++f) {
          w_of(G, f, from, m, W);
          ba_back_rhs(W, dc + 6 * (f - 1), b);
        }
        ba_solve3(L, D, b, d);
        for (int q = 0; q < 3; ++q) x[q] = x[q] + d[q];
      }
      for (int q = 0; q < 3; ++q) X[to][q * n + m] = x[q];
    }
  }
  void run(const double *G0, const CfParams &p) {
    ba_init(st, G0, nframes, p);
    std::vector<double> dc((size_t)(6 * (nframes - 1)));
    while (st.status == kCfRunning) {
      if (st.phase != kBaRetry) {
        point_pass(st.Gt, st.tset);
        frame_pass(st.Gt, st.tset);
      }
      ba_decide(st, fsums.data(), nframes, nsides, p);
      if (st.status != kCfRunning) break;
      schur_pass(st.G, st.cur, st.damp);
      assemble(st.U, st.gc, st.damp);
      const bool ok = reduced_solve(dc.data());
      ba_solved(st, ok, dc.data(), nframes, p);
      if (st.status == kCfRunning && st.phase == kBaTrial) back_pass(st.G, st.cur, st.tset, st.damp, st.dc);
    }
  }
};
#endif

}  // namespace ictr
