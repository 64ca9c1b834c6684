// ictr_fsplit_hd.h -- the bit-pinned steps of the static split (ictr_fsplit.hip), each stated once: the 8-point
// fundamental matrix of one sample and the distance of a point to its epipolar line. Compiled from the same text for the
// device (k_fsplit_fit, k_fsplit_score, k_fsplit_mask) and, as plain C++, for the host (tests/cxx/fsplit_hd_host.cpp, built
// with sanitizers by tests/test_fsplit_cpu.py); invcompcamtrack_amd/fsplit.py restates them operation by operation. Only + - * / sqrt occur, in f64, in the order
// written (the library builds with -ffp-contract=off). Every array below is indexed by constants of fully unrolled
// loops: choices that depend on the data (pivot row and column, the column to drop) are select chains.
#pragma once

#include <math.h>

#include "se3_math.h"

namespace ictr {

constexpr int kFsSweeps = 5;  // Jacobi sweeps of the rank-2 step (DESIGN.md §4 "Static split": 4 needed, one spare)

ICTR_HD double fs_nan() { return __builtin_nan(""); }  // the one NaN that outputs carry (0x7ff8000000000000)

// Hartley normalisation of 8 points: x <- (x - cx) s, y <- (y - cy) s in place; s, tx = -(s cx), ty = -(s cy) are the
// entries of T. Returns false when the mean distance is 0.
ICTR_HD bool fs_normalise(double *x, double *y, double &s, double &tx, double &ty) {
  s = tx = ty = 0.0;
  double sx = x[0], sy = y[0];
#pragma unroll
  for (int k = 1; k < 8; ++k) {
    sx = sx + x[k];
    sy = sy + y[k];
  }
  const double cx = sx / 8.0, cy = sy / 8.0;
  double sd = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    x[k] = x[k] - cx;
    y[k] = y[k] - cy;
    sd = sd + sqrt(x[k] * x[k] + y[k] * y[k]);
  }
  const double d = sd / 8.0;
  if (d == 0.0) return false;
  s = 1.4142135623730951 / d;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    x[k] = x[k] * s;
    y[k] = y[k] * s;
  }
  tx = -(s * cx);
  ty = -(s * cy);
  return true;
}

ICTR_HD void fs_cswap(bool c, double &a, double &b) {
  const double t = a;
  a = c ? b : a;
  b = c ? t : b;
}

// one Hestenes rotation of the column pair (p, q) of U (3x3, row-major) and of V
template <int P, int Q>
ICTR_HD void fs_rotate(double *U, double *V) {
  const double al = (U[P] * U[P] + U[3 + P] * U[3 + P]) + U[6 + P] * U[6 + P];
  const double be = (U[Q] * U[Q] + U[3 + Q] * U[3 + Q]) + U[6 + Q] * U[6 + Q];
  const double ga = (U[P] * U[Q] + U[3 + P] * U[3 + Q]) + U[6 + P] * U[6 + Q];
  if (ga == 0.0) return;
  const double ze = (be - al) / (2.0 * ga);
  const double t = (ze < 0.0 ? -1.0 : 1.0) / (fabs(ze) + sqrt(1.0 + ze * ze));
  const double c = 1.0 / sqrt(1.0 + t * t);
  const double s = c * t;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double up = U[3 * r + P], uq = U[3 * r + Q];
    U[3 * r + P] = c * up - s * uq;
    U[3 * r + Q] = s * up + c * uq;
    const double vp = V[3 * r + P], vq = V[3 * r + Q];
    V[3 * r + P] = c * vp - s * vq;
    V[3 * r + Q] = s * vp + c * vq;
  }
}

// The fundamental matrix F (row-major, xb^T F xa = 0, unit Frobenius norm) of 8 correspondences. Returns false (F =
// fs_nan() nine times) when a mean distance is 0, a pivot is exactly 0 or an entry of F is not finite.
ICTR_HD bool fs_fit8(const double *xa_in, const double *ya_in, const double *xb_in, const double *yb_in, double *F) {
  double xa[8], ya[8], xb[8], yb[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    xa[k] = xa_in[k];
    ya[k] = ya_in[k];
    xb[k] = xb_in[k];
    yb[k] = yb_in[k];
  }
  double sa, txa, tya, sb, txb, tyb;
  bool ok = fs_normalise(xa, ya, sa, txa, tya);
  ok = fs_normalise(xb, yb, sb, txb, tyb) && ok;
  double A[8][9];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    A[r][0] = xb[r] * xa[r];
    A[r][1] = xb[r] * ya[r];
    A[r][2] = xb[r];
    A[r][3] = yb[r] * xa[r];
    A[r][4] = yb[r] * ya[r];
    A[r][5] = yb[r];
    A[r][6] = xa[r];
    A[r][7] = ya[r];
    A[r][8] = 1.0;
  }
  int perm[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) perm[j] = j;
  // Gaussian elimination, full pivoting: the largest |a| of rows k.., columns k..; ties: lowest row, then lowest column
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    double best = fabs(A[k][k]);
    int pr = k, pc = k;
#pragma unroll
    for (int i = k; i < 8; ++i)
#pragma unroll
      for (int j = k; j < 9; ++j) {
        const double v = fabs(A[i][j]);
        const bool g = v > best;
        best = g ? v : best;
        pr = g ? i : pr;
        pc = g ? j : pc;
      }
#pragma unroll
    for (int i = k + 1; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 9; ++j) fs_cswap(pr == i, A[k][j], A[i][j]);
#pragma unroll
    for (int j = k + 1; j < 9; ++j) {
      const bool c = pc == j;
#pragma unroll
      for (int i = 0; i < 8; ++i) fs_cswap(c, A[i][k], A[i][j]);
      const int t = perm[k];
      perm[k] = c ? perm[j] : perm[k];
      perm[j] = c ? t : perm[j];
    }
    const double piv = A[k][k];
    if (piv == 0.0) ok = false;
#pragma unroll
    for (int i = k + 1; i < 8; ++i) {
      const double f = A[i][k] / piv;
#pragma unroll
      for (int j = k + 1; j < 9; ++j) A[i][j] = A[i][j] - f * A[k][j];
    }
  }
  // the null vector: free variable (column 8 of the permuted system) = 1, back-substitution
  double z[9];
  z[8] = 1.0;
#pragma unroll
  for (int k = 7; k >= 0; --k) {
    double acc = A[k][k + 1] * z[k + 1];
#pragma unroll
    for (int j = k + 2; j < 9; ++j) acc = acc + A[k][j] * z[j];
    z[k] = -acc / A[k][k];
  }
  double U[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    double v = z[0];
#pragma unroll
    for (int j = 1; j < 9; ++j) v = perm[j] == t ? z[j] : v;
    U[t] = v;
  }
  // rank 2: one-sided Jacobi, U <- U V with orthogonal columns; the shortest column dropped; back by V^T
  double V[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
#pragma unroll 1
  for (int sw = 0; sw < kFsSweeps; ++sw) {
    fs_rotate<0, 1>(U, V);
    fs_rotate<0, 2>(U, V);
    fs_rotate<1, 2>(U, V);
  }
  const double n0 = (U[0] * U[0] + U[3] * U[3]) + U[6] * U[6];
  const double n1 = (U[1] * U[1] + U[4] * U[4]) + U[7] * U[7];
  const double n2 = (U[2] * U[2] + U[5] * U[5]) + U[8] * U[8];
  int drop = 0;
  double nm = n0;
  if (n1 < nm) {
    nm = n1;
    drop = 1;
  }
  if (n2 < nm) drop = 2;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    U[3 * r + 0] = drop == 0 ? 0.0 : U[3 * r + 0];
    U[3 * r + 1] = drop == 1 ? 0.0 : U[3 * r + 1];
    U[3 * r + 2] = drop == 2 ? 0.0 : U[3 * r + 2];
  }
  double G[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      G[3 * r + c] = (U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1]) + U[3 * r + 2] * V[3 * c + 2];
  // F = Tb^T G Ta
  double H[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    H[3 * r + 0] = G[3 * r + 0] * sa;
    H[3 * r + 1] = G[3 * r + 1] * sa;
    H[3 * r + 2] = (G[3 * r + 0] * txa + G[3 * r + 1] * tya) + G[3 * r + 2];
  }
  double ss = 0.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    F[c] = sb * H[c];
    F[3 + c] = sb * H[3 + c];
    F[6 + c] = (txb * H[c] + tyb * H[3 + c]) + H[6 + c];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) ss = ss + F[k] * F[k];
  const double nrm = sqrt(ss);
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    F[k] = F[k] / nrm;
    if (!(fabs(F[k]) <= 1.7976931348623157e308)) ok = false;  // NaN or infinite
  }
  if (!ok) {
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = fs_nan();
  }
  return ok;
}

// func_F_transfer_points (func_util_geom.py:52-55): distance of (xb, yb) to the epipolar line F (xa, ya, 1)
ICTR_HD double fs_dist(const double *F, double xa, double ya, double xb, double yb) {
  const double l0 = ((F[0] * xa) + (F[1] * ya)) + F[2];
  const double l1 = ((F[3] * xa) + (F[4] * ya)) + F[5];
  const double l2 = ((F[6] * xa) + (F[7] * ya)) + F[8];
  return fabs(((l0 * xb) + (l1 * yb)) + l2) / sqrt(l0 * l0 + l1 * l1);
}

// the running maximum over the pairs; a NaN stays (as fs_nan()). Start from -1.
ICTR_HD double fs_max(double mx, double d) { return d != d ? fs_nan() : (d > mx ? d : mx); }

}  // namespace ictr
