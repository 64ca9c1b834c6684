// ictr_p3p_hd.h -- the P3P hypothesis of the RANSAC stages, stated once: Lambda Twist (Persson and Nordberg 2018) and the
// body of one trial after its draws -- undistortion of the four pixels, the script's degeneracy test, the solver on the
// first three matches and the root that reprojects the fourth nearest. The same text compiles for the device
// (k_ransac_hyp of ictr_ransac.hip, k_cr_hyp of ictr_camransac.hip) and, as plain C++ under sanitizers, for
// tests/cxx/camransac_hd_host.cpp (tests/test_camransac_cpu.py); invcompcamtrack_amd/ransac.py (p3p, _hypothesis)
// restates it operation by operation. f64 in the order written (the library builds with -ffp-contract=off).
#pragma once

#include <math.h>

#include "se3_math.h"

namespace ictr {

ICTR_HD double triple(const double *a, const double *b, const double *c) {
  const double c0 = a[1] * b[2] - a[2] * b[1];
  const double c1 = a[2] * b[0] - a[0] * b[2];
  const double c2 = a[0] * b[1] - a[1] * b[0];
  return c0 * c[0] + c1 * c[1] + c2 * c[2];
}

// real roots of x^2 + b x + c (stable form); false when complex
ICTR_HD bool root2real(double b, double c, double &r1, double &r2) {
  const double v = b * b - 4.0 * c;
  if (v < 0.0) return false;
  const double y = sqrt(v);
  const double q = b < 0.0 ? 0.5 * (-b + y) : 0.5 * (-b - y);
  r1 = q;
  r2 = q != 0.0 ? c / q : 0.0;
  return true;
}

// an extreme real root of x^3 + b x^2 + c x + d (Lambda Twist's cubick)
ICTR_HD double cubick(double b, double c, double d) {
  double r0;
  if (b * b >= 3.0 * c) {
    const double v = sqrt(b * b - 3.0 * c);
    const double t1 = (-b - v) / 3.0;
    double k = ((t1 + b) * t1 + c) * t1 + d;
    if (k > 0.0) {
      r0 = t1 - sqrt(-k / (3.0 * t1 + b));
    } else {
      const double t2 = (-b + v) / 3.0;
      k = ((t2 + b) * t2 + c) * t2 + d;
      r0 = t2 + sqrt(-k / (3.0 * t2 + b));
    }
  } else {
    r0 = -b / 3.0;
    if (fabs((3.0 * r0 + 2.0 * b) * r0 + c) < 1e-4) r0 += 1.0;
  }
  for (int it = 0; it < 50; ++it) {
    const double fx = ((r0 + b) * r0 + c) * r0 + d;
    if (it >= 7 && fabs(fx) <= 1e-13) break;
    const double fpx = (3.0 * r0 + 2.0 * b) * r0 + c;
    r0 -= fx / fpx;
  }
  return r0;
}

// eigenvector of the symmetric 3x3 A (row-major) for eigenvalue lam: the longest cross product of two rows of A - lam I
ICTR_HD void cross_keep(const double *a, const double *b, double &best, double *v) {
  const double c0 = a[1] * b[2] - a[2] * b[1], c1 = a[2] * b[0] - a[0] * b[2], c2 = a[0] * b[1] - a[1] * b[0];
  const double n = c0 * c0 + c1 * c1 + c2 * c2;
  if (n > best) {
    best = n;
    v[0] = c0;
    v[1] = c1;
    v[2] = c2;
  }
}
ICTR_HD void eigvec(const double *A, double lam, double *v) {
  const double r0[3] = {A[0] - lam, A[1], A[2]}, r1[3] = {A[3], A[4] - lam, A[5]}, r2[3] = {A[6], A[7], A[8] - lam};
  double best = -1.0;
  cross_keep(r0, r1, best, v);
  cross_keep(r0, r2, best, v);
  cross_keep(r1, r2, best, v);
  const double s = 1.0 / sqrt(best);
  v[0] *= s;
  v[1] *= s;
  v[2] *= s;
}

// Gauss-Newton on the three distance equations (Lambda Twist's refinement)
ICTR_HD void refine_lambda(double *L, double a12, double a13, double a23, double b12, double b13, double b23) {
  for (int it = 0; it < 5; ++it) {
    const double l1 = L[0], l2 = L[1], l3 = L[2];
    const double r1 = l1 * l1 + l2 * l2 + b12 * l1 * l2 - a12;
    const double r2 = l1 * l1 + l3 * l3 + b13 * l1 * l3 - a13;
    const double r3 = l2 * l2 + l3 * l3 + b23 * l2 * l3 - a23;
    const double e0 = fabs(r1) + fabs(r2) + fabs(r3);
    if (e0 < 1e-10) break;
    const double v0 = 2.0 * l1 + b12 * l2, v1 = 2.0 * l2 + b12 * l1;
    const double v3 = 2.0 * l1 + b13 * l3, v5 = 2.0 * l3 + b13 * l1;
    const double v7 = 2.0 * l2 + b23 * l3, v8 = 2.0 * l3 + b23 * l2;
    const double det = 1.0 / (-v0 * v5 * v7 - v1 * v3 * v8);
    const double n1 = l1 - det * (-v5 * v7 * r1 - v1 * v8 * r2 + v1 * v5 * r3);
    const double n2 = l2 - det * (-v3 * v8 * r1 + v0 * v8 * r2 - v0 * v5 * r3);
    const double n3 = l3 - det * (v3 * v7 * r1 - v0 * v7 * r2 - v1 * v3 * r3);
    const double s1 = n1 * n1 + n2 * n2 + b12 * n1 * n2 - a12;
    const double s2 = n1 * n1 + n3 * n3 + b13 * n1 * n3 - a13;
    const double s3 = n2 * n2 + n3 * n3 + b23 * n2 * n3 - a23;
    if (fabs(s1) + fabs(s2) + fabs(s3) > e0) break;
    L[0] = n1;
    L[1] = n2;
    L[2] = n3;
  }
}

// cofactor matrix of a symmetric 3x3 (row-major; symmetric as well)
ICTR_HD void cof3(const double *A, double *C) {
  C[0] = A[4] * A[8] - A[5] * A[7];
  C[1] = A[5] * A[6] - A[3] * A[8];
  C[2] = A[3] * A[7] - A[4] * A[6];
  C[3] = A[2] * A[7] - A[1] * A[8];
  C[4] = A[0] * A[8] - A[2] * A[6];
  C[5] = A[1] * A[6] - A[0] * A[7];
  C[6] = A[1] * A[5] - A[2] * A[4];
  C[7] = A[2] * A[3] - A[0] * A[5];
  C[8] = A[0] * A[4] - A[1] * A[3];
}

// P3P, Lambda Twist (Persson and Nordberg 2018): bearings y (unit), world points x. Every solution (R, T), y ~ R x + T,
// is handed to use(R, T) in a fixed order as it is found: +v before -v, the larger-magnitude tau first.
template <class Use>
ICTR_HD void p3p_lambda_twist(const double (*y)[3], const double (*x)[3], Use &&use) {
  const double b12 = -2.0 * (y[0][0] * y[1][0] + y[0][1] * y[1][1] + y[0][2] * y[1][2]);
  const double b13 = -2.0 * (y[0][0] * y[2][0] + y[0][1] * y[2][1] + y[0][2] * y[2][2]);
  const double b23 = -2.0 * (y[1][0] * y[2][0] + y[1][1] * y[2][1] + y[1][2] * y[2][2]);
  double d12[3], d13[3], d23[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    d12[k] = x[0][k] - x[1][k];
    d13[k] = x[0][k] - x[2][k];
    d23[k] = x[1][k] - x[2][k];
  }
  const double a12 = d12[0] * d12[0] + d12[1] * d12[1] + d12[2] * d12[2];
  const double a13 = d13[0] * d13[0] + d13[1] * d13[1] + d13[2] * d13[2];
  const double a23 = d23[0] * d23[0] + d23[1] * d23[1] + d23[2] * d23[2];
  // D1 = a23 M12 - a12 M23, D2 = a23 M13 - a13 M23; det(D1 - g D2) = c3 g^3 + c2 g^2 + c1 g + c0
  const double D1[9] = {a23, 0.5 * a23 * b12, 0.0, 0.5 * a23 * b12, a23 - a12, -0.5 * a12 * b23,
                        0.0, -0.5 * a12 * b23, -a12};
  const double D2[9] = {a23, 0.0, 0.5 * a23 * b13, 0.0, -a13, -0.5 * a13 * b23,
                        0.5 * a23 * b13, -0.5 * a13 * b23, a23 - a13};
  double C1[9], C2[9];
  cof3(D1, C1);
  cof3(D2, C2);
  double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {  // the determinants along the first row
    c0 += D1[k] * C1[k];
    c3 += D2[k] * C2[k];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    c1 += C1[k] * D2[k];
    c2 += D1[k] * C2[k];
  }
  c3 = -c3;
  c1 = -c1;
  if (!(fabs(c3) > 0.0) || !isfinite(c3)) return;
  const double g = cubick(c2 / c3, c1 / c3, c0 / c3);
  double A[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) A[k] = D1[k] - g * D2[k];
  // A is of rank 2: its nonzero eigenvalues solve e^2 - tr e + m = 0 (m: sum of the principal 2x2 minors)
  const double tr = A[0] + A[4] + A[8];
  const double m = (A[0] * A[4] - A[1] * A[3]) + (A[0] * A[8] - A[2] * A[6]) + (A[4] * A[8] - A[5] * A[7]);
  double e1, e2;
  if (!root2real(-tr, m, e1, e2)) return;
  if (fabs(e1) < fabs(e2)) {
    const double s = e1;
    e1 = e2;
    e2 = s;
  }
  if (!(fabs(e1) > 0.0)) return;
  double V0[3], V1[3];
  eigvec(A, e1, V0);
  eigvec(A, e2, V1);
  const double v = sqrt(fmax(0.0, -e2 / e1));
  // inv(X), X = [d12 d13 d12 x d13] (columns): cof3 is the plain cofactor matrix, inv(X) = cof^T / det
  const double xc3[3] = {d12[1] * d13[2] - d12[2] * d13[1], d12[2] * d13[0] - d12[0] * d13[2],
                         d12[0] * d13[1] - d12[1] * d13[0]};
  const double X[9] = {d12[0], d13[0], xc3[0], d12[1], d13[1], xc3[1], d12[2], d13[2], xc3[2]};
  double CX[9];
  cof3(X, CX);
  const double detX = X[0] * CX[0] + X[1] * CX[1] + X[2] * CX[2];
  if (!(fabs(detX) > 0.0)) return;
  const double idet = 1.0 / detX;
  double Xi[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) Xi[r * 3 + c] = CX[c * 3 + r] * idet;
#pragma unroll
  for (int sg = 0; sg < 2; ++sg) {
    const double s = sg == 0 ? v : -v;
    const double w2 = 1.0 / (s * V1[0] - V0[0]);
    const double w0 = (V0[1] - s * V1[1]) * w2;
    const double w1 = (V0[2] - s * V1[2]) * w2;
    const double ia = 1.0 / ((a13 - a12) * w1 * w1 - a12 * b13 * w1 - a12);
    const double qb = (a13 * b12 * w1 - a12 * b13 * w0 - 2.0 * w0 * w1 * (a12 - a13)) * ia;
    const double qc = ((a13 - a12) * w0 * w0 + a13 * b12 * w0 + a13) * ia;
    double tau[2];
    if (!root2real(qb, qc, tau[0], tau[1])) continue;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      if (!(tau[q] > 0.0)) continue;
      const double d = a23 / (tau[q] * (b23 + tau[q]) + 1.0);
      if (!(d > 0.0)) continue;
      double L[3];
      L[1] = sqrt(d);
      L[2] = tau[q] * L[1];
      L[0] = w0 * L[1] + w1 * L[2];
      if (!(L[0] >= 0.0)) continue;
      refine_lambda(L, a12, a13, a23, b12, b13, b23);
      double ry[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) ry[i][k] = y[i][k] * L[i];
      double yd1[3], yd2[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        yd1[k] = ry[0][k] - ry[1][k];
        yd2[k] = ry[0][k] - ry[2][k];
      }
      const double yc[3] = {yd1[1] * yd2[2] - yd1[2] * yd2[1], yd1[2] * yd2[0] - yd1[0] * yd2[2],
                            yd1[0] * yd2[1] - yd1[1] * yd2[0]};
      const double Y[9] = {yd1[0], yd2[0], yc[0], yd1[1], yd2[1], yc[1], yd1[2], yd2[2], yc[2]};
      double R[9], T[3];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          R[r * 3 + c] = Y[r * 3 + 0] * Xi[0 * 3 + c] + Y[r * 3 + 1] * Xi[1 * 3 + c] + Y[r * 3 + 2] * Xi[2 * 3 + c];
#pragma unroll
      for (int r = 0; r < 3; ++r)
        T[r] = ry[0][r] - (R[r * 3 + 0] * x[0][0] + R[r * 3 + 1] * x[0][1] + R[r * 3 + 2] * x[0][2]);
      use(R, T);
    }
  }
}

// One trial after its draws: P the four 3-D points, (u, v) their four pixels. Undistortion, degeneracy, P3P and the choice
// of root. Returns 1 and fills R (row-major) and t (the camera centre) on success.
ICTR_HD int p3p_hypothesis(const double (*P)[3], const double *u, const double *v, double fx, double fy, double cx,
                           double cy, double kc, double *Rout, double *tout) {
  double x2[4][3];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double xd = (u[q] - cx) / fx, yd = (v[q] - cy) / fy;
    double xn = xd, yn = yd;
    for (int it = 0; it < 20; ++it) {
      const double f = 1.0 + kc * (xn * xn + yn * yn);
      xn = xd / f;
      yn = yd / f;
    }
    x2[q][0] = xn * fx + cx;
    x2[q][1] = yn * fy + cy;
    x2[q][2] = 1.0;
  }
  const double eps = 2.220446049250313e-16;  // MATLAB's eps
  // degenfn_P: every triple of nchoosek(1:4, 3), 3-D points, then the homogeneous undistorted 2-D points
  if (fabs(triple(P[0], P[1], P[2])) < eps || fabs(triple(P[0], P[1], P[3])) < eps ||
      fabs(triple(P[0], P[2], P[3])) < eps || fabs(triple(P[1], P[2], P[3])) < eps)
    return 0;
  if (fabs(triple(x2[0], x2[1], x2[2])) < eps || fabs(triple(x2[0], x2[1], x2[3])) < eps ||
      fabs(triple(x2[0], x2[2], x2[3])) < eps || fabs(triple(x2[1], x2[2], x2[3])) < eps)
    return 0;
  double yb[3][3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const double bx = (x2[q][0] - cx) / fx, by = (x2[q][1] - cy) / fy;
    const double s = 1.0 / sqrt(bx * bx + by * by + 1.0);
    yb[q][0] = bx * s;
    yb[q][1] = by * s;
    yb[q][2] = s;
  }
  double best = INFINITY;
  int found = 0;
  p3p_lambda_twist(yb, P, [&](const double *R, const double *T) {
    double t[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = -(R[0 * 3 + c] * T[0] + R[1 * 3 + c] * T[1] + R[2 * 3 + c] * T[2]);
    const double dX = P[3][0] - t[0], dY = P[3][1] - t[1], dZ = P[3][2] - t[2];
    const double xc = R[0] * dX + R[1] * dY + R[2] * dZ;
    const double yc = R[3] * dX + R[4] * dY + R[5] * dZ;
    const double zc = R[6] * dX + R[7] * dY + R[8] * dZ;
    const double iz = 1.0 / zc;
    const double du = fx * (xc * iz) + cx - x2[3][0], dv = fy * (yc * iz) + cy - x2[3][1];
    const double e = du * du + dv * dv;
    if (e < best) {  // strict: the first of equal errors stays
      best = e;
      found = 1;
#pragma unroll
      for (int k = 0; k < 9; ++k) Rout[k] = R[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) tout[k] = t[k];
    }
  });
  return found;
}

}  // namespace ictr
