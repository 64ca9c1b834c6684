"""RANSAC pose sampling from 2-D/3-D matches and its odometry verification: func_ransac_fitcameras_odom.m, the function
run_ransac_test.m calls, with the hypothesis stage on the device (ictr_ransac_*) and the verification through
run_track_nposes.

Semantics (0-based inside, 1-based inlier ids in files; deviations from the script in DESIGN.md §4):

- trial ``t`` draws from a counter-based stream: ``u_k = mix(mix(seed) ^ ((t << 32) | k))``, ``mix`` = splitmix64,
  index ``((u_k >> 32) * N) >> 32``; repeats are skipped, the first 4 distinct indices are kept in draw order. This
  replaces ``randsample``: samples are not reproducible against MATLAB, but every run is bit-reproducible.
  The shift is taken in 64 bits, so the stream has period 2^32 in ``t``: trial ``2^32 + j`` draws what trial ``j``
  draws (and so computes the same hypothesis). Runs of 2^32 trials or more repeat themselves.
- undistortion for the solver (:22-24): normalise, ``x_n <- x_d / (1 + kc |x_n|^2)`` 20 times, back to pixels. The
  one-coefficient model is not pinned by the reference (its ``func_undist_kc`` / ``func_reproject`` are not part of
  it); ``kc = 0`` is the plain pinhole.
- degeneracy (``degenfn_P``, :175-194), literally: any triple with ``|dot(cross(p1, p2), p3)| < 2^-52`` over the 3-D
  points (coplanar with the origin, not collinear: the script's quirk) or the homogeneous undistorted 2-D points.
- P3P (Lambda Twist) on the first three drawn matches replaces ASPnP; of its solutions the one that reprojects the
  fourth match nearest is taken (first on ties). None: the trial fails.
- inliers (:44-49): ``x_cam = R (X - t)``, pinhole + forward distortion, ``sqrt(dx^2 + dy^2) <= inlthresh`` against
  the original ``pt2d`` in f64; no depth test. A trial succeeds with >= 4 inliers.
- acceptance (:29-72): the first ``nsamples`` successes among trials ``0 .. maxtrials-1``; fewer (or none) is a
  normal result.
- post-filter (:76-87): ``inl_cnt`` is per match; sample ``s`` is dropped when ``s < N`` and ``inl_cnt[s] <= 4``
  (the script's logical index over matches applied to samples; MATLAB would raise where a flagged index is >= the
  sample count, here that part is ignored). ``inl_cnt`` loses its entries ``<= 4``.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import _lib
from ._hostmath import M64 as _M64, div as _div, draw_indices_n, se3_exp_d as _se3_exp_d
from ._lib import check, dp, f64c

__all__ = ["sample_poses", "sample_poses_host", "fit_cameras_odom", "best_sample", "draw_indices", "undistort",
           "distort", "is_degenerate", "p3p"]

_EPS = 2.0 ** -52


def draw_indices(seed, t, n, max_draws=1024):
    """The 4 distinct match indices of trial t (draw order), or None when max_draws draws do not give 4."""
    out = draw_indices_n(seed, t, n, 4, max_draws)
    return out if len(out) == 4 else None


def undistort(xd, yd, kc):
    """Normalised distorted coordinates -> undistorted (20 fixed-point steps); works on floats and arrays."""
    xn, yn = xd, yd
    for _ in range(20):
        f = 1.0 + kc * (xn * xn + yn * yn)
        xn, yn = xd / f, yd / f
    return xn, yn


def distort(xn, yn, kc):
    f = 1.0 + kc * (xn * xn + yn * yn)
    return xn * f, yn * f


def _triple(a, b, c):
    c0 = a[1] * b[2] - a[2] * b[1]
    c1 = a[2] * b[0] - a[0] * b[2]
    c2 = a[0] * b[1] - a[1] * b[0]
    return c0 * c[0] + c1 * c[1] + c2 * c[2]


_TRIPLES = ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))  # nchoosek(1:4, 3)


def is_degenerate(P, x2):
    """degenfn_P: P the four 3-D points, x2 the four homogeneous (undistorted) 2-D points."""
    return (any(abs(_triple(P[a], P[b], P[c])) < _EPS for a, b, c in _TRIPLES)
            or any(abs(_triple(x2[a], x2[b], x2[c])) < _EPS for a, b, c in _TRIPLES))


def _root2real(b, c):
    v = b * b - 4.0 * c
    if v < 0.0:
        return None
    y = math.sqrt(v)
    q = 0.5 * (-b + y) if b < 0.0 else 0.5 * (-b - y)
    return q, (c / q if q != 0.0 else 0.0)


def _cubick(b, c, d):
    if b * b >= 3.0 * c:
        v = math.sqrt(b * b - 3.0 * c)
        t1 = (-b - v) / 3.0
        k = ((t1 + b) * t1 + c) * t1 + d
        if k > 0.0:
            r0 = t1 - _sqrt(_div(-k, 3.0 * t1 + b))
        else:
            t2 = (-b + v) / 3.0
            k = ((t2 + b) * t2 + c) * t2 + d
            r0 = t2 + _sqrt(_div(-k, 3.0 * t2 + b))
    else:
        r0 = -b / 3.0
        if abs((3.0 * r0 + 2.0 * b) * r0 + c) < 1e-4:
            r0 += 1.0
    for it in range(50):
        fx = ((r0 + b) * r0 + c) * r0 + d
        if it >= 7 and abs(fx) <= 1e-13:
            break
        fpx = (3.0 * r0 + 2.0 * b) * r0 + c
        r0 -= _div(fx, fpx)
    return r0


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else math.nan


def _cof3(A):
    return [A[4] * A[8] - A[5] * A[7], A[5] * A[6] - A[3] * A[8], A[3] * A[7] - A[4] * A[6],
            A[2] * A[7] - A[1] * A[8], A[0] * A[8] - A[2] * A[6], A[1] * A[6] - A[0] * A[7],
            A[1] * A[5] - A[2] * A[4], A[2] * A[3] - A[0] * A[5], A[0] * A[4] - A[1] * A[3]]


def _eigvec(A, lam):
    r = [[A[0] - lam, A[1], A[2]], [A[3], A[4] - lam, A[5]], [A[6], A[7], A[8] - lam]]
    best, v = -1.0, [0.0, 0.0, 0.0]
    for a, b in ((r[0], r[1]), (r[0], r[2]), (r[1], r[2])):
        c = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
        n = c[0] * c[0] + c[1] * c[1] + c[2] * c[2]
        if n > best:
            best, v = n, c
    s = _div(1.0, _sqrt(best))
    return [v[0] * s, v[1] * s, v[2] * s]


def _refine(L, a12, a13, a23, b12, b13, b23):
    for _ in range(5):
        l1, l2, l3 = L
        r1 = l1 * l1 + l2 * l2 + b12 * l1 * l2 - a12
        r2 = l1 * l1 + l3 * l3 + b13 * l1 * l3 - a13
        r3 = l2 * l2 + l3 * l3 + b23 * l2 * l3 - a23
        e0 = abs(r1) + abs(r2) + abs(r3)
        if e0 < 1e-10:
            break
        v0, v1 = 2.0 * l1 + b12 * l2, 2.0 * l2 + b12 * l1
        v3, v5 = 2.0 * l1 + b13 * l3, 2.0 * l3 + b13 * l1
        v7, v8 = 2.0 * l2 + b23 * l3, 2.0 * l3 + b23 * l2
        det = _div(1.0, -v0 * v5 * v7 - v1 * v3 * v8)
        n1 = l1 - det * (-v5 * v7 * r1 - v1 * v8 * r2 + v1 * v5 * r3)
        n2 = l2 - det * (-v3 * v8 * r1 + v0 * v8 * r2 - v0 * v5 * r3)
        n3 = l3 - det * (v3 * v7 * r1 - v0 * v7 * r2 - v1 * v3 * r3)
        s1 = n1 * n1 + n2 * n2 + b12 * n1 * n2 - a12
        s2 = n1 * n1 + n3 * n3 + b13 * n1 * n3 - a13
        s3 = n2 * n2 + n3 * n3 + b23 * n2 * n3 - a23
        if abs(s1) + abs(s2) + abs(s3) > e0:
            break
        L = [n1, n2, n3]
    return L


def p3p(y, x):
    """Lambda Twist P3P (Persson and Nordberg 2018): unit bearings y[3][3], world points x[3][3] -> list of (R 3x3
    row-major list of 9, T 3), y ~ R x + T, in the device's order (+v before -v, the larger-magnitude tau first)."""
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]  # noqa: E731
    b12, b13, b23 = -2.0 * dot(y[0], y[1]), -2.0 * dot(y[0], y[2]), -2.0 * dot(y[1], y[2])
    d12 = [x[0][k] - x[1][k] for k in range(3)]
    d13 = [x[0][k] - x[2][k] for k in range(3)]
    d23 = [x[1][k] - x[2][k] for k in range(3)]
    a12, a13, a23 = dot(d12, d12), dot(d13, d13), dot(d23, d23)
    D1 = [a23, 0.5 * a23 * b12, 0.0, 0.5 * a23 * b12, a23 - a12, -0.5 * a12 * b23, 0.0, -0.5 * a12 * b23, -a12]
    D2 = [a23, 0.0, 0.5 * a23 * b13, 0.0, -a13, -0.5 * a13 * b23, 0.5 * a23 * b13, -0.5 * a13 * b23, a23 - a13]
    C1, C2 = _cof3(D1), _cof3(D2)
    c0 = c1 = c2 = c3 = 0.0
    for k in range(3):
        c0 += D1[k] * C1[k]
        c3 += D2[k] * C2[k]
    for k in range(9):
        c1 += C1[k] * D2[k]
        c2 += D1[k] * C2[k]
    c3, c1 = -c3, -c1
    if not (abs(c3) > 0.0) or not math.isfinite(c3):
        return []
    g = _cubick(c2 / c3, c1 / c3, c0 / c3)
    A = [D1[k] - g * D2[k] for k in range(9)]
    tr = A[0] + A[4] + A[8]
    m = (A[0] * A[4] - A[1] * A[3]) + (A[0] * A[8] - A[2] * A[6]) + (A[4] * A[8] - A[5] * A[7])
    r = _root2real(-tr, m)
    if r is None:
        return []
    e1, e2 = r
    if abs(e1) < abs(e2):
        e1, e2 = e2, e1
    if not (abs(e1) > 0.0):
        return []
    V0, V1 = _eigvec(A, e1), _eigvec(A, e2)
    v = _sqrt(max(0.0, _div(-e2, e1)))
    xc3 = [d12[1] * d13[2] - d12[2] * d13[1], d12[2] * d13[0] - d12[0] * d13[2], d12[0] * d13[1] - d12[1] * d13[0]]
    X = [d12[0], d13[0], xc3[0], d12[1], d13[1], xc3[1], d12[2], d13[2], xc3[2]]
    CX = _cof3(X)
    detX = X[0] * CX[0] + X[1] * CX[1] + X[2] * CX[2]
    if not (abs(detX) > 0.0):
        return []
    idet = 1.0 / detX
    Xi = [CX[c * 3 + rr] * idet for rr in range(3) for c in range(3)]
    out = []
    for s in (v, -v):
        w2 = _div(1.0, s * V1[0] - V0[0])
        w0 = (V0[1] - s * V1[1]) * w2
        w1 = (V0[2] - s * V1[2]) * w2
        ia = _div(1.0, (a13 - a12) * w1 * w1 - a12 * b13 * w1 - a12)
        qb = (a13 * b12 * w1 - a12 * b13 * w0 - 2.0 * w0 * w1 * (a12 - a13)) * ia
        qc = ((a13 - a12) * w0 * w0 + a13 * b12 * w0 + a13) * ia
        taus = _root2real(qb, qc) if math.isfinite(qb) and math.isfinite(qc) else None
        if taus is None:
            continue
        for tau in taus:
            if not (tau > 0.0):
                continue
            d = _div(a23, tau * (b23 + tau) + 1.0)
            if not (d > 0.0):
                continue
            l2 = math.sqrt(d)
            l3 = tau * l2
            L = _refine([w0 * l2 + w1 * l3, l2, l3], a12, a13, a23, b12, b13, b23) if w0 * l2 + w1 * l3 >= 0.0 else None
            if L is None:
                continue
            ry = [[y[i][k] * L[i] for k in range(3)] for i in range(3)]
            yd1 = [ry[0][k] - ry[1][k] for k in range(3)]
            yd2 = [ry[0][k] - ry[2][k] for k in range(3)]
            yc = [yd1[1] * yd2[2] - yd1[2] * yd2[1], yd1[2] * yd2[0] - yd1[0] * yd2[2], yd1[0] * yd2[1] - yd1[1] * yd2[0]]
            Y = [yd1[0], yd2[0], yc[0], yd1[1], yd2[1], yc[1], yd1[2], yd2[2], yc[2]]
            R = [Y[rr * 3 + 0] * Xi[0 * 3 + c] + Y[rr * 3 + 1] * Xi[1 * 3 + c] + Y[rr * 3 + 2] * Xi[2 * 3 + c]
                 for rr in range(3) for c in range(3)]
            T = [ry[0][rr] - (R[rr * 3 + 0] * x[0][0] + R[rr * 3 + 1] * x[0][1] + R[rr * 3 + 2] * x[0][2])
                 for rr in range(3)]
            out.append((R, T))
    return out


def _hypothesis(seed, t, u, v, P3, fx, fy, cx, cy, kc, detail=False):
    """One trial. Returns (draws, R, t) or (draws, None, None); with detail also the 4th-match errors of every root."""
    idx = draw_indices(seed, t, len(u))
    if idx is None:
        return (None, None, None, []) if detail else (None, None, None)
    P = [[float(P3[0][i]), float(P3[1][i]), float(P3[2][i])] for i in idx]
    x2 = []
    for i in idx:
        xd, yd = (float(u[i]) - cx) / fx, (float(v[i]) - cy) / fy
        xn, yn = undistort(xd, yd, kc)
        x2.append([xn * fx + cx, yn * fy + cy, 1.0])
    fail = (idx, None, None, []) if detail else (idx, None, None)
    if is_degenerate(P, x2):
        return fail
    yb = []
    for q in range(3):
        bx, by = (x2[q][0] - cx) / fx, (x2[q][1] - cy) / fy
        s = 1.0 / math.sqrt(bx * bx + by * by + 1.0)
        yb.append([bx * s, by * s, s])
    best, pick, errs = math.inf, None, []
    for R, T in p3p(yb, P):
        t3 = [-(R[0 * 3 + c] * T[0] + R[1 * 3 + c] * T[1] + R[2 * 3 + c] * T[2]) for c in range(3)]
        dX, dY, dZ = P[3][0] - t3[0], P[3][1] - t3[1], P[3][2] - t3[2]
        xc = R[0] * dX + R[1] * dY + R[2] * dZ
        yc = R[3] * dX + R[4] * dY + R[5] * dZ
        zc = R[6] * dX + R[7] * dY + R[8] * dZ
        iz = _div(1.0, zc)
        du = fx * (xc * iz) + cx - x2[3][0]
        dv = fy * (yc * iz) + cy - x2[3][1]
        e = du * du + dv * dv
        errs.append(e)
        if e < best:
            best, pick = e, (np.array(R).reshape(3, 3), np.array(t3))
    if pick is None:
        return fail
    return (idx, pick[0], pick[1], errs) if detail else (idx, pick[0], pick[1])


def _residuals(R, t, u, v, P3, fx, fy, cx, cy, kc):
    """Reprojection distance of every match (f64, the device's order of operations)."""
    dX, dY, dZ = P3[0] - t[0], P3[1] - t[1], P3[2] - t[2]
    xc = R[0, 0] * dX + R[0, 1] * dY + R[0, 2] * dZ
    yc = R[1, 0] * dX + R[1, 1] * dY + R[1, 2] * dZ
    zc = R[2, 0] * dX + R[2, 1] * dY + R[2, 2] * dZ
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iz = 1.0 / zc
        xn, yn = xc * iz, yc * iz
        f = 1.0 + kc * (xn * xn + yn * yn)
        du = fx * (xn * f) + cx - u
        dv = fy * (yn * f) + cy - v
        return np.sqrt(du * du + dv * dv)


def _log_pose(R, t):
    G = np.zeros(12)
    for i in range(3):
        G[i * 4:i * 4 + 3] = R[i]
        G[i * 4 + 3] = -R[i, 0] * t[0] - R[i, 1] * t[1] - R[i, 2] * t[2]
    p = np.zeros(6)
    _lib.load().ictr_se3_group_to_coeff_d(dp(p), dp(G))
    return p


def _post_filter(inl_sets, n):
    S = len(inl_sets)
    cnt = np.zeros(n, np.int64)
    for s in inl_sets:
        cnt[s] += 1
    keep = [s for s in range(S) if not (s < n and cnt[s] <= 4)]
    return keep, cnt[cnt > 4]


def _as_pts(pt2d, pt3d):
    """(2, N) / (N, 2) pixels and (3, N) / (N, 3) points (homogeneous rows / columns beyond are ignored) -> SoA f64."""
    a, b = np.asarray(pt2d, np.float64), np.asarray(pt3d, np.float64)
    if a.ndim != 2 or b.ndim != 2:
        raise ValueError("pt2d and pt3d must be 2-D arrays")
    if a.shape[0] in (2, 3) and b.shape[0] in (3, 4) and a.shape[1] == b.shape[1]:
        return f64c(a[:2]), f64c(b[:3])
    if a.shape[1] in (2, 3) and b.shape[1] in (3, 4) and a.shape[0] == b.shape[0]:
        return f64c(a[:, :2].T), f64c(b[:, :3].T)
    raise ValueError(f"pt2d {a.shape} and pt3d {b.shape} are not (2, N) / (3, N) or (N, 2) / (N, 3) of one N")


def _fc_cc(fc, cc):
    fc = np.asarray(fc, np.float64).reshape(-1)
    fc = np.array([fc[0], fc[0]]) if fc.size == 1 else fc[:2]  # :13-15
    return f64c(fc), f64c(np.asarray(cc, np.float64).reshape(-1)[:2])


def _result(R, t, p, inl, inl_cnt, trials, draws, accepted, trials_used):
    return dict(R=np.asarray(R, np.float64).reshape(-1, 3, 3), t=np.asarray(t, np.float64).reshape(-1, 3),
                p=np.asarray(p, np.float64).reshape(-1, 6), inl=inl, inl_cnt=np.asarray(inl_cnt, np.int64),
                trials=np.asarray(trials, np.int64), draws=np.asarray(draws, np.int64).reshape(-1, 4),
                accepted=int(accepted), trials_used=int(trials_used))


def sample_poses_host(pt2d, pt3d, fc, cc, nsamples, maxtrials, inlthresh, kc=0.0, seed=0, detail=False):
    """The hypothesis stage restated in NumPy / Python f64 (the checker of sample_poses). Same result dict. detail:
    also ``margins`` -- per accepted sample the smallest |residual - inlthresh| over the matches and the two smallest
    4th-match errors of its P3P roots (for tests that need clear decisions)."""
    xy, P3 = _as_pts(pt2d, pt3d)
    fc, cc = _fc_cc(fc, cc)
    fx, fy, cx, cy = float(fc[0]), float(fc[1]), float(cc[0]), float(cc[1])
    u, v = xy[0], xy[1]
    n = u.size
    if n < 4:
        raise ValueError("at least 4 matches are needed")
    thr = float(inlthresh)
    Rs, ts, inl, trials, draws, margins = [], [], [], [], [], []
    used = int(maxtrials)
    for t in range(int(maxtrials)):
        idx, R, tc, *errs = _hypothesis(seed, t, u, v, P3, fx, fy, cx, cy, float(kc), detail)
        if R is None:
            continue
        res = _residuals(R, tc, u, v, P3, fx, fy, cx, cy, float(kc))
        ids = np.nonzero(res <= thr)[0]
        if ids.size < 4:
            continue
        Rs.append(R)
        ts.append(tc)
        inl.append(ids)
        trials.append(t)
        draws.append(idx)
        if detail:
            e = sorted(errs[0])
            with np.errstate(invalid="ignore"):
                margins.append((float(np.nanmin(np.abs(res - thr))), e[0], e[1] if len(e) > 1 else math.inf))
        if len(Rs) == int(nsamples):
            used = t + 1
            break
    keep, cnt = _post_filter(inl, n)
    out = _result([Rs[s] for s in keep], [ts[s] for s in keep], [_log_pose(Rs[s], ts[s]) for s in keep],
                  [inl[s] for s in keep], cnt, [trials[s] for s in keep], [draws[s] for s in keep], len(Rs), used)
    if detail:
        out["margins"] = [margins[s] for s in keep]
        out["accepted_trials"] = np.asarray(trials, np.int64)
    return out


class RansacSampler:
    """The device path: one ictr_ransac object for N matches and up to max_samples samples."""

    def __init__(self, n, max_samples):
        self._h = C.c_void_p()
        check(_lib.load().ictr_ransac_create(C.byref(self._h), int(n), int(max_samples)))
        self.n, self.max_samples = int(n), int(max_samples)
        self.nwords = (self.n + 63) // 64

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.load().ictr_ransac_destroy(self._h)
            self._h = None

    @property
    def chunk(self):
        return _lib.load().ictr_ransac_chunk_size(self._h)

    def set_points(self, pt2d, pt3d):
        xy, P3 = _as_pts(pt2d, pt3d)
        if xy.shape[1] != self.n:
            raise ValueError(f"{xy.shape[1]} matches, the sampler was made for {self.n}")
        check(_lib.load().ictr_ransac_set_points(self._h, dp(xy), dp(P3)))

    def run_async(self, fc, cc, nsamples, maxtrials, inlthresh, kc=0.0, seed=0, stream=None):
        fc, cc = _fc_cc(fc, cc)
        sp = getattr(stream, "cuda_stream", stream)
        check(_lib.load().ictr_ransac_run(self._h, dp(fc), dp(cc), float(kc), int(nsamples), int(maxtrials),
                                          float(inlthresh), int(seed) & _M64, C.c_void_p(sp or 0)))

    def debug_trials(self, fc, cc, inlthresh, kc=0.0, seed=0, first_trial=0, count=1):
        """Inspection (ictr_debug_ransac_trials): the hypothesis and score kernels alone over trials first_trial ..
        first_trial + count - 1, no selection. dict: status (count,), draws (count, 4), hyp (count, 12) = R row-major
        then the camera centre, cnt (count,), words (count, nwords); hyp, cnt and words of a status-0 trial are
        undefined."""
        fc, cc = _fc_cc(fc, cc)
        n = int(count)
        status, draws = np.zeros(n, np.int32), np.zeros((n, 4), np.int32)
        hyp, cnt, words = np.zeros((n, 12)), np.zeros(n, np.uint32), np.zeros((n, self.nwords), np.uint64)
        i32 = C.POINTER(C.c_int32)
        check(_lib.load().ictr_debug_ransac_trials(
            self._h, dp(fc), dp(cc), float(kc), float(inlthresh), int(seed) & _M64, int(first_trial), n,
            status.ctypes.data_as(i32), draws.ctypes.data_as(i32), dp(hyp), cnt.ctypes.data_as(C.POINTER(C.c_uint32)),
            words.ctypes.data_as(C.POINTER(C.c_uint64))))
        return dict(status=status, draws=draws, hyp=hyp, cnt=cnt, words=words)

    def wait(self):
        L = _lib.load()
        S, W = self.max_samples, self.nwords
        counts = np.zeros(4, np.int64)
        R, t, p = np.zeros((S, 9)), np.zeros((S, 3)), np.zeros((S, 6))
        words = np.zeros((S, W), np.uint64)
        cnt = np.zeros(self.n, np.int32)
        i64, u64, i32 = C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
        check(L.ictr_ransac_wait(self._h, counts.ctypes.data_as(i64), dp(R), dp(t), dp(p), words.ctypes.data_as(u64),
                                 cnt.ctypes.data_as(i32)))
        k = int(counts[0])
        trials = np.zeros(max(k, 1), np.int64)
        draws = np.zeros((max(k, 1), 4), np.int32)
        check(L.ictr_ransac_samples(self._h, trials.ctypes.data_as(i64), draws.ctypes.data_as(i32)))
        bits = np.unpackbits(words[:k].view(np.uint8).reshape(k, W, 8), axis=2, bitorder="little").reshape(k, W * 64)
        inl = [np.nonzero(bits[s, :self.n])[0] for s in range(k)]
        out = _result(R[:k], t[:k], p[:k], inl, cnt[:int(counts[3])], trials[:k], draws[:k], counts[1], counts[2])
        out["words"] = words[:k].copy()
        return out


def sample_poses(pt2d, pt3d, fc, cc, nsamples, maxtrials, inlthresh, kc=0.0, seed=0, stream=None):
    """The hypothesis stage on the device. Returns dict: R (S, 3, 3), t (S, 3) camera centres, p (S, 6) =
    se3_log([R | -R t]), inl (list of 0-based inlier index arrays), inl_cnt (filtered), trials / draws (trial index
    and drawn matches of each sample), accepted (samples before the post-filter), trials_used."""
    xy, P3 = _as_pts(pt2d, pt3d)
    s = RansacSampler(xy.shape[1], int(nsamples))
    s.set_points(xy, P3)
    s.run_async(fc, cc, nsamples, maxtrials, inlthresh, kc, seed, stream)
    return s.wait()


def best_sample(corr):
    """The sample with the largest mean correlation (:152-153): per sample the mean of its correlations with NaN
    entries ignored (a point that leaves the view scores NaN; all NaN or none -> NaN), then MATLAB's max: NaN means
    ignored, the first on ties; all NaN -> 0; no sample -> None. Returns (index, means)."""
    means = np.full(len(corr), np.nan)
    for i, c in enumerate(corr):
        c = np.asarray(c, np.float64)
        c = c[~np.isnan(c)]
        if c.size:
            means[i] = c.mean()
    if means.size == 0:
        return None, means
    if np.all(np.isnan(means)):
        return 0, means
    return int(np.nanargmax(means)), means


def _op_dict(op, n):
    if isinstance(op, dict):
        d = dict(op)
    else:
        d = dict(lv_f=op.lv_f, lv_l=op.lv_l, psz=op.psz, maxiter=op.maxiter, normdp_ratio=float(op.normdp_ratio),
                 donorm=int(bool(op.donorm)), dopatchnorm=int(bool(op.dopatchnorm)), maxpttrack=op.maxpttrack,
                 verbosity=op.verbosity)
    d["maxpttrack"] = int(n)  # run_ransac_test.m:105: pa.maxpt = nomatches
    return d


def fit_cameras_odom(pt2d, pt3d, cam, nsamples, maxtrials, inlthresh, op, fbframes, frames, kc=0.0, seed=0,
                     write_input=None):
    """func_ransac_fitcameras_odom.m: pose samples on the device, then the odometry check of every sample through
    run_track_nposes.run in process.

    cam: dict with fc, cc, wh (or an object with those attributes). op: optparam or the nposes op dict (maxpttrack is
    set to N, as run_ransac_test.m:105 does). fbframes: (frames back, frames forward). frames: grey images or file
    names, nback + nfwd + 1 of them, the reference frame at index nback. write_input: a path -> the odometrycheck.txt
    the reference writes (images given as arrays are saved next to it as .npy and named in it).

    Returns dict: best (sample index or None); p_best (F, 6), R_best (F, 3, 3), c_best (F, 3): per frame the tracked
    pose of the best sample, its rotation and camera centre -Rᵀ T (the script's t_best is the coefficient list,
    :164: here p_best); inl_best (1-based); samples (sample_poses' dict); res_pose (S, F, 6), res_corr (list),
    res_corravg (S,); the nposes input dict as ``input``."""
    xy, P3 = _as_pts(pt2d, pt3d)
    n = xy.shape[1]
    fc = cam["fc"] if isinstance(cam, dict) else cam.fc
    cc = cam["cc"] if isinstance(cam, dict) else cam.cc
    wh = cam["wh"] if isinstance(cam, dict) else cam.wh
    nback, nfwd = (int(x) for x in fbframes)
    frames = list(frames)
    if len(frames) != nback + nfwd + 1:
        raise ValueError(f"{len(frames)} frames given, fbframes {fbframes} needs {nback + nfwd + 1}")
    smp = sample_poses(xy, P3, fc, cc, nsamples, maxtrials, inlthresh, kc, seed)
    images = None if all(isinstance(f, str) for f in frames) else [
        np.asarray(f, np.float32) if not isinstance(f, str) else None for f in frames]
    names = [f if isinstance(f, str) else "frame%02d.npy" % i for i, f in enumerate(frames)]
    if images is not None:
        from .io_formats import read_image_gray
        images = [im if im is not None else read_image_gray(frames[i]) for i, im in enumerate(images)]
    inp = dict(op=_op_dict(op, n), fc=np.asarray(fc, np.float32).reshape(-1)[:2],
               cc=np.asarray(cc, np.float32).reshape(-1)[:2], wh=np.asarray(wh, np.int32).reshape(-1)[:2],
               fbframes=(nback, nfwd), filenames=names, pt2d=xy.T.copy(), pt3d=P3.T.copy(), poses=smp["p"],
               inlids=[np.sort(i) + 1 for i in smp["inl"]])
    if write_input is not None:
        from .io_formats import write_nposes_input
        if images is not None:
            base = os.path.splitext(str(write_input))[0]
            for i, f in enumerate(frames):
                if not isinstance(f, str):
                    names[i] = "%s_frame%02d.npy" % (base, i)
                    np.save(names[i], images[i])
            inp["filenames"] = names
        write_nposes_input(write_input, inp["op"], inp["fc"], inp["cc"], inp["wh"], inp["fbframes"], names,
                           inp["pt2d"], inp["pt3d"], inp["poses"], inp["inlids"])
    S = len(smp["p"])
    out = dict(samples=smp, input=inp, res_pose=np.zeros((0, len(frames), 6)), res_corr=[],
               res_corravg=np.zeros(0), best=None, p_best=None, R_best=None, c_best=None, inl_best=None)
    if S == 0:
        return out
    from . import run_track_nposes
    res_corr, res_pose = run_track_nposes.run(inp, images)
    best, means = best_sample(res_corr)
    P = np.asarray(res_pose[best], np.float64)
    Gs = [_se3_exp_d(p) for p in P]
    out.update(res_corr=res_corr, res_pose=np.asarray(res_pose, np.float64), res_corravg=means, best=best, p_best=P,
               R_best=np.array([G[:, :3] for G in Gs]), c_best=np.array([-G[:, :3].T @ G[:, 3] for G in Gs]),
               inl_best=inp["inlids"][best])
    return out
