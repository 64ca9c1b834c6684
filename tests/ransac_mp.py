"""An independent judge of one RANSAC trial at 60 digits (mpmath), sharing no formula with Lambda Twist.

P3P by the classical quartic. Unit bearings y_i, world points x_i, depths s_i > 0, c_ij = y_i . y_j, a_ij = |x_i - x_j|^2:

    s_i^2 + s_j^2 - 2 c_ij s_i s_j = a_ij            (the law of cosines, three times)

With u = s2 / s1 and v = s3 / s1, eliminating s1^2 between the pairs (12, 13) and (23, 13) leaves two quadratics in u
whose coefficients are polynomials in v:

    E1: a13 u^2 - 2 a13 c12   u + (a13     - a12 (1 + v^2 - 2 c13 v)) = 0
    E2: a13 u^2 - 2 a13 c23 v u + (a13 v^2 - a23 (1 + v^2 - 2 c13 v)) = 0

Their resultant in u is a quartic in v (mpmath.polyroots). For every real root v > 0: u from E1 - E2 (linear in u; where
that degenerates, from E1 with E2 as the test), then s1 from the 13 equation. R and T map the world triangle onto the
camera triangle s_i y_i: each triangle gets the orthonormal frame (e1 = along 1->2, e3 = its normal, e2 = e3 x e1),
R = F_cam F_world^T, T = s1 y1 - R x1. Kept: real roots with u, v > 0.

On top of the solver, everything a trial decides, in mpmath from the f64 inputs: degenfn_P, the 20-step undistortion, the
choice of root by the fourth match, the reprojection residuals and the inlier set.
"""
import mpmath as mp

DPS = 60
mp.mp.dps = DPS
_EPS = mp.mpf(2) ** -52
_REAL = mp.mpf(10) ** -25   # |imag| below this (relative): a real root; double roots come out at about 10^-30
_SAME = mp.mpf(10) ** -20   # two solutions nearer than this are one (a double root found twice)


def _f(x):
    return mp.mpf(float(x))


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _pmul(p, q):  # polynomials as ascending coefficient lists
    out = [mp.mpf(0)] * (len(p) + len(q) - 1)
    for i, a in enumerate(p):
        for j, b in enumerate(q):
            out[i + j] += a * b
    return out


def _padd(p, q, s=1):
    n = max(len(p), len(q))
    return [(p[i] if i < len(p) else 0) + s * (q[i] if i < len(q) else 0) for i in range(n)]


def _peval(p, x):
    r = mp.mpf(0)
    for c in reversed(p):
        r = r * x + c
    return r


def _frame(p1, p2, p3):
    """Columns e1, e2, e3 of the triangle's orthonormal frame, or None for a degenerate triangle."""
    d1, n = _sub(p2, p1), _cross(_sub(p2, p1), _sub(p3, p1))
    l1, ln = mp.sqrt(_dot(d1, d1)), mp.sqrt(_dot(n, n))
    if l1 == 0 or ln == 0:
        return None
    e1, e3 = [c / l1 for c in d1], [c / ln for c in n]
    return e1, _cross(e3, e1), e3


def p3p(y, x):
    """All (R 3x3 nested list, T 3) with s_i y_i = R x_i + T, s_i > 0, for unit bearings y[3] and world points x[3]
    (mpf). Degenerate world triangles (coincident or collinear points) have no isolated solution: []."""
    c12, c13, c23 = _dot(y[0], y[1]), _dot(y[0], y[2]), _dot(y[1], y[2])
    a12 = _dot(_sub(x[0], x[1]), _sub(x[0], x[1]))
    a13 = _dot(_sub(x[0], x[2]), _sub(x[0], x[2]))
    a23 = _dot(_sub(x[1], x[2]), _sub(x[1], x[2]))
    Fw = _frame(x[0], x[1], x[2])
    if Fw is None or a12 == 0 or a13 == 0 or a23 == 0:
        return []
    g = [mp.mpf(1), -2 * c13, mp.mpf(1)]                  # 1 - 2 c13 v + v^2
    A = a13
    B1, B2 = [-2 * a13 * c12], [mp.mpf(0), -2 * a13 * c23]
    C1 = _padd([a13], [a12 * c for c in g], -1)
    C2 = _padd([mp.mpf(0), mp.mpf(0), a13], [a23 * c for c in g], -1)
    dC, dB = _padd(C2, C1, -1), _padd(B2, B1, -1)
    res = _padd([A * c for c in _pmul(dC, dC)], _pmul(dB, _padd(_pmul(B1, C2), _pmul(C1, B2), -1)), -1)
    res = (res + [mp.mpf(0)] * 5)[:5]
    while len(res) > 1 and res[-1] == 0:
        res.pop()
    if len(res) < 2:
        return []
    scale = max(abs(c) for c in res)
    roots = mp.polyroots([c / scale for c in reversed(res)], maxsteps=2000, extraprec=4 * mp.mp.prec)
    out = []
    for v in roots:
        if abs(mp.im(v)) > _REAL * (1 + abs(v)):
            continue
        v = mp.re(v)
        if not v > 0:
            continue
        b1, b2 = _peval(B1, v), _peval(B2, v)
        k1, k2 = _peval(C1, v), _peval(C2, v)
        if abs(b1 - b2) > _REAL * (abs(b1) + abs(b2)):
            us = [(k2 - k1) / (b1 - b2)]
        else:  # E1 - E2 does not give u: both roots of E1, E2 decides
            disc = b1 * b1 - 4 * A * k1
            if disc < 0:
                continue
            us = [(-b1 + sg * mp.sqrt(disc)) / (2 * A) for sg in (1, -1)]
            us = [u for u in us if abs(A * u * u + b2 * u + k2) <= _REAL * (abs(A) * u * u + abs(b2 * u) + abs(k2))]
        for u in us:
            if not u > 0:
                continue
            den = 1 - 2 * c13 * v + v * v
            if not den > 0:
                continue
            s1 = mp.sqrt(a13 / den)
            s = [s1, u * s1, v * s1]
            pc = [[y[i][k] * s[i] for k in range(3)] for i in range(3)]
            Fc = _frame(pc[0], pc[1], pc[2])
            if Fc is None:
                continue
            R = [[sum(Fc[m][r] * Fw[m][c] for m in range(3)) for c in range(3)] for r in range(3)]
            T = [pc[0][r] - _dot(R[r], x[0]) for r in range(3)]
            if any(max(max(abs(R[r][c] - R2[r][c]) for r in range(3) for c in range(3)),
                       max(abs(T[r] - T2[r]) for r in range(3))) < _SAME for R2, T2 in out):
                continue
            out.append((R, T))
    return out


def undistort(xd, yd, kc):
    xn, yn = xd, yd
    for _ in range(20):
        f = 1 + kc * (xn * xn + yn * yn)
        xn, yn = xd / f, yd / f
    return xn, yn


def is_degenerate(P, x2):
    tr = ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))
    return (any(abs(_dot(_cross(P[a], P[b]), P[c])) < _EPS for a, b, c in tr)
            or any(abs(_dot(_cross(x2[a], x2[b]), x2[c])) < _EPS for a, b, c in tr))


def bearings_and_points(idx, u, v, P3, fx, fy, cx, cy, kc):
    """The solver's inputs of a trial: P [4][3], the undistorted homogeneous pixels x2 [4][3], unit bearings yb [3][3]."""
    fx, fy, cx, cy, kc = _f(fx), _f(fy), _f(cx), _f(cy), _f(kc)
    P = [[_f(P3[0][i]), _f(P3[1][i]), _f(P3[2][i])] for i in idx]
    x2 = []
    for i in idx:
        xn, yn = undistort((_f(u[i]) - cx) / fx, (_f(v[i]) - cy) / fy, kc)
        x2.append([xn * fx + cx, yn * fy + cy, mp.mpf(1)])
    yb = []
    for q in range(3):
        bx, by = (x2[q][0] - cx) / fx, (x2[q][1] - cy) / fy
        s = 1 / mp.sqrt(bx * bx + by * by + 1)
        yb.append([bx * s, by * s, s])
    return P, x2, yb


def residuals(R, t, u, v, P3, fx, fy, cx, cy, kc):
    """Reprojection distance of every match under x_cam = R (X - t); +inf where the point lies in the camera plane."""
    fx, fy, cx, cy, kc = _f(fx), _f(fy), _f(cx), _f(cy), _f(kc)
    out = []
    for i in range(len(u)):
        d = [_f(P3[0][i]) - t[0], _f(P3[1][i]) - t[1], _f(P3[2][i]) - t[2]]
        xc, yc, zc = _dot(R[0], d), _dot(R[1], d), _dot(R[2], d)
        if zc == 0:
            out.append(mp.inf)
            continue
        xn, yn = xc / zc, yc / zc
        f = 1 + kc * (xn * xn + yn * yn)
        du, dv = fx * (xn * f) + cx - _f(u[i]), fy * (yn * f) + cy - _f(v[i])
        out.append(mp.sqrt(du * du + dv * dv))
    return out


def trial(idx, u, v, P3, fx, fy, cx, cy, kc):
    """One trial on the drawn indices idx. dict: degenerate, sols [(R, T)], errs (squared 4th-match error per
    solution, +inf where the 4th point lies in the camera plane), pick (index or None), R, t (camera centre) of it."""
    P, x2, yb = bearings_and_points(idx, u, v, P3, fx, fy, cx, cy, kc)
    out = dict(degenerate=is_degenerate(P, x2), sols=[], errs=[], pick=None, R=None, t=None)
    if out["degenerate"]:
        return out
    fxm, fym, cxm, cym = _f(fx), _f(fy), _f(cx), _f(cy)
    out["sols"] = p3p(yb, P)
    cents = []
    for R, T in out["sols"]:
        t = [-(R[0][c] * T[0] + R[1][c] * T[1] + R[2][c] * T[2]) for c in range(3)]
        cents.append(t)
        d = _sub(P[3], t)
        xc, yc, zc = _dot(R[0], d), _dot(R[1], d), _dot(R[2], d)
        if zc == 0:
            out["errs"].append(mp.inf)
            continue
        du, dv = fxm * (xc / zc) + cxm - x2[3][0], fym * (yc / zc) + cym - x2[3][1]
        out["errs"].append(du * du + dv * dv)
    if out["errs"] and min(out["errs"]) < mp.inf:
        k = min(range(len(out["errs"])), key=lambda i: out["errs"][i])
        out.update(pick=k, R=out["sols"][k][0], t=cents[k])
    return out


def sol_err(Rh, Th, Rm, Tm):
    """max |dR|, max |dT| between a host solution (flat list of 9, list of 3) and an mpmath one."""
    eR = max(abs(_f(Rh[r * 3 + c]) - Rm[r][c]) for r in range(3) for c in range(3))
    eT = max(abs(_f(Th[r]) - Tm[r]) for r in range(3))
    return float(eR), float(eT)
