"""Multi-view triangulation restated in float32 NumPy (test infrastructure, like parity_util.py): the checker of
ictr_triang.hip on machines that have no reference binary.

Vectorised over points, serial over a point's views, every product and sum in f32, in the order and with the grouping
of the reference's misc_src/triang.c (the DLT normal equations, Gauss-Newton and Levenberg-Marquardt on the full 3-D
point, Gauss-Newton on the depth along a ray). tests/test_triang_cpu.py pins it to the reference binary's recorded
outputs (tests/golden/triang_golden.npz) bit for bit.

Tracks are a ragged list: point i owns the observations offsets[i] .. offsets[i+1]-1 of view[] (camera index), x[], y[].
A lane whose track is shorter than the longest one skips the missing views (its sums are left untouched).
"""
import numpy as np

F32 = np.float32
MODES = ("dlt", "gn", "lm", "depth")


class _Tracks:
    def __init__(self, P, offsets, view, x, y):
        self.P = np.ascontiguousarray(P, F32).reshape(-1, 12)
        self.off = np.asarray(offsets, np.int64)
        self.view = np.asarray(view, np.int64)
        self.x, self.y = np.asarray(x, F32), np.asarray(y, F32)
        self.len = self.off[1:] - self.off[:-1]
        self.n = self.len.size
        self.kmax = int(self.len.max()) if self.n else 0
        self.nv2 = (2 * self.len).astype(F32)  # the C's `2*noviews`, converted for the f32 division

    def at(self, k):
        """Slot k of every track: validity mask, the 12 camera entries (each [n]) and the observation."""
        m = self.len > k
        idx = np.where(m, self.off[:-1] + k, self.off[:-1])
        p = self.P[self.view[idx]]
        return m, [p[:, j] for j in range(12)], self.x[idx], self.y[idx]


def _acc(m, a, t):
    return np.where(m, a + t, a)


def _inv3(m0, m1, m2, m4, m5, m8):
    """Adjugate / determinant inverse of a symmetric 3x3, nine divisions."""
    i0 = m8 * m4 - m5 * m5
    i1 = m2 * m5 - m8 * m1
    i2 = m1 * m5 - m2 * m4
    i4 = m8 * m0 - m2 * m2
    i5 = m1 * m2 - m0 * m5
    i8 = m0 * m4 - m1 * m1
    det = (m0 * i0 + m1 * i1) + m2 * i2
    return [i0 / det, i1 / det, i2 / det, i1 / det, i4 / det, i5 / det, i2 / det, i5 / det, i8 / det]


def _project(p, X):
    u = ((p[0] * X[0] + p[1] * X[1]) + p[2] * X[2]) + p[3]
    v = ((p[4] * X[0] + p[5] * X[1]) + p[6] * X[2]) + p[7]
    w = ((p[8] * X[0] + p[9] * X[1]) + p[10] * X[2]) + p[11]
    return u, v, w


def _residual(p, xo, yo, X):
    u, v, w = _project(p, X)
    return xo - u / w, yo - v / w


def _res_msq(T, X):
    s = np.zeros(T.n, F32)
    for k in range(T.kmax):
        m, p, xo, yo = T.at(k)
        rx, ry = _residual(p, xo, yo, X)
        s = _acc(m, s, rx * rx + ry * ry)
    return s / T.nv2


def _jacobian(p, X):
    den = ((p[8] * X[0] + p[9] * X[1]) + p[10] * X[2]) + p[11]
    den = den * den
    c0n0 = (p[1] * X[1] + p[2] * X[2]) + p[3]
    c1n0 = (p[0] * X[0] + p[2] * X[2]) + p[3]
    c2n0 = (p[0] * X[0] + p[1] * X[1]) + p[3]
    c0n1 = (p[5] * X[1] + p[6] * X[2]) + p[7]
    c1n1 = (p[4] * X[0] + p[6] * X[2]) + p[7]
    c2n1 = (p[4] * X[0] + p[5] * X[1]) + p[7]
    c0n2 = (p[9] * X[1] + p[10] * X[2]) + p[11]
    c1n2 = (p[8] * X[0] + p[10] * X[2]) + p[11]
    c2n2 = (p[8] * X[0] + p[9] * X[1]) + p[11]
    jx = [(p[0] * c0n2 - p[8] * c0n0) / den, (p[1] * c1n2 - p[9] * c1n0) / den, (p[2] * c2n2 - p[10] * c2n0) / den]
    jy = [(p[4] * c0n2 - p[8] * c0n1) / den, (p[5] * c1n2 - p[9] * c1n1) / den, (p[6] * c2n2 - p[10] * c2n1) / den]
    return jx, jy


def _normal_sums(T, X, Xr, want_jtj=True):
    """J(X)^T J(X) (6 unique sums) and J(X)^T r(Xr): all x-rows in view order, then all y-rows."""
    z = lambda: np.zeros(T.n, F32)  # noqa: E731
    h = [z() for _ in range(6)]
    g = [z() for _ in range(3)]
    for row in (0, 1):
        for k in range(T.kmax):
            m, p, xo, yo = T.at(k)
            j = _jacobian(p, X)[row]
            r = _residual(p, xo, yo, Xr)[row]
            if want_jtj:
                h[0] = _acc(m, h[0], j[0] * j[0])
                h[1] = _acc(m, h[1], j[0] * j[1])
                h[2] = _acc(m, h[2], j[0] * j[2])
                h[3] = _acc(m, h[3], j[1] * j[1])
                h[4] = _acc(m, h[4], j[1] * j[2])
                h[5] = _acc(m, h[5], j[2] * j[2])
            for c in range(3):
                g[c] = _acc(m, g[c], j[c] * r)
    return h, g


def _step(inv, g):
    return [(inv[0] * g[0] + inv[1] * g[1]) + inv[2] * g[2],
            (inv[1] * g[0] + inv[4] * g[1]) + inv[5] * g[2],
            (inv[2] * g[0] + inv[5] * g[1]) + inv[8] * g[2]]


def _sel(m, a, b):
    return [np.where(m, x, y) for x, y in zip(a, b)]


def _dlt(T):
    z = lambda: np.zeros(T.n, F32)  # noqa: E731
    h = [z() for _ in range(6)]
    g = [z() for _ in range(3)]
    for row in (0, 1):
        for k in range(T.kmax):
            m, p, xo, yo = T.at(k)
            o, q = (xo, 0) if row == 0 else (yo, 4)
            a = [o * p[8] - p[q], o * p[9] - p[q + 1], o * p[10] - p[q + 2], o * p[11] - p[q + 3]]
            h[0] = _acc(m, h[0], a[0] * a[0])
            h[1] = _acc(m, h[1], a[0] * a[1])
            h[2] = _acc(m, h[2], a[0] * a[2])
            h[3] = _acc(m, h[3], a[1] * a[1])
            h[4] = _acc(m, h[4], a[1] * a[2])
            h[5] = _acc(m, h[5], a[2] * a[2])
            for c in range(3):
                g[c] = np.where(m, g[c] - a[c] * a[3], g[c])
    inv = _inv3(*h)
    pt = [(inv[3 * r] * g[0] + inv[3 * r + 1] * g[1]) + inv[3 * r + 2] * g[2] for r in range(3)]
    return pt, inv, np.zeros(T.n, np.int32)


def _gn(T, X, noiter, minres):
    cov = [np.zeros(T.n, F32) for _ in range(9)]
    res = np.full(T.n, np.inf, F32)
    iters = np.zeros(T.n, np.int32)
    alive = np.ones(T.n, bool)
    for _ in range(noiter):
        alive = alive & (res > minres)
        if not alive.any():
            break
        h, g = _normal_sums(T, X, X)
        inv = _inv3(*h)
        d = _step(inv, g)
        res = np.where(alive, _res_msq(T, X), res)
        X = _sel(alive, [X[c] + d[c] for c in range(3)], X)
        cov = _sel(alive, inv, cov)
        iters = iters + alive
    return X, cov, iters


def _lm(T, X, noiter, minres, damp_init, fct, maxdamp):
    cov = [np.zeros(T.n, F32) for _ in range(9)]
    res = np.full(T.n, np.inf, F32)
    damp = np.full(T.n, damp_init, F32)
    iters = np.zeros(T.n, np.int32)
    alive = np.ones(T.n, bool)
    res_old = _res_msq(T, X)
    Xr = X  # where the stored residual vector was evaluated
    for _ in range(noiter):
        alive = alive & (res > minres) & (damp < maxdamp)
        if not alive.any():
            break
        h, g = _normal_sums(T, X, Xr)

        def update(dmp, gg):
            inv = _inv3(h[0] + dmp * h[0], h[1], h[2], h[3] + dmp * h[3], h[4], h[5] + dmp * h[5])
            d = _step(inv, gg)
            return [X[c] + d[c] for c in range(3)], inv

        Xt, inv1 = update(damp, g)
        res_t = _res_msq(T, Xt)
        ok = res_t < (res_old - minres)
        # not accepted: stronger damping, and the second step multiplies the Jacobian taken at X with the residual
        # vector the trial has just overwritten (the residuals at Xt)
        damp2 = damp * fct
        _, g2 = _normal_sums(T, X, Xt, want_jtj=False)
        X2, inv2 = update(damp2, g2)
        res_2 = _res_msq(T, X2)
        Xn = _sel(ok, Xt, X2)
        X = _sel(alive, Xn, X)
        Xr = X
        cov = _sel(alive, _sel(ok, inv1, inv2), cov)
        damp = np.where(alive, np.where(ok, damp / fct, damp2), damp)
        res = np.where(alive, np.where(ok, res_t, res_2), res)
        res_old = np.where(alive, res, res_old)
        iters = iters + alive
    return X, cov, iters


def _depth(T, X, campos, ptdir, noiter, minres):
    c = [np.ascontiguousarray(campos[:, j], F32) for j in range(3)]
    d = [np.ascontiguousarray(ptdir[:, j], F32) for j in range(3)]
    j = [X[q] - c[q] for q in range(3)]
    depth = np.sqrt((j[0] * j[0] + j[1] * j[1]) + j[2] * j[2])
    X = [d[q] * depth + c[q] for q in range(3)]
    prep = []
    for k in range(T.kmax):
        m, p, xo, yo = T.at(k)
        den1 = ((p[8] * c[0] + p[9] * c[1]) + p[10] * c[2]) + p[11]
        den2 = (p[8] * d[0] + p[9] * d[1]) + p[10] * d[2]
        aa0 = (p[0] * d[0] + p[1] * d[1]) + p[2] * d[2]
        aa1 = (p[4] * d[0] + p[5] * d[1]) + p[6] * d[2]
        bb0 = ((p[0] * c[0] + p[1] * c[1]) + p[2] * c[2]) + p[3]
        bb1 = ((p[4] * c[0] + p[5] * c[1]) + p[6] * c[2]) + p[7]
        prep.append((aa0 * den1 - bb0 * den2, aa1 * den1 - bb1 * den2, den1, den2))
    cov = np.zeros(T.n, F32)
    res = np.full(T.n, np.inf, F32)
    iters = np.zeros(T.n, np.int32)
    alive = np.ones(T.n, bool)
    for _ in range(noiter):
        alive = alive & (res > minres)
        if not alive.any():
            break
        jtj = np.zeros(T.n, F32)
        dp = np.zeros(T.n, F32)
        rs = np.zeros(T.n, F32)
        for k in range(T.kmax):
            m, p, xo, yo = T.at(k)
            rx, ry = _residual(p, xo, yo, X)
            rs = _acc(m, rs, rx * rx + ry * ry)
            n0, n1, den1, den2 = prep[k]
            den = den2 * depth + den1
            den = den * den
            j0, j1 = n0 / den, n1 / den
            jtj = _acc(m, jtj, j0 * j0 + j1 * j1)
            dp = _acc(m, dp, j0 * rx + j1 * ry)
        inv = F32(1) / jtj
        dp = dp * inv
        res = np.where(alive, rs / T.nv2, res)
        depth = np.where(alive, depth + dp, depth)
        X = _sel(alive, [d[q] * depth + c[q] for q in range(3)], X)
        cov = np.where(alive, inv, cov)
        iters = iters + alive
    cov9 = [cov] + [np.zeros(T.n, F32) for _ in range(8)]
    return X, cov9, iters


def status_bits(P, offsets, view, pts, cov, mode):
    """bit 0: a non-finite output word; bit 1: the point is not in front of its first view's camera (P2 . X <= 0)."""
    P = np.ascontiguousarray(P, F32).reshape(-1, 12)
    off = np.asarray(offsets, np.int64)
    p = P[np.asarray(view, np.int64)[off[:-1]]]
    pts = np.asarray(pts, F32)
    cov = np.asarray(cov, F32).reshape(len(pts), -1)
    with np.errstate(all="ignore"):
        w = ((p[:, 8] * pts[:, 0] + p[:, 9] * pts[:, 1]) + p[:, 10] * pts[:, 2]) + p[:, 11]
        bad = ~np.isfinite(pts).all(1) | ~np.isfinite(cov[:, :1] if mode == "depth" else cov).all(1)
        return bad.astype(np.int32) | ((w <= 0).astype(np.int32) << 1)


def triangulate(P, offsets, view, x, y, mode="dlt", noiter=10, minres=1e-5, damp_init=2.0, damp_fct=10.0,
                maxdamp=1e10, init=None, campos=None, ptdir=None):
    """Returns dict: pts [n, 3] f32, cov [n, 9] f32 (depth mode: the scalar in column 0, zeros beyond), iters [n] i32,
    status [n] i32. The iterative modes start from `init` ([n, 3])."""
    if mode not in MODES:
        raise ValueError(mode)
    T = _Tracks(P, offsets, view, x, y)
    with np.errstate(all="ignore"):
        if mode == "dlt":
            X, cov, iters = _dlt(T)
        else:
            init = np.asarray(init, F32)
            X0 = [np.ascontiguousarray(init[:, c]) for c in range(3)]
            if mode == "gn":
                X, cov, iters = _gn(T, X0, int(noiter), F32(minres))
            elif mode == "lm":
                X, cov, iters = _lm(T, X0, int(noiter), F32(minres), F32(damp_init), F32(damp_fct), F32(maxdamp))
            else:
                X, cov, iters = _depth(T, X0, np.asarray(campos, F32), np.asarray(ptdir, F32), int(noiter), F32(minres))
    pts = np.stack(X, 1).astype(F32)
    cov = np.stack(cov, 1).astype(F32)
    return dict(pts=pts, cov=cov, iters=iters.astype(np.int32), status=status_bits(T.P, T.off, T.view, pts, cov, mode))


def same_bits(a, b):
    """Word-for-word equality of two f32 arrays; a NaN on both sides counts as equal whatever its sign or payload."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    if a.shape != b.shape:
        return np.zeros(a.shape, bool)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
