"""An independent judge of one 8-point fit at 50 digits (mpmath), sharing no step with the elimination and the Jacobi
sweeps of invcompcamtrack_amd.fsplit: the Hartley-normalised design matrix in exact-input arithmetic, its null vector as
the last right singular vector (mpmath.svd_r), rank 2 by zeroing the smallest singular value of the 3x3 (svd_r again),
denormalisation, and the point-to-epipolar-line distances, all in mpf from the f64 inputs."""
import mpmath as mp

DPS = 50  # set inside workdps(): other judges of the suite (tests/ransac_mp.py) keep their own global precision


def _f(x):
    return mp.mpf(float(x))


def _normalise(x, y):
    cx, cy = sum(x) / 8, sum(y) / 8
    d = sum(mp.sqrt((a - cx) ** 2 + (b - cy) ** 2) for a, b in zip(x, y)) / 8
    s = mp.sqrt(2) / d
    T = mp.matrix([[s, 0, -s * cx], [0, s, -s * cy], [0, 0, 1]])
    return [(a - cx) * s for a in x], [(b - cy) * s for b in y], T


def fit(xa, ya, xb, yb):
    """(F as mp.matrix 3x3, sigma_8 / sigma_1 of the design matrix) for four sequences of 8 finite f64 values."""
    with mp.workdps(DPS):
        return _fit(xa, ya, xb, yb)


def _fit(xa, ya, xb, yb):
    xa, ya, Ta = _normalise([_f(v) for v in xa], [_f(v) for v in ya])
    xb, yb, Tb = _normalise([_f(v) for v in xb], [_f(v) for v in yb])
    A = mp.zeros(9, 9)  # the ninth row stays 0: svd_r of a square matrix gives the full V
    for r in range(8):
        row = [xb[r] * xa[r], xb[r] * ya[r], xb[r], yb[r] * xa[r], yb[r] * ya[r], yb[r], xa[r], ya[r], mp.mpf(1)]
        for c in range(9):
            A[r, c] = row[c]
    _, S, V = mp.svd_r(A)
    order = sorted(range(9), key=lambda i: S[i], reverse=True)
    ratio = S[order[7]] / S[order[0]]
    f = [V[order[8], c] for c in range(9)]
    G = mp.matrix(3, 3)
    for k in range(9):
        G[k // 3, k % 3] = f[k]
    U3, S3, V3 = mp.svd_r(G)
    o3 = sorted(range(3), key=lambda i: S3[i], reverse=True)
    D = mp.zeros(3, 3)
    for i in o3[:2]:
        D[i, i] = S3[i]
    G2 = U3 * D * V3
    F = Tb.T * G2 * Ta
    nrm = mp.sqrt(sum(F[i, j] ** 2 for i in range(3) for j in range(3)))
    return F / nrm, ratio


def dist(F, xa, ya, xb, yb):
    """Distances (list of mpf) of the points (xb, yb) to the lines F (xa, ya, 1)."""
    with mp.workdps(DPS):
        return _dist(F, xa, ya, xb, yb)


def _dist(F, xa, ya, xb, yb):
    out = []
    for a, b, c, d in zip(xa, ya, xb, yb):
        a, b, c, d = _f(a), _f(b), _f(c), _f(d)
        l0 = F[0, 0] * a + F[0, 1] * b + F[0, 2]
        l1 = F[1, 0] * a + F[1, 1] * b + F[1, 2]
        l2 = F[2, 0] * a + F[2, 1] * b + F[2, 2]
        out.append(abs(l0 * c + l1 * d + l2) / mp.sqrt(l0 * l0 + l1 * l1))
    return out
