"""Window bundle adjustment: item 3 of the list that ends misc_src/run_test_OF_track.py ("BA Adjust cameras and static
points"), with the adjustment on the device (ictr_ba_*).

Semantics (decisions in DESIGN.md §4 "Window bundle adjustment"):

- input: N points ``X`` (3, N) in the first view's frame, observations ``xy`` (S, F, 2, N) of S = 1 or 2 sides in F frames
  ((F, 2, N) is one side), one pinhole camera ``cam = (fc, cc)``, start poses ``init`` (F, 3, 4), ``offset`` (3,) of side 1
  (the script's ``P1[:, 3]``), optionally a point mask as in camfit. Side s of frame f sees ``R_f X + t_f + o_s``.
- a point is adjusted iff its mask bit is set and its three coordinates and all its 2 S F observation coordinates are
  finite; any other point adds exact zeros and comes back unchanged. ``n`` counts the adjusted points; the cost is
  ``c = sum(rx^2 + ry^2) / (n S F)``.
- frame 0 keeps its start pose; the poses of frames 1 .. F - 1 and the adjusted points move. One step solves the
  Marquardt-damped normal equations through the Schur complement of the points: per point a 3 x 3 LDL^T, for the cameras
  a dense 6 (F - 1) LDL^T, both without pivoting, then the back-substitution.
- the schedule is camfit's (DEFAULTS, same accept test, same order of stops, same status codes). A failed solve (a pivot
  that is not finite or not > 0 at any adjusted point or in the reduced system) raises the damping, counts an iteration
  and is retried at the same linearisation.

``adjust_window_host`` restates csrc/ictr_ba_hd.h operation by operation in NumPy f64 and is the statement of record; the
device matches it bit for bit.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from . import _wininputs as W
from . import camfit as F
from ._hostmath import div as _div
from ._lib import check, dp, f64c
from .camfit import CONVERGED, DEFAULTS, FEW_OBS, MAXDAMP, NOITER, START_NOT_FINITE  # noqa: F401

__all__ = ["BundleAdjuster", "adjust_window", "adjust_window_host", "system_host", "MAX_FRAMES", "DEFAULTS", "CONVERGED",
           "NOITER", "MAXDAMP", "FEW_OBS", "START_NOT_FINITE"]

MAX_FRAMES = 32       # kBaMaxFrames
MIN_POINTS = 8
_RUNNING = -1
_START, _TRIAL, _RETRY = 0, 1, 2
_DBL_MAX = F._DBL_MAX


def _vidx(i, j):
    """ba_vidx: the place of V[i][j], i <= j, among the 6 entries of the upper triangle."""
    return i * 3 - i * (i - 1) // 2 + (j - i)


def _ridx(n, i, j):
    """ba_ridx: the place of entry (i, j), i <= j, in the packed upper triangle of the reduced system."""
    return i * n - i * (i - 1) // 2 + (j - i)


def _pairs(nframes):
    """ba_pair: the block pairs (f, g), 1 <= f <= g < F, in the order of their index."""
    return [(f, g) for f in range(1, nframes) for g in range(f, nframes)]


# ---------------------------------------------------------------- per observation and per point (on arrays over the points)
def _obs(G, o, cam, X, xy):
    """ba_obs: rx, ry, jx (6), jy (6), px (3), py (3)."""
    fx, fy = cam[0], cam[1]
    iz, xz, yz, rx, ry = F._project(G, G[3] + o[0], G[7] + o[1], G[11] + o[2], cam, X, xy)
    zero = np.zeros_like(iz)
    qx, qy, qz = xz - o[0] * iz, yz - o[1] * iz, 1.0 - o[2] * iz   # the part of x_cam that cf_update turns, over z
    jx = [fx * iz, zero, fx * (-(xz * iz)), fx * (-(xz * qy)), fx * (qz + xz * qx), fx * (-qy)]
    jy = [zero, fy * iz, fy * (-(yz * iz)), fy * (-(qz + yz * qy)), fy * (yz * qx), fy * qx]
    ax, ay = fx * iz, fy * iz
    px = [ax * (G[q] - xz * G[8 + q]) for q in range(3)]
    py = [ay * (G[4 + q] - yz * G[8 + q]) for q in range(3)]
    return rx, ry, jx, jy, px, py


def _factor3(V, damp):
    """ba_factor3 on arrays: ok, L (3, N) = [1][0], [2][0], [2][1], D (3, N)."""
    n = V.shape[1]
    l = [[None] * 3 for _ in range(3)]
    D = [None] * 3
    ok = np.ones(n, bool)
    for j in range(3):
        d = V[_vidx(j, j)] + damp * V[_vidx(j, j)]
        for q in range(j):
            d = d - l[j][q] * (l[j][q] * D[q])
        ok &= (d > 0.0) & (np.abs(d) <= _DBL_MAX)
        D[j] = d
        for i in range(j + 1, 3):
            s = V[_vidx(j, i)]
            for q in range(j):
                s = s - l[i][q] * (l[j][q] * D[q])
            l[i][j] = s / d
    return ok, [l[1][0], l[2][0], l[2][1]], D


def _solve3(L, D, b):
    """ba_solve3 on arrays."""
    y0 = b[0]
    y1 = b[1] - L[0] * y0
    y2 = (b[2] - L[1] * y0) - L[2] * y1
    x2 = y2 / D[2]
    x1 = y1 / D[1] - L[2] * x2
    x0 = (y0 / D[0] - L[0] * x1) - L[1] * x2
    return [x0, x1, x2]


class _Problem:
    """BaHost: the inputs and the passes."""

    def __init__(self, X, xy, cam, offset, mask):
        self.X0 = F._as_points(X)
        self.n = self.X0.shape[1]
        self.xy = _as_obs(xy, self.n)
        self.S, self.F = self.xy.shape[0], self.xy.shape[1]
        self.cam = F._as_cam(cam)
        self.off = [[0.0, 0.0, 0.0], _as_offset(offset)]
        bits = F._bits_of(F._words_of(mask, self.n), self.n)
        with np.errstate(invalid="ignore"):
            ok = bits & (np.abs(self.X0) <= _DBL_MAX).all(axis=0)
            ok &= (np.abs(self.xy) <= _DBL_MAX).all(axis=(0, 1, 2))
        self.adj = ok
        self.count = int(ok.sum())

    def obs(self, G, f, s, X):
        return _obs([float(v) for v in G[f]], self.off[s], self.cam, X, self.xy[s, f])

    def zeroed(self, a):
        return np.where(self.adj, a, 0.0)

    def point_pass(self, G, X):
        """V (6, N), gp (3, N) at the poses G and the points X."""
        V = [np.zeros(self.n) for _ in range(6)]
        gp = [np.zeros(self.n) for _ in range(3)]
        for f in range(self.F):
            for s in range(self.S):
                rx, ry, _, _, px, py = self.obs(G, f, s, X)
                for i in range(3):
                    for j in range(i, 3):
                        V[_vidx(i, j)] = V[_vidx(i, j)] + (px[i] * px[j] + py[i] * py[j])
                    gp[i] = gp[i] + (px[i] * rx + py[i] * ry)
        return self.zeroed(np.array(V)), self.zeroed(np.array(gp))

    def frame_pass(self, G, X):
        """The frames' ordered sums (F, 28)."""
        out = np.zeros((self.F, 28))
        for f in range(self.F):
            t = [np.zeros(self.n) for _ in range(28)]
            for s in range(self.S):
                rx, ry, jx, jy, _, _ = self.obs(G, f, s, X)
                for i in range(6):
                    for j in range(i, 6):
                        t[F._hidx(i, j)] = t[F._hidx(i, j)] + (jx[i] * jx[j] + jy[i] * jy[j])
                    t[21 + i] = t[21 + i] + (jx[i] * rx + jy[i] * ry)
                t[27] = t[27] + (rx * rx + ry * ry)
            out[f] = F._ordered_sum(self.zeroed(np.array(t)))
        return out

    def w_of(self, G, f, X):
        """W_f (6, 3, N)."""
        W = [[np.zeros(self.n) for _ in range(3)] for _ in range(6)]
        for s in range(self.S):
            _, _, jx, jy, px, py = self.obs(G, f, s, X)
            for a in range(6):
                for q in range(3):
                    W[a][q] = W[a][q] + (jx[a] * px[q] + jy[a] * py[q])
        return W

    def schur_pass(self, G, X, V, gp, damp):
        """The pairs' ordered sums T (npairs, 42) and the number of adjusted points whose 3 x 3 factorisation failed."""
        ok, L, D = _factor3(V, damp)
        nfail = int((self.adj & ~ok).sum())
        W = {f: self.w_of(G, f, X) for f in range(1, self.F)}
        Y = {f: [_solve3(L, D, W[f][a]) for a in range(6)] for f in range(1, self.F)}
        T = np.zeros((len(_pairs(self.F)), 42))
        for p, (f, g) in enumerate(_pairs(self.F)):
            t = np.zeros((42, self.n))
            for a in range(6):
                y = Y[f][a]
                for b in range(6):
                    t[6 * a + b] = (y[0] * W[g][b][0] + y[1] * W[g][b][1]) + y[2] * W[g][b][2]
                t[36 + a] = (y[0] * gp[0] + y[1] * gp[1]) + y[2] * gp[2]
            T[p] = F._ordered_sum(self.zeroed(t))
        return T, nfail

    def assemble(self, U, gc, T, damp):
        """ba_reduced_entry / ba_reduced_rhs: the packed upper triangle and the right-hand side."""
        dim = 6 * (self.F - 1)
        A, rhs = np.zeros(dim * (dim + 1) // 2), np.zeros(dim)
        pidx = {fg: p for p, fg in enumerate(_pairs(self.F))}
        with np.errstate(all="ignore"):
            for i in range(dim):
                f, a = i // 6 + 1, i % 6
                for j in range(i, dim):
                    g, b = j // 6 + 1, j % 6
                    u = np.float64(0.0)
                    if f == g:
                        u = U[f, F._hidx(a, b)]
                        if a == b:
                            u = u + damp * u
                    A[_ridx(dim, i, j)] = u - T[pidx[(f, g)], 6 * a + b]
                rhs[i] = gc[f, a] - T[pidx[(f, f)], 36 + a]
        return np.where(A != A, np.nan, A), np.where(rhs != rhs, np.nan, rhs)  # cf_canon

    def back_pass(self, G, X, V, gp, damp, dc):
        """The points moved by the step: X + V*^-1 (gp - sum_f W_f^T dc_f); a point that is not adjusted stays."""
        _, L, D = _factor3(V, damp)
        b = [gp[0], gp[1], gp[2]]
        for f in range(1, self.F):
            W = self.w_of(G, f, X)
            d = dc[6 * (f - 1):6 * f]
            for q in range(3):
                t = W[0][q] * d[0]
                for a in range(1, 6):
                    t = t + W[a][q] * d[a]
                b[q] = b[q] - t
        dx = _solve3(L, D, b)
        return np.where(self.adj, X + np.array(dx), X)


def _reduced_solve(A, rhs, dim):
    """The LDL^T of the packed triangle, columns left to right (ba_ldl_sum), and ba_ldl_solve: (ok, x)."""
    A = [float(v) for v in A]
    for j in range(dim):
        col = []
        for i in range(j, dim):
            s = A[_ridx(dim, j, i)]
            for q in range(j):
                s = s - A[_ridx(dim, q, i)] * (A[_ridx(dim, q, j)] * A[_ridx(dim, q, q)])
            col.append(s)
        d = col[0]
        if not (d > 0.0 and abs(d) <= _DBL_MAX):
            return False, None
        A[_ridx(dim, j, j)] = d
        for i in range(j + 1, dim):
            A[_ridx(dim, j, i)] = _div(col[i - j], d)
    x = [0.0] * dim
    for i in range(dim):
        s = float(rhs[i])
        for q in range(i):
            s = s - A[_ridx(dim, q, i)] * x[q]
        x[i] = s
    for i in range(dim - 1, -1, -1):
        s = _div(x[i], A[_ridx(dim, i, i)])
        for q in range(i + 1, dim):
            s = s - A[_ridx(dim, i, q)] * x[q]
        x[i] = s
    return True, x


def _stops(st, prm):
    """ba_stops."""
    if not (st["c"] > prm["minres"]):
        st["status"] = CONVERGED
    elif not (st["it"] < prm["noiter"]):
        st["status"] = NOITER
    elif not (st["damp"] < prm["maxdamp"]):
        st["status"] = MAXDAMP


def _cost(P, sums):
    """The cost of ba_decide from the frames' sums."""
    tot = 0.0
    for f in range(P.F):
        tot = tot + float(sums[f, 27])
    if tot != tot:
        tot = math.nan
    c = _div(tot, float(P.count) * float(P.S * P.F))
    return math.nan if c != c else c


# ---------------------------------------------------------------- arguments
def _as_obs(xy, n):
    a = W._as_obs(xy, n, (2, MAX_FRAMES), sides=True)
    if n < MIN_POINTS:
        raise ValueError(f"{n} points (at least {MIN_POINTS})")
    return a


def _as_offset(offset):
    if offset is None:
        return [0.0, 0.0, 0.0]
    o = [float(v) for v in f64c(offset).reshape(-1)]
    if len(o) != 3 or not all(abs(v) <= _DBL_MAX for v in o):
        raise ValueError("offset must be three finite numbers")
    return o


def _result(G, X, cost, damp, iters, status, n):
    from .tracker import util_SE3_group_to_coeff
    G = np.asarray(G, np.float64).reshape(-1, 3, 4)
    p = np.array([util_SE3_group_to_coeff(g) for g in G]).reshape(-1, 6)
    return dict(G=G, p=p, X=None if X is None else np.asarray(X, np.float64), cost=np.float64(cost), damp=np.float64(damp),
                iters=np.int32(iters), status=np.int32(status), n=np.int64(n))


# ---------------------------------------------------------------- the host restatement
def system_host(X, xy, cam, G, damp, offset=None, mask=None):
    """The checker of BundleAdjuster.debug_system: dict n, cost, A (the reduced system's packed upper triangle), rhs,
    V (6, N), gp (3, N), nfail at the poses G and the points X."""
    P = _Problem(X, xy, cam, offset, mask)
    G = F._as_poses(G, P.F)
    damp = float(damp)
    with np.errstate(all="ignore"):
        V, gp = P.point_pass(G, P.X0)
        sums = P.frame_pass(G, P.X0)
        T, nfail = P.schur_pass(G, P.X0, V, gp, damp)
        A, rhs = P.assemble(sums[:, 0:21], sums[:, 21:27], T, damp)
    return dict(n=P.count, cost=_cost(P, sums), A=A, rhs=rhs, V=V, gp=gp, nfail=nfail)


def adjust_window_host(X, xy, cam, offset=None, mask=None, init=None, detail=False, **schedule):
    """The whole adjustment restated on the host (the checker of adjust_window). Returns dict: G (F, 3, 4), p (F, 6) =
    se3_log(G), X (3, N), cost, damp, iters, status, n. detail: also trace (what every step did) and costs (the cost at
    the start and after every accepted step)."""
    P = _Problem(X, xy, cam, offset, mask)
    prm = F._params(schedule)
    G0 = F._as_poses(init, P.F)
    if not np.isfinite(G0).all():
        raise ValueError("a start pose is not finite")
    dim = 6 * (P.F - 1)
    st = dict(G=G0.copy(), Gt=G0.copy(), c=0.0, damp=prm["damp_init"], it=0, status=_RUNNING, phase=_START)
    Xs, Vs, gps = [P.X0, P.X0.copy()], [None, None], [None, None]
    cur = tset = 0
    U = gc = None
    trace, costs = [], []
    with np.errstate(all="ignore"):
        while st["status"] == _RUNNING:
            # the passes at the trial set and ba_decide
            if st["phase"] != _RETRY:
                Vs[tset], gps[tset] = P.point_pass(st["Gt"], Xs[tset])
                sums = P.frame_pass(st["Gt"], Xs[tset])
                c = _cost(P, sums)
                take = False
                if st["phase"] == _START:
                    st["c"] = c
                    if P.count < 3:
                        st["status"] = FEW_OBS
                        break
                    if not F._finite(c):
                        st["status"] = START_NOT_FINITE
                        break
                    take = True
                    trace.append("start")
                else:
                    st["it"] += 1
                    if F._finite(c) and c < st["c"]:
                        imp = st["c"] - c
                        st["G"] = st["Gt"].copy()
                        cur = tset
                        st["c"] = c
                        st["damp"] = _div(st["damp"], prm["damp_fct"])
                        take = True
                        trace.append("accept")
                        if imp <= prm["minres"]:
                            st["status"] = CONVERGED
                    else:
                        st["damp"] = st["damp"] * prm["damp_fct"]
                        trace.append("reject")
                if take:
                    U, gc = sums[:, 0:21].copy(), sums[:, 21:27].copy()
                    costs.append(st["c"])
                st["phase"] = _RETRY
                if st["status"] == _RUNNING:
                    _stops(st, prm)
            if st["status"] != _RUNNING:
                break
            # the reduced system at the accepted set, its solve and ba_solved
            T, nfail = P.schur_pass(st["G"], Xs[cur], Vs[cur], gps[cur], st["damp"])
            A, rhs = P.assemble(U, gc, T, st["damp"])
            ok, dc = (False, None) if nfail else _reduced_solve(A, rhs, dim)
            if ok:
                st["Gt"] = st["G"].copy()
                for f in range(1, P.F):
                    st["Gt"][f] = F._update([float(v) for v in st["G"][f]], dc[6 * (f - 1):6 * f])
                tset = cur ^ 1
                st["phase"] = _TRIAL
                Xs[tset] = P.back_pass(st["G"], Xs[cur], Vs[cur], gps[cur], st["damp"], dc)
            else:
                st["damp"] = st["damp"] * prm["damp_fct"]
                st["it"] += 1
                trace.append("failed-solve")
                _stops(st, prm)
    out = _result(st["G"], Xs[cur].copy(), st["c"], st["damp"], st["it"], st["status"], P.count)
    if detail:
        out["trace"], out["costs"] = trace, np.array(costs)
    return out


# ---------------------------------------------------------------- the device path
class BundleAdjuster(W._MaskedWindowInputs):
    """The device path: one ictr_ba object for N points seen from S sides in F frames."""
    KERNELS = ("point", "frames", "decide", "schur", "gather", "solve", "back")
    _PREFIX, _NOUN, _KINDS = "ba", "adjuster", KERNELS
    _as_obs = staticmethod(_as_obs)

    def __init__(self, n, nframes, nsides=1):
        self._create(n, nframes, nsides)

    def set_offset(self, offset=None):
        check(_lib.load().ictr_ba_set_offset(self._h, dp(np.array(_as_offset(offset)))))

    def run_async(self, init=None, stream=None, **schedule):
        prm = dict(DEFAULTS)
        prm.update(schedule)
        G0 = F._as_poses(init, self.nframes)
        check(_lib.load().ictr_ba_run(self._h, dp(G0), int(prm["noiter"]), float(prm["damp_init"]), float(prm["damp_fct"]),
                                      float(prm["minres"]), float(prm["maxdamp"]), W._stream(stream)))

    def wait(self, points=True):
        """The result of the run in flight; points = False leaves the points on the device (X is None)."""
        G, X = np.zeros((self.nframes, 12)), np.zeros((3, self.n)) if points else None
        cost, damp = C.c_double(), C.c_double()
        iters, status, n = C.c_int32(), C.c_int32(), C.c_int64()
        check(_lib.load().ictr_ba_wait(self._h, dp(G), None if X is None else dp(X), C.byref(cost), C.byref(damp),
                                       C.byref(iters), C.byref(status), C.byref(n)))
        return _result(G, X, cost.value, damp.value, iters.value, status.value, n.value)

    def debug_system(self, G, damp, X=None):
        """Inspection (ictr_debug_ba_system): the passes, the Schur pass and the assembly alone at the poses G and the
        points X (default: the set ones). dict as system_host."""
        G = F._as_poses(G, self.nframes)
        Xa = None
        if X is not None:
            Xa = F._as_points(X)
            if Xa.shape[1] != self.n:
                raise ValueError(f"X {Xa.shape}, the adjuster was made for (3, {self.n})")
        dim = 6 * (self.nframes - 1)
        A, rhs, V, gp = np.zeros(dim * (dim + 1) // 2), np.zeros(dim), np.zeros((6, self.n)), np.zeros((3, self.n))
        n, nfail, cost = C.c_int64(), C.c_int64(), C.c_double()
        check(_lib.load().ictr_debug_ba_system(self._h, dp(G), None if Xa is None else dp(Xa), float(damp), C.byref(n),
                                               C.byref(cost), dp(A), dp(rhs), dp(V), dp(gp), C.byref(nfail)))
        return dict(n=n.value, cost=cost.value, A=A, rhs=rhs, V=V, gp=gp, nfail=nfail.value)


def adjust_window(X, xy, cam, offset=None, mask=None, init=None, stream=None, **schedule):
    """The adjustment on the device; arguments and result as adjust_window_host (without detail)."""
    X = F._as_points(X)
    xy = _as_obs(xy, X.shape[1])
    F._params(schedule)
    b = BundleAdjuster(X.shape[1], xy.shape[1], xy.shape[0])
    b.set_points(X)
    b.set_observations(xy)
    b.set_camera(cam)
    b.set_offset(offset)
    b.set_mask(mask)
    b.run_async(init, stream, **schedule)
    return b.wait()
