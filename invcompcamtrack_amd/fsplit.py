"""Static / moving split of a track window by fundamental-matrix RANSAC: misc_src/run_test_OF_track.py:309-343
("Divide points in static and dynamic using the fundamental matrix"), with the rounds on the device (ictr_fsplit_*).

Semantics (deviations from the script in DESIGN.md §4 "Static split"):

- input: P "view pairs" over the same N points, ``pairs[p] = (xa, ya, xb, yb)[N]`` (f64).
- trial ``t`` draws 8 distinct point indices from the counter-based stream of ransac.draw_indices (``draw_indices_n``);
  the same 8 serve all P pairs. No 8 distinct indices after 1024 draws: the trial fails.
- per (trial, pair) an 8-point fundamental matrix, ``xb^T F xa = 0`` (``fit_f8``): Hartley normalisation, the null
  vector of the 8x9 design matrix by Gaussian elimination with full pivoting, rank 2 by a one-sided Jacobi SVD of the
  3x3, denormalisation, unit Frobenius norm. It fails (F = NaN) when a mean distance is 0, a pivot is exactly 0 or an
  entry of F is not finite.
- score (``epiline_dist`` = func_F_transfer_points): the distance of xb to the line F xa; per point the maximum over
  the pairs (a NaN stays); inlier iff that maximum is < thresh. A trial with a failed fit has no inliers.
- the trial with the most inliers wins, the lowest index on ties; no inlier anywhere is a normal result.

``fit_f8`` / ``epiline_dist`` / ``split_static_host`` restate csrc/ictr_fsplit_hd.h operation by operation in Python /
NumPy f64; the device matches them bit for bit.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._hostmath import M64 as _M64, div as _div, draw_indices_n
from ._lib import check, dp, f64c
from ._wininputs import _pack_words

__all__ = ["fit_f8", "epiline_dist", "draw_indices_n", "trials_host", "split_static_host", "split_static", "StaticSplitter",
           "pairs_from_tracks", "pairs_from_stereo_tracks", "SWEEPS"]

SWEEPS = 5          # kFsSweeps of csrc/ictr_fsplit_hd.h
MAX_TRIALS = 1 << 20
_SQRT2 = 1.4142135623730951
_NAN9 = [math.nan] * 9


def _normalise(x, y):
    """fs_normalise: (x', y', s, tx, ty) or None when the mean distance is 0."""
    sx, sy = x[0], y[0]
    for k in range(1, 8):
        sx = sx + x[k]
        sy = sy + y[k]
    cx, cy = sx / 8.0, sy / 8.0
    x = [v - cx for v in x]
    y = [v - cy for v in y]
    sd = 0.0
    for k in range(8):
        sd = sd + math.sqrt(x[k] * x[k] + y[k] * y[k])
    d = sd / 8.0
    if d == 0.0:
        return None
    s = _div(_SQRT2, d)
    return [v * s for v in x], [v * s for v in y], s, -(s * cx), -(s * cy)


def _rotate(U, V, p, q):
    """fs_rotate: one Hestenes rotation of columns p, q of U and V (lists of 9, row-major)."""
    al = (U[p] * U[p] + U[3 + p] * U[3 + p]) + U[6 + p] * U[6 + p]
    be = (U[q] * U[q] + U[3 + q] * U[3 + q]) + U[6 + q] * U[6 + q]
    ga = (U[p] * U[q] + U[3 + p] * U[3 + q]) + U[6 + p] * U[6 + q]
    if ga == 0.0:
        return
    ze = _div(be - al, 2.0 * ga)
    t = _div(-1.0 if ze < 0.0 else 1.0, abs(ze) + math.sqrt(1.0 + ze * ze))
    c = 1.0 / math.sqrt(1.0 + t * t)
    s = c * t
    for r in range(3):
        up, uq = U[3 * r + p], U[3 * r + q]
        U[3 * r + p] = c * up - s * uq
        U[3 * r + q] = s * up + c * uq
        vp, vq = V[3 * r + p], V[3 * r + q]
        V[3 * r + p] = c * vp - s * vq
        V[3 * r + q] = s * vp + c * vq


def _null_vector(A):
    """The null vector of the 8x9 A (list of rows, changed in place) by Gaussian elimination with full pivoting, free
    variable 1; None when a pivot is exactly 0."""
    perm = list(range(9))
    for k in range(8):
        best, pr, pc = abs(A[k][k]), k, k
        for i in range(k, 8):
            for j in range(k, 9):
                v = abs(A[i][j])
                if v > best:
                    best, pr, pc = v, i, j
        A[k], A[pr] = A[pr], A[k]
        if pc != k:
            for i in range(8):
                A[i][k], A[i][pc] = A[i][pc], A[i][k]
            perm[k], perm[pc] = perm[pc], perm[k]
        piv = A[k][k]
        if piv == 0.0:
            return None
        for i in range(k + 1, 8):
            f = A[i][k] / piv
            for j in range(k + 1, 9):
                A[i][j] = A[i][j] - f * A[k][j]
    z = [0.0] * 9
    z[8] = 1.0
    for k in range(7, -1, -1):
        acc = A[k][k + 1] * z[k + 1]
        for j in range(k + 2, 9):
            acc = acc + A[k][j] * z[j]
        z[k] = -acc / A[k][k]
    f = [0.0] * 9
    for j in range(9):
        f[perm[j]] = z[j]
    return f


def _rank2(U, sweeps):
    """The nearest rank-2 matrix of the 3x3 U (list of 9): one-sided Jacobi, the shortest column dropped."""
    U = list(U)
    V = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    for _ in range(sweeps):
        _rotate(U, V, 0, 1)
        _rotate(U, V, 0, 2)
        _rotate(U, V, 1, 2)
    n = [(U[c] * U[c] + U[3 + c] * U[3 + c]) + U[6 + c] * U[6 + c] for c in range(3)]
    drop, nm = 0, n[0]
    if n[1] < nm:
        nm, drop = n[1], 1
    if n[2] < nm:
        drop = 2
    for r in range(3):
        U[3 * r + drop] = 0.0
    return [(U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1]) + U[3 * r + 2] * V[3 * c + 2]
            for r in range(3) for c in range(3)]


def _fit_f8_list(xa, ya, xb, yb, sweeps=SWEEPS):
    """fs_fit8 on four lists of 8 floats -> list of 9 (NaN nine times on failure)."""
    na, nb = _normalise(xa, ya), _normalise(xb, yb)
    if na is None or nb is None:
        return _NAN9
    xa, ya, sa, txa, tya = na
    xb, yb, sb, txb, tyb = nb
    A = [[xb[r] * xa[r], xb[r] * ya[r], xb[r], yb[r] * xa[r], yb[r] * ya[r], yb[r], xa[r], ya[r], 1.0]
         for r in range(8)]
    f = _null_vector(A)
    if f is None:
        return _NAN9
    G = _rank2(f, sweeps)
    H = [0.0] * 9
    for r in range(3):
        H[3 * r + 0] = G[3 * r + 0] * sa
        H[3 * r + 1] = G[3 * r + 1] * sa
        H[3 * r + 2] = (G[3 * r + 0] * txa + G[3 * r + 1] * tya) + G[3 * r + 2]
    F = [0.0] * 9
    for c in range(3):
        F[c] = sb * H[c]
        F[3 + c] = sb * H[3 + c]
        F[6 + c] = (txb * H[c] + tyb * H[3 + c]) + H[6 + c]
    ss = 0.0
    for k in range(9):
        ss = ss + F[k] * F[k]
    nrm = math.sqrt(ss)
    F = [_div(v, nrm) for v in F]
    if not all(math.isfinite(v) for v in F):
        return _NAN9
    return F


def fit_f8(xa, xb, sweeps=SWEEPS):
    """The 8-point fundamental matrix of xa (8, 2) -> xb (8, 2), ``[xb 1] F [xa 1]^T = 0``, unit Frobenius norm; the
    host restatement of the device's fit. Returns F (3, 3), or None when the fit fails."""
    xa, xb = np.asarray(xa, np.float64), np.asarray(xb, np.float64)
    if xa.shape != (8, 2) or xb.shape != (8, 2):
        raise ValueError(f"fit_f8 needs two (8, 2) arrays, got {xa.shape} and {xb.shape}")
    F = _fit_f8_list(xa[:, 0].tolist(), xa[:, 1].tolist(), xb[:, 0].tolist(), xb[:, 1].tolist(), sweeps)
    return None if F[0] != F[0] else np.array(F).reshape(3, 3)


def _dist(F, xa, ya, xb, yb):
    """fs_dist on arrays; F: 9 floats."""
    with np.errstate(all="ignore"):
        l0 = ((F[0] * xa) + (F[1] * ya)) + F[2]
        l1 = ((F[3] * xa) + (F[4] * ya)) + F[5]
        l2 = ((F[6] * xa) + (F[7] * ya)) + F[8]
        return np.abs(((l0 * xb) + (l1 * yb)) + l2) / np.sqrt(l0 * l0 + l1 * l1)


def epiline_dist(F, xa, xb):
    """func_F_transfer_points (func_util_geom.py:52-55): the distance of every xb (N, 2) to its epipolar line
    F [xa 1]^T, the line scaled to a^2 + b^2 = 1."""
    F = np.asarray(F, np.float64).reshape(9)
    xa, xb = np.asarray(xa, np.float64), np.asarray(xb, np.float64)
    return _dist([float(v) for v in F], f64c(xa[:, 0]), f64c(xa[:, 1]), f64c(xb[:, 0]), f64c(xb[:, 1]))


def _as_pairs(pairs):
    a = f64c(pairs)
    if a.ndim != 3 or a.shape[1] != 4:
        raise ValueError(f"pairs must be (P, 4, N): rows xa, ya, xb, yb per pair; got {a.shape}")
    return a


def _max_dist(F, pairs):
    """dd (N,): per point the maximum over the pairs of its distance (fs_max: a NaN stays). F: (P, 9)."""
    dd = np.full(pairs.shape[2], -1.0)
    for p in range(pairs.shape[0]):
        d = _dist([float(v) for v in F[p]], pairs[p, 0], pairs[p, 1], pairs[p, 2], pairs[p, 3])
        with np.errstate(invalid="ignore"):
            dd = np.where(d != d, np.nan, np.where(d > dd, d, dd))
    return dd


def _trial_host(pairs, seed, t):
    """(status, draws (8,) with -1 for what was not drawn, F (P, 9)) of trial t."""
    P, _, n = pairs.shape
    idx = draw_indices_n(seed, t, n, 8)
    draws = np.full(8, -1, np.int32)
    draws[:len(idx)] = idx
    F = np.full((P, 9), np.nan)
    if len(idx) < 8:
        return 0, draws, F
    for p in range(P):
        F[p] = _fit_f8_list(*(pairs[p, c, idx].tolist() for c in range(4)))
    return int(not np.isnan(F[:, 0]).any()), draws, F


def trials_host(pairs, thresh=2.0, seed=0, first_trial=0, count=1):
    """The checker of StaticSplitter.debug_trials: status (count,), draws (count, 8), F (count, P, 9) and cnt (count,)
    of trials first_trial .. first_trial + count - 1 restated on the host."""
    pairs = _as_pairs(pairs)
    thr = float(thresh)
    status, draws, F, cnt = [], [], [], []
    for t in range(int(first_trial), int(first_trial) + int(count)):
        st, d, f = _trial_host(pairs, seed, t)
        c = 0
        if st:
            with np.errstate(invalid="ignore"):
                c = int(np.count_nonzero(_max_dist(f, pairs) < thr))
        status.append(st)
        draws.append(d)
        F.append(f)
        cnt.append(c)
    return dict(status=np.array(status, np.int32), draws=np.array(draws, np.int32), F=np.array(F),
                cnt=np.array(cnt, np.uint32))


def split_static_host(pairs, ntrials=100, thresh=2.0, seed=0, detail=False):
    """The whole split restated on the host (the checker of split_static). Returns dict: inliers (indices), mask
    (N,) bool, dd (N,), F (P, 3, 3), best_trial, best_count, draws (8,), words (inlier bits, uint64). detail: also
    status (ntrials,), cnt (ntrials,), all_draws (ntrials, 8), all_F (ntrials, P, 9)."""
    pairs = _as_pairs(pairs)
    P, _, n = pairs.shape
    if n < 8:
        raise ValueError("at least 8 points are needed")
    thr = float(thresh)
    best = None
    status, cnt, all_draws, all_F = [], [], [], []
    for t in range(int(ntrials)):
        st, draws, F = _trial_host(pairs, seed, t)
        c = 0
        dd = None
        if st:
            dd = _max_dist(F, pairs)
            with np.errstate(invalid="ignore"):
                c = int(np.count_nonzero(dd < thr))
        if best is None or c > best[0]:
            best = (c, t, draws, F, dd)
        if detail:
            status.append(st)
            cnt.append(c)
            all_draws.append(draws)
            all_F.append(F)
    c, t, draws, F, dd = best
    if dd is None:
        dd = _max_dist(F, pairs)
    with np.errstate(invalid="ignore"):
        mask = dd < thr
    out = _result(t, c, draws, F, mask, dd)
    if detail:
        out.update(status=np.array(status, np.int32), cnt=np.array(cnt, np.uint32),
                   all_draws=np.array(all_draws, np.int32), all_F=np.array(all_F))
    return out


def _result(best_trial, best_count, draws, F, mask, dd):
    mask = np.asarray(mask, bool)
    return dict(inliers=np.nonzero(mask)[0], mask=mask, dd=np.asarray(dd, np.float64),
                F=np.asarray(F, np.float64).reshape(-1, 3, 3), best_trial=int(best_trial), best_count=int(best_count),
                draws=np.asarray(draws, np.int32), words=_pack_words(mask))


class StaticSplitter:
    """The device path: one ictr_fsplit object for N points in P view pairs."""

    def __init__(self, n, npairs):
        self._h = C.c_void_p()
        check(_lib.load().ictr_fsplit_create(C.byref(self._h), int(n), int(npairs)))
        self.n, self.npairs = int(n), int(npairs)
        self.nwords = (self.n + 63) // 64

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.load().ictr_fsplit_destroy(self._h)
            self._h = None

    def set_pairs(self, pairs):
        a = _as_pairs(pairs)
        if a.shape[0] != self.npairs or a.shape[2] != self.n:
            raise ValueError(f"pairs {a.shape}, the splitter was made for ({self.npairs}, 4, {self.n})")
        check(_lib.load().ictr_fsplit_set_pairs(self._h, dp(a)))

    def set_pairs_from_window(self, win):
        """The view pairs of a counted StereoTrackWindow, written on the device (ictr_fsplit_set_pairs_from_window):
        pairs_from_stereo_tracks of the window's xy_t, which is not formed. Enqueued on the null stream."""
        check(_lib.load().ictr_fsplit_set_pairs_from_window(self._h, win._h))

    def debug_pairs(self):
        """Inspection (ictr_debug_fsplit_pairs): the pairs (P, 4, N) as they stand on the device."""
        a = np.zeros((self.npairs, 4, self.n))
        check(_lib.load().ictr_debug_fsplit_pairs(self._h, dp(a)))
        return a

    def run_async(self, ntrials=100, thresh=2.0, seed=0, stream=None):
        sp = getattr(stream, "cuda_stream", stream)
        check(_lib.load().ictr_fsplit_run(self._h, int(ntrials), float(thresh), int(seed) & _M64, C.c_void_p(sp or 0)))

    def set_timing(self, on=True):
        """Record the stages' device time stamps on the next runs (kernel_times)."""
        check(_lib.load().ictr_fsplit_set_timing(self._h, int(bool(on))))

    def kernel_times(self):
        """ms of the last waited run spent in (fit, score, select, mask), summed over its chunks."""
        ms = np.zeros(4, np.float32)
        check(_lib.load().ictr_fsplit_get_kernel_times(self._h, ms.ctypes.data_as(_lib.FP)))
        return dict(zip(("fit", "score", "select", "mask"), (float(v) for v in ms)))

    def debug_trials(self, thresh=2.0, seed=0, first_trial=0, count=1):
        """Inspection (ictr_debug_fsplit_trials): the fit and score kernels alone over trials first_trial ..
        first_trial + count - 1. dict: status (count,), draws (count, 8), F (count, P, 9), cnt (count,)."""
        n, first = int(count), int(first_trial)
        if n < 1 or first < 0 or first + n > MAX_TRIALS:  # before the output arrays are sized by it
            raise _lib.IctrError(f"debug_trials: trials {first} + {n} (1 .. 2^20 trials below 2^20)")
        status, draws = np.zeros(n, np.int32), np.zeros((n, 8), np.int32)
        F, cnt = np.zeros((n, self.npairs, 9)), np.zeros(n, np.uint32)
        i32 = C.POINTER(C.c_int32)
        check(_lib.load().ictr_debug_fsplit_trials(self._h, float(thresh), int(seed) & _M64, int(first_trial), n,
                                                   status.ctypes.data_as(i32), draws.ctypes.data_as(i32), dp(F),
                                                   cnt.ctypes.data_as(C.POINTER(C.c_uint32))))
        return dict(status=status, draws=draws, F=F, cnt=cnt)

    def wait(self):
        best = np.zeros(2, np.int64)
        draws = np.zeros(8, np.int32)
        F = np.zeros((self.npairs, 9))
        words = np.zeros(self.nwords, np.uint64)
        dd = np.zeros(self.n)
        i64 = C.POINTER(C.c_int64)
        check(_lib.load().ictr_fsplit_wait(self._h, best[0:1].ctypes.data_as(i64), best[1:2].ctypes.data_as(i64),
                                           draws.ctypes.data_as(C.POINTER(C.c_int32)), dp(F),
                                           words.ctypes.data_as(C.POINTER(C.c_uint64)), dp(dd)))
        mask = np.unpackbits(words.view(np.uint8), bitorder="little")[:self.n].astype(bool)
        out = _result(best[0], best[1], draws, F, mask, dd)
        out["words"] = words
        return out


def split_static(pairs, ntrials=100, thresh=2.0, seed=0, stream=None):
    """The split on the device. Returns dict: inliers (indices of the static points), mask (N,), dd (N,) the largest
    epipolar distance of every point under the winning trial, F (P, 3, 3), best_trial, best_count, draws (8,),
    words (the inlier bits, uint64)."""
    a = _as_pairs(pairs)
    s = StaticSplitter(a.shape[2], a.shape[0])
    s.set_pairs(a)
    s.run_async(ntrials, thresh, seed, stream)
    return s.wait()


def _half(bsize):
    return bsize // 2, (bsize + 1) // 2  # frame pairs, and the offset ceil(bsize / 2) of the later frame


def pairs_from_tracks(tracks):
    """View pairs of one block of PointTracker.tracks(): tracks (M, 2, bsize) -> (pairs (bsize // 2, 4, K), rows (K,)).
    Pair fr is (frame fr, frame fr + ceil(bsize / 2)) (run_test_OF_track.py:322-323); rows with a NaN anywhere are
    compacted out, `rows` holds the original indices of those kept."""
    tr = np.asarray(tracks, np.float64)
    if tr.ndim != 3 or tr.shape[1] != 2:
        raise ValueError(f"tracks must be (M, 2, bsize), got {tr.shape}")
    npairs, off = _half(tr.shape[2])
    rows = np.nonzero(~np.isnan(tr).any(axis=(1, 2)))[0]
    tr = tr[rows]
    pairs = np.empty((npairs, 4, len(rows)))
    for fr in range(npairs):
        pairs[fr, 0], pairs[fr, 1] = tr[:, 0, fr], tr[:, 1, fr]
        pairs[fr, 2], pairs[fr, 3] = tr[:, 0, fr + off], tr[:, 1, fr + off]
    return pairs, rows


def pairs_from_stereo_tracks(xy_t):
    """View pairs of the script's stereo layout: xy_t (N, 4, bsize) = left x, y, right x, y per frame -> (pairs
    (2 (bsize // 2), 4, K), rows (K,)). Per frame pair (fr, fr_f = fr + ceil(bsize / 2)) first left fr -> right fr_f,
    then right fr -> left fr_f (run_test_OF_track.py:326-331); rows with a NaN are compacted out."""
    xy = np.asarray(xy_t, np.float64)
    if xy.ndim != 3 or xy.shape[1] != 4:
        raise ValueError(f"xy_t must be (N, 4, bsize), got {xy.shape}")
    npairs, off = _half(xy.shape[2])
    rows = np.nonzero(~np.isnan(xy).any(axis=(1, 2)))[0]
    xy = xy[rows]
    pairs = np.empty((2 * npairs, 4, len(rows)))
    for fr in range(npairs):
        pairs[2 * fr, 0:2] = xy[:, 0:2, fr].T
        pairs[2 * fr, 2:4] = xy[:, 2:4, fr + off].T
        pairs[2 * fr + 1, 0:2] = xy[:, 2:4, fr].T
        pairs[2 * fr + 1, 2:4] = xy[:, 0:2, fr + off].T
    return pairs, rows
