"""Window camera RANSAC: "RANSAC camera estimation left for whole sequence, check right for consistency"
(misc_src/run_test_OF_track.py, TODO 1), with the trials on the device (ictr_camransac_*).

Semantics (DESIGN.md §4 "Window camera RANSAC"); all arithmetic is f64 in a fixed order, only ``+ - * / sqrt``:

- input: N points ``X`` (3, N) of a track window in the first view's frame, their observations ``xy`` (S, F, 2, N), S = 1
  (left only) or 2 (left and right; the bundle adjuster's layout), one pinhole camera ``cam = (fc, cc)``, the side offset
  ``o_1`` (``o_0 = 0``), optionally a mask (bool (N,) or words).
- counts: point i counts iff its mask bit is set, its three coordinates are finite and all its 2 S F observation
  coordinates are finite (the adjuster's "adjusted" rule). A point that does not count is never an inlier.
- draws: trial g draws ``ran_draw<4>(mix(seed), g, N)`` over all N, the pose sampler's stream. A trial fails with fewer
  than 4 distinct indices or a drawn point that does not count.
- hypothesis of frame f (frame 0 included): ``ransac._hypothesis(seed, g, left_f.x, left_f.y, X, fx, fy, cx, cy, kc = 0)``;
  the pose is ``G_f = [R | t]``, ``t[r] = -R[r][0] c[0] - R[r][1] c[1] - R[r][2] c[2]`` left to right. A frame without a
  hypothesis is twelve NaN, and the trial fails; by arithmetic alone it then scores nothing.
- score: ``d(i, f, s)`` is cf_reproj_point at ``t_f + o_s``; ``dd_i`` its maximum over f (outer) and s (inner), a NaN stays;
  point i is an inlier iff it counts and ``dd_i < thresh``. No depth test.
- winner: the largest count, the lowest trial on ties. No successful trial: ``best_trial = -1``, ``best_count = 0``, every
  G NaN, the words zero, ``dd`` NaN, the draws -1.

``window_ransac_host`` restates csrc/ictr_camransac_hd.h operation by operation in Python / NumPy f64 and is the statement
of record; the device matches it bit for bit.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import _wininputs as W
from . import ransac as _ransac
from ._hostmath import M64 as _M64, draw_indices_n
from ._lib import check, dp, f64c
from ._wininputs import _pack_words
from .camfit import _DBL_MAX, _as_cam, _as_points, _bits_of, _project, _words_of

__all__ = ["window_ransac", "window_ransac_host", "CameraRansac", "MAX_TRIALS", "MAX_FRAMES"]

MAX_TRIALS = 1 << 20
MAX_FRAMES = 64  # kCrMaxFrames


def _as_obs(xy, n):
    """(S, F, 2, N); (F, 2, N) is one side."""
    return W._as_obs(xy, n, (1, MAX_FRAMES), sides=True)


def _as_offset(offset, nsides):
    if offset is None:
        if nsides == 2:
            raise ValueError("two sides need the offset of the second")
        return None
    o = f64c(offset).reshape(-1)
    if o.size != 3 or not np.isfinite(o).all():
        raise ValueError("offset must be 3 finite numbers")
    return o


def _counts(bits, X, xy):
    """cr_counts on arrays: (N,) bool."""
    with np.errstate(invalid="ignore"):
        ok = bits.copy()
        for v in (X[0], X[1], X[2]):
            ok &= np.abs(v) <= _DBL_MAX
        for s in range(xy.shape[0]):
            for f in range(xy.shape[1]):
                ok &= np.abs(xy[s, f, 0]) <= _DBL_MAX
                ok &= np.abs(xy[s, f, 1]) <= _DBL_MAX
    return ok


def _pose(R, c):
    """cr_pose: G (12,) = [R | t] from R (3, 3) and the camera centre c."""
    G = [0.0] * 12
    for r in range(3):
        for k in range(3):
            G[4 * r + k] = float(R[r][k])
        G[4 * r + 3] = -float(R[r][0]) * float(c[0]) - float(R[r][1]) * float(c[1]) - float(R[r][2]) * float(c[2])
    return G


def _trial(seed, g, X, xy, cam, counts):
    """The draws and the F poses of trial g: (status, draws (4,) with -1 where none, G (F, 12))."""
    n, F = X.shape[1], xy.shape[1]
    fx, fy, cx, cy = cam
    idx = draw_indices_n(seed, g, n, 4)
    draws = np.full(4, -1, np.int32)
    draws[:len(idx)] = idx
    G = np.full((F, 12), np.nan)
    if len(idx) < 4 or not all(counts[i] for i in idx):
        return 0, draws, G
    status = 1
    for f in range(F):
        _, R, c = _ransac._hypothesis(seed, g, xy[0, f, 0], xy[0, f, 1], X, fx, fy, cx, cy, 0.0)
        if R is None:
            status = 0
        else:
            G[f] = _pose(R, c)
    return status, draws, G


def _distances(G, X, xy, cam, off):
    """dd (N,): per point the maximum over the frames (outer) and sides (inner) of the reprojection distance at
    t_f + o_s; a NaN stays, as the canonical one."""
    S, F, n = xy.shape[0], xy.shape[1], X.shape[1]
    o = [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0] if off is None else [float(v) for v in off]]
    dd = np.full(n, -1.0)
    with np.errstate(all="ignore"):
        for f in range(F):
            g = [float(v) for v in G[f]]
            for s in range(S):
                _, _, _, rx, ry = _project(g, g[3] + o[s][0], g[7] + o[s][1], g[11] + o[s][2], cam, X, xy[s, f])
                d = np.sqrt(rx * rx + ry * ry)
                dd = np.where(d != d, np.nan, np.where(d > dd, d, dd))
    return np.where(dd != dd, np.nan, dd)


def _log(G):
    """p (F, 6) = se3_log(G) by the library's host log map; NaN where G is."""
    G = f64c(G).reshape(-1, 12)
    p = np.full((G.shape[0], 6), np.nan)
    for f in range(G.shape[0]):
        if np.isfinite(G[f]).all():
            _lib.load().ictr_se3_group_to_coeff_d(dp(p[f]), dp(G[f]))
    return p


def _result(best_trial, best_count, draws, G, mask, dd, p=None):
    mask = np.asarray(mask, bool)
    G = np.asarray(G, np.float64).reshape(-1, 3, 4)
    return dict(best_trial=int(best_trial), best_count=int(best_count), draws=np.asarray(draws, np.int32), G=G,
                p=_log(G) if p is None else np.asarray(p, np.float64).reshape(-1, 6), words=_pack_words(mask), mask=mask,
                inliers=np.nonzero(mask)[0], dd=np.asarray(dd, np.float64))


def _args(X, xy, cam, offset, mask):
    X = _as_points(X)
    n = X.shape[1]
    if n < 4:
        raise ValueError("at least 4 points are needed")
    xy, cam = _as_obs(xy, n), _as_cam(cam)
    return X, xy, cam, _as_offset(offset, xy.shape[0]), _words_of(mask, n)


def window_ransac_host(X, xy, cam, offset=None, mask=None, ntrials=100, thresh=2.0, seed=0, detail=False):
    """The whole RANSAC restated on the host (the checker of window_ransac). Returns dict: best_trial, best_count,
    draws (4,), G (F, 3, 4), p (F, 6) = se3_log(G), words (inlier bits, uint64), mask (N,) bool, inliers (indices),
    dd (N,). detail: also status (ntrials,), cnt (ntrials,), all_draws (ntrials, 4), all_G (ntrials, F, 12),
    all_dd (ntrials, N) and counts (N,) bool."""
    X, xy, cam, off, words = _args(X, xy, cam, offset, mask)
    n, F = X.shape[1], xy.shape[1]
    thr = float(thresh)
    if thr != thr:
        raise ValueError("thresh is NaN")
    if not 1 <= int(ntrials) <= MAX_TRIALS:
        raise ValueError("ntrials 1 .. 2^20")
    counts = _counts(_bits_of(words, n), X, xy)
    best = None
    st, cn, dr, gs, ds = [], [], [], [], []
    for g in range(int(ntrials)):
        status, draws, G = _trial(seed, g, X, xy, cam, counts)
        dd = _distances(G, X, xy, cam, off)
        with np.errstate(invalid="ignore"):
            inl = counts & (dd < thr)
        c = int(inl.sum())
        if status and (best is None or c > best[1]):
            best = (g, c, draws, G, inl, dd)
        if detail:
            st.append(status), cn.append(c), dr.append(draws), gs.append(G), ds.append(dd)
    if best is None:
        out = _result(-1, 0, np.full(4, -1), np.full((F, 12), np.nan), np.zeros(n, bool), np.full(n, np.nan))
    else:
        out = _result(*best)
    if detail:
        out.update(status=np.array(st, np.int32), cnt=np.array(cn, np.uint32), all_draws=np.array(dr, np.int32),
                   all_G=np.array(gs), all_dd=np.array(ds), counts=counts)
    return out


class CameraRansac(W._WindowInputs):
    """The device path: one ictr_camransac object for N points seen in F frames from S sides. debug_inputs answers in
    words the mask in effect: every point's bit where no mask is set."""
    _PREFIX, _NOUN, _KINDS = "camransac", "RANSAC", ("hyp", "score", "select", "mask")  # mask: flags + mask
    _as_obs = staticmethod(_as_obs)

    def __init__(self, n, nframes, nsides=2):
        self._create(n, nframes, nsides)

    @property
    def chunk(self):
        return _lib.load().ictr_camransac_chunk_size(self._h)

    def set_offset(self, offset):
        check(_lib.load().ictr_camransac_set_offset(self._h, dp(f64c(offset).reshape(3))))

    def run_async(self, ntrials=100, thresh=2.0, seed=0, stream=None):
        check(_lib.load().ictr_camransac_run(self._h, int(ntrials), float(thresh), int(seed) & _M64, W._stream(stream)))

    def debug_trials(self, thresh=2.0, seed=0, first_trial=0, count=1):
        """Inspection (ictr_debug_camransac_trials): the hypothesis and score kernels alone over trials first_trial ..
        first_trial + count - 1. dict: status (count,), draws (count, 4), G (count, F, 12), cnt (count,)."""
        n, first = int(count), int(first_trial)
        if n < 1 or first < 0 or first + n > MAX_TRIALS:  # before the output arrays are sized by it
            raise _lib.IctrError(f"debug_trials: trials {first} + {n} (1 .. 2^20 trials below 2^20)")
        status, draws = np.zeros(n, np.int32), np.zeros((n, 4), np.int32)
        G, cnt = np.zeros((n, self.nframes, 12)), np.zeros(n, np.uint32)
        i32 = C.POINTER(C.c_int32)
        check(_lib.load().ictr_debug_camransac_trials(self._h, float(thresh), int(seed) & _M64, first, n,
                                                      status.ctypes.data_as(i32), draws.ctypes.data_as(i32), dp(G),
                                                      cnt.ctypes.data_as(C.POINTER(C.c_uint32))))
        return dict(status=status, draws=draws, G=G, cnt=cnt)

    def wait(self):
        best = np.zeros(2, np.int64)
        draws = np.zeros(4, np.int32)
        G, p = np.zeros((self.nframes, 12)), np.zeros((self.nframes, 6))
        words = np.zeros(self.nwords, np.uint64)
        dd = np.zeros(self.n)
        i64 = C.POINTER(C.c_int64)
        check(_lib.load().ictr_camransac_wait(self._h, best[0:1].ctypes.data_as(i64), best[1:2].ctypes.data_as(i64),
                                              draws.ctypes.data_as(C.POINTER(C.c_int32)), dp(G), dp(p),
                                              words.ctypes.data_as(C.POINTER(C.c_uint64)), dp(dd)))
        return _result(best[0], best[1], draws, G, _bits_of(words, self.n), dd, p)


def window_ransac(X, xy, cam, offset=None, mask=None, ntrials=100, thresh=2.0, seed=0, stream=None):
    """The RANSAC on the device. X (3, N), xy (S, F, 2, N) (or (F, 2, N) for the left side alone), cam = (fc, cc),
    offset (3,) of the second side, mask: bool (N,) or words. Returns window_ransac_host's dict."""
    X, xy, cam, off, words = _args(X, xy, cam, offset, mask)
    r = CameraRansac(X.shape[1], xy.shape[1], xy.shape[0])
    r.set_points(X)
    r.set_observations(xy)
    r.set_camera(((cam[0], cam[1]), (cam[2], cam[3])))
    if off is not None and xy.shape[0] == 2:
        r.set_offset(off)
    r.set_mask(words)
    r.run_async(ntrials, thresh, seed, stream)
    return r.wait()
