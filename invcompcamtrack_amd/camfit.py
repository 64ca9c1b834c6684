"""One camera per frame of a track window: misc_src/run_test_OF_track.py:360-411 ("Triangulate points based on baseline
in first frame", "Fit cameras", "Reprojection test into left and right camera"), with the fit and the reprojection means
on the device (ictr_camfit_*).

Semantics (deviations from cv2.solvePnP in DESIGN.md §4 "Camera fit"):

- input: N points ``X`` (3, N) in any world frame, F frames of observations ``xy`` (F, 2, N) in pixels, one pinhole camera
  ``cam = (fc, cc)`` without distortion, per frame a start pose ``[R | t]`` with ``x_cam = R X + t`` (the identity when
  none is given), optionally a point mask (bool (N,), or the inlier words of split_static).
- an observation counts in a frame iff its mask bit is set and its three point and two pixel coordinates are finite; there
  is no depth test. Per frame the mean squared reprojection residual ``c = sum(rx^2 + ry^2) / n`` is minimised.
- per pass H (21 entries), b (6), s are summed in an order that depends on N alone (``_ordered_sum``): chunks of 1024
  points, 4 points per lane serially, a pairwise tree over the 256 lanes, the chunks serially.
- ``(H + damp diag(H)) d = b`` by LDL^T without pivoting (``_solve``); the pose moves by the Cayley retraction (``_update``).
- the schedule (``_step``): noiter 20, damp_init 2, damp_fct 10, minres 1e-5, maxdamp 1e10 as triang.c:327. A trial pose is
  accepted iff its cost is finite and smaller. Stops, tested in this order: cost <= minres or an accepted improvement
  <= minres (CONVERGED), noiter solves tried (NOITER), damp >= maxdamp (MAXDAMP). A failed solve raises the damping and
  counts as an iteration. Fewer than 3 counted observations (FEW_OBS) and a start cost that is not finite
  (START_NOT_FINITE) leave the start pose.

``fit_cameras_host`` / ``reprojection_errors_host`` restate csrc/ictr_camfit_hd.h operation by operation in Python / NumPy
f64; the device matches them bit for bit.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._hostmath import div as _div
from ._lib import check, dp, f64c
from ._wininputs import _MaskedWindowInputs, _as_cam, _as_obs, _as_points, _stream, _words_of

__all__ = ["CameraFitter", "fit_cameras", "fit_cameras_host", "reprojection_errors", "reprojection_errors_host",
           "pass_host", "depth_from_disparity", "points_from_first_view", "observations_from_stereo_tracks", "CHUNK",
           "CONVERGED", "NOITER", "MAXDAMP", "FEW_OBS", "START_NOT_FINITE", "DEFAULTS"]

BLOCK, PER_LANE = 256, 4        # kCfBlock, kCfPerLane of csrc/ictr_camfit_hd.h
CHUNK = BLOCK * PER_LANE        # kCfChunk, C
CONVERGED, NOITER, MAXDAMP, FEW_OBS, START_NOT_FINITE = 0, 1, 2, 3, 4  # ICTR_CAMFIT_*
_RUNNING = -1
DEFAULTS = dict(noiter=20, damp_init=2.0, damp_fct=10.0, minres=1e-5, maxdamp=1e10)
MAX_ITER = 1000
_DBL_MAX = 1.7976931348623157e308


def _hidx(i, j):
    """cf_hidx: the place of H[i][j], i <= j, among the 21 entries of the upper triangle, row-major."""
    return i * 6 - i * (i - 1) // 2 + (j - i)


def _finite(v):
    return abs(v) <= _DBL_MAX


def _project(G, tx, ty, tz, cam, X, xy):
    """cf_project on arrays: iz, xz, yz, rx, ry."""
    fx, fy, cx, cy = cam
    Xc = ((G[0] * X[0] + G[1] * X[1]) + G[2] * X[2]) + tx
    Yc = ((G[4] * X[0] + G[5] * X[1]) + G[6] * X[2]) + ty
    Zc = ((G[8] * X[0] + G[9] * X[1]) + G[10] * X[2]) + tz
    iz = 1.0 / Zc
    xz = Xc * iz
    yz = Yc * iz
    rx = xy[0] - (fx * xz + cx)
    ry = xy[1] - (fy * yz + cy)
    return iz, xz, yz, rx, ry


def _counted(bits, X, xy):
    """cf_counted on arrays."""
    with np.errstate(invalid="ignore"):
        ok = bits.copy()
        for v in (X[0], X[1], X[2], xy[0], xy[1]):
            ok &= np.abs(v) <= _DBL_MAX
    return ok


def _terms(G, cam, X, xy, counted):
    """cf_point on arrays: (28, N)."""
    fx, fy = cam[0], cam[1]
    with np.errstate(all="ignore"):
        iz, xz, yz, rx, ry = _project(G, G[3], G[7], G[11], cam, X, xy)
        zero = np.zeros_like(iz)
        jx = [fx * iz, zero, fx * (-(xz * iz)), fx * (-(xz * yz)), fx * (1.0 + xz * xz), fx * (-yz)]
        jy = [zero, fy * iz, fy * (-(yz * iz)), fy * (-(1.0 + yz * yz)), fy * (xz * yz), fy * xz]
        t = np.zeros((28, iz.size))
        for i in range(6):
            for j in range(i, 6):
                t[_hidx(i, j)] = np.where(counted, jx[i] * jx[j] + jy[i] * jy[j], 0.0)
            t[21 + i] = np.where(counted, jx[i] * rx + jy[i] * ry, 0.0)
        t[27] = np.where(counted, rx * rx + ry * ry, 0.0)
    return t


def _ordered_sum(t):
    """The sums of the rows of t (T, N) in the stated order: chunks of CHUNK points; in a chunk lane l of BLOCK adds its
    PER_LANE points l, BLOCK + l, .. to +0.0 serially, the lanes are added by the pairwise tree, the chunks to +0.0
    serially; a NaN comes out as the canonical one."""
    T, n = t.shape
    nch = (n + CHUNK - 1) // CHUNK
    tp = np.zeros((T, nch * CHUNK))
    tp[:, :n] = t
    v = tp.reshape(T, nch, PER_LANE, BLOCK)
    with np.errstate(all="ignore"):
        acc = np.zeros((T, nch, BLOCK))
        for r in range(PER_LANE):
            acc = acc + v[:, :, r, :]
        while acc.shape[2] > 1:
            acc = acc[:, :, 0::2] + acc[:, :, 1::2]
        tot = np.zeros(T)
        for ch in range(nch):
            tot = tot + acc[:, ch, 0]
    return np.where(tot != tot, np.nan, tot)


def _solve(H, b, damp):
    """cf_solve: (ok, x) of (H + damp diag(H)) x = b by LDL^T; H: 21 floats, b: 6."""
    L = [[0.0] * 6 for _ in range(6)]
    D = [0.0] * 6
    ok = True
    for j in range(6):
        d = H[_hidx(j, j)] + damp * H[_hidx(j, j)]
        for q in range(j):
            d = d - L[j][q] * (L[j][q] * D[q])
        if not (d > 0.0) or not _finite(d):
            ok = False
        D[j] = d
        for i in range(j + 1, 6):
            s = H[_hidx(j, i)]
            for q in range(j):
                s = s - L[i][q] * (L[j][q] * D[q])
            L[i][j] = _div(s, d)
    y = [0.0] * 6
    for i in range(6):
        s = b[i]
        for q in range(i):
            s = s - L[i][q] * y[q]
        y[i] = s
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = _div(y[i], D[i])
        for q in range(i + 1, 6):
            s = s - L[q][i] * x[q]
        x[i] = s
    return ok, x


def _update(G, d):
    """cf_update: the pose (12 floats) moved by d = (dt, dw) through the Cayley retraction."""
    a0, a1, a2 = d[3] * 0.5, d[4] * 0.5, d[5] * 0.5
    aa = (a0 * a0 + a1 * a1) + a2 * a2
    den, kk = 1.0 + aa, 1.0 - aa
    r = [_div(kk + 2.0 * (a0 * a0), den), _div(2.0 * (a0 * a1) - 2.0 * a2, den), _div(2.0 * (a0 * a2) + 2.0 * a1, den),
         _div(2.0 * (a1 * a0) + 2.0 * a2, den), _div(kk + 2.0 * (a1 * a1), den), _div(2.0 * (a1 * a2) - 2.0 * a0, den),
         _div(2.0 * (a2 * a0) - 2.0 * a1, den), _div(2.0 * (a2 * a1) + 2.0 * a0, den), _div(kk + 2.0 * (a2 * a2), den)]
    Go = [0.0] * 12
    for i in range(3):
        for j in range(3):
            Go[4 * i + j] = (r[3 * i] * G[j] + r[3 * i + 1] * G[4 + j]) + r[3 * i + 2] * G[8 + j]
        Go[4 * i + 3] = ((r[3 * i] * G[3] + r[3 * i + 1] * G[7]) + r[3 * i + 2] * G[11]) + d[i]
    return Go


class _State:
    """CfState after cf_init."""

    def __init__(self, G0, prm):
        self.G, self.Gt = list(G0), list(G0)
        self.c, self.damp = 0.0, prm["damp_init"]
        self.H, self.b = [0.0] * 21, [0.0] * 6
        self.n, self.it, self.status, self.phase = 0, 0, _RUNNING, 0
        self.trace = []  # per step: what it did ("start", "accept", "reject", "failed-solve")


def _step(s, sums, prm):
    """cf_step."""
    if s.status != _RUNNING:
        return
    n = sums[28]
    c = _div(sums[27], n)
    if c != c:
        c = math.nan
    take = False
    if s.phase == 0:
        s.phase = 1
        s.n = int(n)
        s.c = c
        if n < 3.0:
            s.status = FEW_OBS
            return
        if not _finite(c):
            s.status = START_NOT_FINITE
            return
        take = True
        s.trace.append("start")
    else:
        s.it = s.it + 1
        if _finite(c) and c < s.c:
            imp = s.c - c
            s.G = list(s.Gt)
            s.c = c
            s.damp = _div(s.damp, prm["damp_fct"])
            take = True
            s.trace.append("accept")
            if imp <= prm["minres"]:
                s.status = CONVERGED
        else:
            s.damp = s.damp * prm["damp_fct"]
            s.trace.append("reject")
    if take:
        s.H = [float(v) for v in sums[0:21]]
        s.b = [float(v) for v in sums[21:27]]
    if s.status != _RUNNING:
        return
    while True:
        if not (s.c > prm["minres"]):
            s.status = CONVERGED
            return
        if not (s.it < prm["noiter"]):
            s.status = NOITER
            return
        if not (s.damp < prm["maxdamp"]):
            s.status = MAXDAMP
            return
        ok, d = _solve(s.H, s.b, s.damp)
        if ok:
            s.Gt = _update(s.G, d)
            return
        s.damp = s.damp * prm["damp_fct"]
        s.it = s.it + 1
        s.trace.append("failed-solve")


# ---------------------------------------------------------------- arguments
def _as_poses(G, nframes):
    if G is None:
        G = np.tile(np.eye(3, 4).reshape(1, 12), (nframes, 1))
    a = f64c(G).reshape(-1, 12)
    if a.shape[0] != nframes:
        raise ValueError(f"{a.shape[0]} poses for {nframes} frames")
    return a


def _bits_of(words, n):
    if words is None:
        return np.ones(n, bool)
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


def _params(kw):
    prm = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in prm:
            raise TypeError(f"unknown schedule parameter {k!r}")
        prm[k] = v
    prm["noiter"] = int(prm["noiter"])
    for k in ("damp_init", "damp_fct", "minres", "maxdamp"):
        prm[k] = float(prm[k])
    if not (0 <= prm["noiter"] <= MAX_ITER and 0.0 < prm["damp_init"] <= _DBL_MAX and 1.0 < prm["damp_fct"] <= _DBL_MAX
            and 0.0 <= prm["minres"] <= _DBL_MAX and prm["maxdamp"] > 0.0):
        raise ValueError("needs 0 <= noiter <= 1000, damp_init > 0, damp_fct > 1, minres >= 0 (all finite), maxdamp > 0")
    return prm


def _result(G, cost, damp, iters, status, n):
    from .tracker import util_SE3_group_to_coeff
    G = np.asarray(G, np.float64).reshape(-1, 3, 4)
    p = np.array([util_SE3_group_to_coeff(g) for g in G]).reshape(-1, 6)
    return dict(G=G, p=p, cost=np.asarray(cost, np.float64), damp=np.asarray(damp, np.float64),
                iters=np.asarray(iters, np.int32), status=np.asarray(status, np.int32), n=np.asarray(n, np.int64))


# ---------------------------------------------------------------- the host restatement
def pass_host(X, xy, cam, G, mask=None):
    """The checker of CameraFitter.debug_pass: n (F,), s (F,), H (F, 21), b (F, 6) of one pass at the poses G."""
    X = _as_points(X)
    n = X.shape[1]
    xy, cam = _as_obs(xy, n), _as_cam(cam)
    G = _as_poses(G, xy.shape[0])
    bits = _bits_of(_words_of(mask, n), n)
    out = dict(n=[], s=[], H=[], b=[])
    for f in range(xy.shape[0]):
        counted = _counted(bits, X, xy[f])
        sums = _ordered_sum(_terms([float(v) for v in G[f]], cam, X, xy[f], counted))
        out["n"].append(int(counted.sum()))
        out["s"].append(sums[27])
        out["H"].append(sums[0:21])
        out["b"].append(sums[21:27])
    return dict(n=np.array(out["n"], np.int64), s=np.array(out["s"]), H=np.array(out["H"]), b=np.array(out["b"]))


def fit_cameras_host(X, xy, cam, mask=None, init=None, detail=False, **schedule):
    """The whole fit restated on the host (the checker of fit_cameras). Returns dict: G (F, 3, 4), p (F, 6) =
    se3_log(G), cost, damp, iters, status, n (all (F,)). detail: also trace, per frame the list of what every step did."""
    X = _as_points(X)
    n = X.shape[1]
    xy, cam, prm = _as_obs(xy, n), _as_cam(cam), _params(schedule)
    G0 = _as_poses(init, xy.shape[0])
    if not np.isfinite(G0).all():
        raise ValueError("a start pose is not finite")
    bits = _bits_of(_words_of(mask, n), n)
    states = []
    for f in range(xy.shape[0]):
        counted = _counted(bits, X, xy[f])
        cnt = float(int(counted.sum()))
        s = _State([float(v) for v in G0[f]], prm)
        while s.status == _RUNNING:
            sums = [float(v) for v in _ordered_sum(_terms(s.Gt, cam, X, xy[f], counted))] + [cnt]
            _step(s, sums, prm)
        states.append(s)
    out = _result([s.G for s in states], [s.c for s in states], [s.damp for s in states], [s.it for s in states],
                  [s.status for s in states], [s.n for s in states])
    if detail:
        out["trace"] = [s.trace for s in states]
    return out


def reprojection_errors_host(X, xy, cam, G, mask=None, offset=None):
    """Per frame the mean reprojection distance (px) of the counted observations at the poses G, with `offset` (3,)
    added to every translation (run_test_OF_track.py:407-411: t + P1[:, 3] for the right camera), and their number.
    Returns (mean_err (F,), n (F,)); the host form of reprojection_errors, same bits."""
    X = _as_points(X)
    n = X.shape[1]
    xy, cam = _as_obs(xy, n), _as_cam(cam)
    G = _as_poses(G, xy.shape[0])
    dt = [0.0, 0.0, 0.0] if offset is None else [float(v) for v in f64c(offset).reshape(3)]
    bits = _bits_of(_words_of(mask, n), n)
    err, cnt = np.empty(xy.shape[0]), np.empty(xy.shape[0], np.int64)
    for f in range(xy.shape[0]):
        g = [float(v) for v in G[f]]
        counted = _counted(bits, X, xy[f])
        with np.errstate(all="ignore"):
            _, _, _, rx, ry = _project(g, g[3] + dt[0], g[7] + dt[1], g[11] + dt[2], cam, X, xy[f])
            d = np.where(counted, np.sqrt(rx * rx + ry * ry), 0.0)
        tot = float(_ordered_sum(d[None])[0])
        cnt[f] = int(counted.sum())
        e = _div(tot, float(cnt[f])) if cnt[f] > 0 else math.nan
        err[f] = math.nan if e != e else e
    return err, cnt


# ---------------------------------------------------------------- the device path
class CameraFitter(_MaskedWindowInputs):
    """The device path: one ictr_camfit object for N points seen in F frames."""
    _PREFIX, _NOUN, _KINDS = "camfit", "fitter", ("pass", "step")

    def __init__(self, n, nframes):
        self._create(n, nframes)

    def set_observations_from_window(self, win, right=False):
        """One side of observations_from_stereo_tracks of a counted StereoTrackWindow, on the device."""
        check(self._c("set_observations_from_window")(self._h, win._h, int(bool(right))))

    def run_async(self, init=None, stream=None, **schedule):
        prm = dict(DEFAULTS)
        prm.update(schedule)
        G0 = _as_poses(init, self.nframes)
        check(_lib.load().ictr_camfit_run(self._h, dp(G0), int(prm["noiter"]), float(prm["damp_init"]),
                                          float(prm["damp_fct"]), float(prm["minres"]), float(prm["maxdamp"]),
                                          _stream(stream)))

    def wait(self):
        F = self.nframes
        G, cost, damp = np.zeros((F, 12)), np.zeros(F), np.zeros(F)
        iters, status, n = np.zeros(F, np.int32), np.zeros(F, np.int32), np.zeros(F, np.int64)
        i32 = C.POINTER(C.c_int32)
        check(_lib.load().ictr_camfit_wait(self._h, dp(G), dp(cost), dp(damp), iters.ctypes.data_as(i32),
                                           status.ctypes.data_as(i32), n.ctypes.data_as(C.POINTER(C.c_int64))))
        return _result(G, cost, damp, iters, status, n)

    def reprojection_errors(self, G, offset=None):
        G = _as_poses(G, self.nframes)
        err, n = np.zeros(self.nframes), np.zeros(self.nframes, np.int64)
        dt = None if offset is None else f64c(offset).reshape(3)
        check(_lib.load().ictr_camfit_reproj(self._h, dp(G), None if dt is None else dp(dt), dp(err),
                                             n.ctypes.data_as(C.POINTER(C.c_int64))))
        return err, n

    def debug_pass(self, G):
        """Inspection (ictr_debug_camfit_pass): k_camfit_pass and the ordered sum alone at the poses G. dict: n (F,),
        s (F,), H (F, 21), b (F, 6)."""
        G = _as_poses(G, self.nframes)
        F = self.nframes
        n, s, H, b = np.zeros(F, np.int64), np.zeros(F), np.zeros((F, 21)), np.zeros((F, 6))
        check(_lib.load().ictr_debug_camfit_pass(self._h, dp(G), n.ctypes.data_as(C.POINTER(C.c_int64)), dp(s), dp(H),
                                                 dp(b)))
        return dict(n=n, s=s, H=H, b=b)


def _fitter(X, xy, cam, mask):
    X = _as_points(X)
    xy = _as_obs(xy, X.shape[1])
    f = CameraFitter(X.shape[1], xy.shape[0])
    f.set_points(X)
    f.set_observations(xy)
    f.set_camera(cam)
    f.set_mask(mask)
    return f


def fit_cameras(X, xy, cam, mask=None, init=None, stream=None, **schedule):
    """The fit on the device. X (3, N), xy (F, 2, N), cam = (fc, cc), mask: bool (N,) or the inlier words of
    split_static, init: (F, 3, 4) start poses (default: the identity), schedule: noiter, damp_init, damp_fct, minres,
    maxdamp. Returns dict: G (F, 3, 4), p (F, 6) = se3_log(G) taken on the host, cost, damp, iters, status, n (all (F,))."""
    f = _fitter(X, xy, cam, mask)
    f.run_async(init, stream, **schedule)
    return f.wait()


def reprojection_errors(X, xy, cam, G, mask=None, offset=None):
    """(mean_err (F,), n (F,)) on the device; see reprojection_errors_host."""
    return _fitter(X, xy, cam, mask).reprojection_errors(G, offset)


# ---------------------------------------------------------------- the script's steps around the fit, on the host
def depth_from_disparity(xy_t, fx, baseline):
    """run_test_OF_track.py:361-362: b = x_right - x_left in frame 0, depth = baseline fx / b. xy_t (N, 4, bsize);
    baseline: P1[0, 3] of the script (signed like the disparity)."""
    xy = np.asarray(xy_t, np.float64)
    if xy.ndim != 3 or xy.shape[1] != 4:
        raise ValueError(f"xy_t must be (N, 4, bsize), got {xy.shape}")
    with np.errstate(all="ignore"):
        return float(baseline) * float(fx) / (xy[:, 2, 0] - xy[:, 0, 0])


def points_from_first_view(xy_t, cam, depth):
    """run_test_OF_track.py:366-371: the frame-0 left pixels in normalised coordinates, z = 1, times the depth:
    X (3, N) in the first left camera's frame."""
    xy = np.asarray(xy_t, np.float64)
    fx, fy, cx, cy = _as_cam(cam)
    d = np.asarray(depth, np.float64)
    with np.errstate(all="ignore"):
        return np.stack([(xy[:, 0, 0] - cx) / fx * d, (xy[:, 1, 0] - cy) / fy * d, d])


def observations_from_stereo_tracks(xy_t):
    """The script's stereo layout xy_t (N, 4, bsize) as the fit's observations: (left (bsize, 2, N), right
    (bsize, 2, N))."""
    xy = np.asarray(xy_t, np.float64)
    if xy.ndim != 3 or xy.shape[1] != 4:
        raise ValueError(f"xy_t must be (N, 4, bsize), got {xy.shape}")
    t = np.ascontiguousarray(xy.transpose(2, 1, 0))
    return np.ascontiguousarray(t[:, 0:2]), np.ascontiguousarray(t[:, 2:4])
