"""Flow producer for the reference's ``misc_src/run_*OF*`` drivers.

Those drivers get their displacement fields from an external binary of the author's OF_DIS repository
(``run_OF_RGB`` / ``run_DE_RGB``, ``misc_src/run_test_OF_track.py:90-108``, ``run_OF_point_track.py.ipynb`` cell 2)
which is not part of the reference. This module replaces it with the in-tree HIP point tracker (``ictr_patchflow``:
per-patch translation inverse-compositional Lucas-Kanade, pyramidal, one wave64 per patch) and re-creates the
notebook's loop: corners -> forward / backward flow -> ``oftrack.addframe`` -> ``savetofile``.

The loop exists twice: ``run_OF_point_track`` (corners, fill, up-sampling and ``addframe`` in NumPy on the host) and
``run_OF_point_track_hip`` (``good_features_hip``, ``FlowGrid``, ``PointTracker``: the same stages in ictr_frontend.hip,
bit for bit the same tracks, nothing but the frames crossing the bus per pair).

Build-defined (no reference implementation exists to pin it): oracle = ``oracle/np_patchflow.py``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, fp
from .classoftrack import oftrack
from .tracker import Pyramid

__all__ = ["track_points", "partition_patches", "dense_flow", "good_features", "run_OF_point_track", "last_kernel_ms",
           "last_form", "track_disparity", "dense_disparity", "disparity_last_kernel_ms", "disparity_last_form",
           "good_features_hip", "FlowGrid", "PointTracker", "run_OF_point_track_hip"]


def last_kernel_ms():
    """Duration of the k_patchflow launch of the last track_points call (HIP events), or None."""
    ms = float(_lib.load().ictr_patchflow_last_kernel_ms())
    return ms if ms >= 0 else None


def last_form():
    """Kernel form of this thread's last k_patchflow launch: pixels per lane * 10 + waves per patch (11, 41, 161 or 82),
    0 before the first. ICTR_PF_WPP=1 / 2 in the environment (read once per process) forces one / two waves per patch."""
    return int(_lib.load().ictr_patchflow_last_form())


def partition_patches(npatches, world):
    """Contiguous, balanced patch ranges: rank r owns [lo, hi). The patches are mutually independent (each owns its two
    parameters: SURVEY.md §8e, BASELINE config 4), so this axis needs no collective in the data path."""
    base, rem = divmod(npatches, world)
    out, lo = [], 0
    for r in range(world):
        hi = lo + base + (1 if r < rem else 0)
        out.append((lo, hi))
        lo = hi
    return out


def track_points(pyr_a, pyr_b, pts, psz=15, lv_f=None, lv_l=0, maxiter=10, eps=0.01, dist=None, group=None, _local=None):
    """Track K points from frame A to frame B. pts: (K,2) level-0 pixel coordinates (x,y).
    Returns (new_pts (K,2) float32 with NaN rows for lost points, status (K,) bool, iters (K,) int32).

    dist (torch.distributed, initialised; optional `group`): BASELINE config 4's multi-GPU form -- every rank holds both
    frames (its own pyramids on its own GPU) and tracks the contiguous range partition_patches(K, world)[rank] of the K
    patches; rank 0 gathers the ranges in rank order and returns the full arrays, the other ranks return None. The
    result on rank 0 equals the single-process result bit for bit (a patch's arithmetic does not depend on what else
    is in its launch). `_local` replaces the GPU call in the CPU tests of the partition / gather logic."""
    pts = np.atleast_2d(np.asarray(pts, np.float32))
    if dist is not None:
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        lo, hi = partition_patches(pts.shape[0], world)[rank]
        local = _local if _local is not None else (
            lambda q: track_points(pyr_a, pyr_b, q, psz, lv_f, lv_l, maxiter, eps) if len(q) else
            (np.zeros((0, 2), np.float32), np.zeros(0, bool), np.zeros(0, np.int32)))
        mine = local(pts[lo:hi])
        parts = [None] * world if rank == 0 else None
        dist.gather_object(mine, parts, dst=0, group=group)
        if rank != 0:
            return None
        return (np.concatenate([q[0] for q in parts], 0), np.concatenate([q[1] for q in parts], 0),
                np.concatenate([q[2] for q in parts], 0))
    K = pts.shape[0]
    lv_f = pyr_a.lv_f if lv_f is None else lv_f
    soa = np.ascontiguousarray(pts.T)
    out = np.empty((2, K), np.float32)
    status = np.zeros(K, np.int32)
    iters = np.zeros(K, np.int32)
    check(_lib.load().ictr_patchflow(pyr_a._h, pyr_b._h, fp(soa), K, psz, lv_f, lv_l, maxiter, float(eps), fp(out),
                                     status.ctypes.data_as(_lib.IP), iters.ctypes.data_as(_lib.IP)))
    return np.ascontiguousarray(out.T), status.astype(bool), iters


def disparity_last_kernel_ms():
    """Duration of the k_patchdisp launch of the last track_disparity call (HIP events), or None."""
    ms = float(_lib.load().ictr_patchdisp_last_kernel_ms())
    return ms if ms >= 0 else None


def disparity_last_form():
    """Kernel form of this thread's last k_patchdisp launch: 11, 41 or 82 by the patch size alone, 0 before the first."""
    return int(_lib.load().ictr_patchdisp_last_form())


def track_disparity(pyr_a, pyr_b, pts, psz=15, lv_f=None, lv_l=0, maxiter=10, eps=0.01):
    """track_points for a rectified stereo pair (``ictr_patchdisp``): a 1-parameter search along x. Same arguments and
    types; new[:, 1] has pts[:, 1]'s bits for a tracked point. A patch of vertical edges alone is kept (track_points
    loses it), a patch of horizontal edges alone is lost."""
    pts = np.atleast_2d(np.asarray(pts, np.float32))
    K = pts.shape[0]
    lv_f = pyr_a.lv_f if lv_f is None else lv_f
    soa = np.ascontiguousarray(pts.T)
    out = np.empty((2, K), np.float32)
    status = np.zeros(K, np.int32)
    iters = np.zeros(K, np.int32)
    check(_lib.load().ictr_patchdisp(pyr_a._h, pyr_b._h, fp(soa), K, psz, lv_f, lv_l, maxiter, float(eps), fp(out),
                                     status.ctypes.data_as(_lib.IP), iters.ctypes.data_as(_lib.IP)))
    return np.ascontiguousarray(out.T), status.astype(bool), iters


def dense_disparity(pyr_a, pyr_b, step=4, psz=15, lv_f=None, maxiter=10, eps=0.01):
    """dense_flow with the nodes tracked by track_disparity: the definition of FlowGrid.compute_x's result. The y plane
    is +0.0 everywhere."""
    return dense_flow(pyr_a, pyr_b, step, psz, lv_f, maxiter, eps, _track=track_disparity)


def dense_flow(pyr_a, pyr_b, step=4, psz=15, lv_f=None, maxiter=10, eps=0.01, _track=None):
    """(H, W, 2) float32 displacement field A -> B: patches tracked on a `step`-pixel grid, bilinearly up-sampled;
    lost grid points take the displacement of the nearest tracked one in their row/column scan (0 if none)."""
    w, h = pyr_a.w, pyr_a.h
    xs = np.arange(step // 2, w, step, dtype=np.float32)
    ys = np.arange(step // 2, h, step, dtype=np.float32)
    gx, gy = np.meshgrid(xs, ys)
    pts = np.stack([gx.ravel(), gy.ravel()], 1)
    new, ok, _ = (_track or track_points)(pyr_a, pyr_b, pts, psz=psz, lv_f=lv_f, maxiter=maxiter, eps=eps)
    d = (new - pts).reshape(len(ys), len(xs), 2)
    bad = ~ok.reshape(len(ys), len(xs))
    if bad.any():
        d[bad] = np.nan
        for axis in (1, 0):  # forward/backward fill along rows, then columns
            for rev in (False, True):
                v = d[:, ::-1] if (rev and axis == 1) else d[::-1] if rev else d
                idx = np.isnan(v[..., 0])
                pos = np.where(~idx, np.arange(v.shape[axis]).reshape((-1, 1) if axis == 0 else (1, -1)), 0)
                np.maximum.accumulate(pos, axis=axis, out=pos)
                filled = np.take_along_axis(v, pos[..., None].repeat(2, -1), axis=axis)
                v[idx] = filled[idx]
        d[np.isnan(d)] = 0.0
    # bilinear up-sampling to every pixel (grid nodes sit at step//2 + k*step)
    fx = np.clip((np.arange(w) - step // 2) / step, 0, len(xs) - 1)
    fy = np.clip((np.arange(h) - step // 2) / step, 0, len(ys) - 1)
    x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
    x1, y1 = np.minimum(x0 + 1, len(xs) - 1), np.minimum(y0 + 1, len(ys) - 1)
    ax, ay = (fx - x0)[None, :, None], (fy - y0)[:, None, None]
    top = d[y0][:, x0] * (1 - ax) + d[y0][:, x1] * ax
    bot = d[y1][:, x0] * (1 - ax) + d[y1][:, x1] * ax
    return (top * (1 - ay) + bot * ay).astype(np.float32)


def good_features(img, maxcorners=1000, quality=0.001, mindist=5, win=3):
    """Shi-Tomasi style corner picker standing in for cv2.goodFeaturesToTrack(gray, 1000, 0.001, 5) of the reference's
    notebook (cv2 is not available here; the reference does not pin the detector): minimum eigenvalue of
    the windowed structure tensor, strongest first, greedy minimum distance. Returns (K,2) float32 (x,y)."""
    img = np.asarray(img, np.float64)
    gx = np.zeros_like(img)
    gy = np.zeros_like(img)
    gx[:, 1:-1] = img[:, 2:] - img[:, :-2]
    gy[1:-1, :] = img[2:, :] - img[:-2, :]

    def box(a):
        c = np.cumsum(np.cumsum(np.pad(a, ((win + 1, win), (win + 1, win))), 0), 1)
        k = 2 * win + 1
        return c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]

    sxx, sxy, syy = box(gx * gx), box(gx * gy), box(gy * gy)
    lam = 0.5 * (sxx + syy) - np.sqrt(0.25 * (sxx - syy) ** 2 + sxy * sxy)
    lam[:mindist], lam[-mindist:], lam[:, :mindist], lam[:, -mindist:] = 0, 0, 0, 0
    thr = quality * lam.max()
    # local maxima in a 3x3 neighbourhood
    p = np.pad(lam, 1, constant_values=-1)
    ismax = np.ones_like(lam, bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if dy != 1 or dx != 1:
                ismax &= lam >= p[dy:dy + lam.shape[0], dx:dx + lam.shape[1]]
    ys, xs = np.nonzero(ismax & (lam > thr))
    order = np.argsort(-lam[ys, xs], kind="stable")
    taken = np.zeros((lam.shape[0] // mindist + 2, lam.shape[1] // mindist + 2), bool)
    out = []
    for i in order:
        cy, cx = ys[i] // mindist, xs[i] // mindist
        if taken[cy, cx]:
            continue
        taken[cy, cx] = True
        out.append((xs[i], ys[i]))
        if len(out) >= maxcorners:
            break
    return np.array(out, np.float32).reshape(-1, 2)


def run_OF_point_track(frames, bsize=10, psz=15, lv_f=3, step=4, maxcorners=1000, th_flowvalid_ratio=0.2,
                       th_flowvalid_abs=1.0, savefile=None):
    """The loop of misc_src/run_OF_point_track.py.ipynb cell 2 with the external flow binary replaced by dense_flow():
    per consecutive frame pair: forward and backward flow, new corners on the first frame of the pair, addframe.
    frames: list of grey float images. Returns the oftrack object."""
    h, w = np.asarray(frames[0]).shape
    tracker = oftrack(bsize, w, h, th_flowvalid_ratio, th_flowvalid_abs)
    pyrs = [Pyramid(np.asarray(f, np.float32), lv_f, psz, True) for f in frames]
    for k in range(len(frames) - 1):
        of_forw = dense_flow(pyrs[k], pyrs[k + 1], step=step, psz=psz, lv_f=lv_f)
        of_back = dense_flow(pyrs[k + 1], pyrs[k], step=step, psz=psz, lv_f=lv_f)
        corners = good_features(frames[k], maxcorners, 0.001, 5)
        tracker.addframe(of_forw, of_back, corners if len(corners) else None)
    if savefile is not None:
        tracker.savetofile(savefile)
    return tracker


# ---------------------------------------------------------------- the same stages on the device (ictr_frontend.hip)
def good_features_hip(img, maxcorners=1000, quality=0.001, mindist=5, win=3):
    """good_features on the device (``ictr_good_features``): same arguments, same (K,2) float32 result in the same order.
    img: a host image, or a Pyramid whose level 0 is the image. The host function sums its windows through an integral
    image, the device sums them directly; the two agree wherever the integral image is exact (integer-valued frames).
    No CPU fallback: raises IctrError without a GPU."""
    out = np.empty((int(maxcorners), 2), np.float32)
    n = C.c_int(0)
    L = _lib.load()
    if isinstance(img, Pyramid):
        check(L.ictr_good_features(img._h, None, 0, 0, int(maxcorners), float(quality), int(mindist), int(win), fp(out),
                                   C.byref(n)))
    else:
        img = _lib.f32c(img)
        if img.ndim != 2:
            raise ValueError("img must be (H, W)")
        check(L.ictr_good_features(None, fp(img), img.shape[1], img.shape[0], int(maxcorners), float(quality),
                                   int(mindist), int(win), fp(out), C.byref(n)))
    return out[:n.value].copy()


class FlowGrid:
    """One direction of one frame pair on a `step` grid (``ictr_flowgrid_*``): the node displacements of dense_flow
    after its fill, kept on the device. ``gather`` moves points by the dense field without forming it; ``dense``
    materialises it for callers that write .flo files."""

    def __init__(self, w, h, step=4):
        self._h = C.c_void_p()
        check(_lib.load().ictr_flowgrid_create(C.byref(self._h), int(w), int(h), int(step)))
        self.w, self.h, self.step = int(w), int(h), int(step)
        nx, ny = C.c_int(), C.c_int()
        check(_lib.load().ictr_flowgrid_dims(self._h, C.byref(nx), C.byref(ny)))
        self.nx, self.ny = nx.value, ny.value

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.load().ictr_flowgrid_destroy(self._h)
            self._h = None

    def compute(self, pyr_a, pyr_b, psz=15, lv_f=None, maxiter=10, eps=0.01, stream=None):
        """Track the nodes A -> B (k_patchflow), d = out - pts, fill the lost nodes. Enqueued, no host wait."""
        lv_f = pyr_a.lv_f if lv_f is None else lv_f
        check(_lib.load().ictr_flowgrid_compute(self._h, pyr_a._h, pyr_b._h, int(psz), int(lv_f), int(maxiter),
                                                float(eps), C.c_void_p(stream or 0)))
        return self

    def compute_x(self, pyr_a, pyr_b, psz=15, lv_f=None, maxiter=10, eps=0.01, stream=None):
        """compute for a rectified stereo pair: the nodes are tracked along x only (k_patchdisp); every y displacement
        of the grid is +0.0. The field equals dense_disparity's. Enqueued, no host wait."""
        lv_f = pyr_a.lv_f if lv_f is None else lv_f
        check(_lib.load().ictr_flowgrid_compute_x(self._h, pyr_a._h, pyr_b._h, int(psz), int(lv_f), int(maxiter),
                                                  float(eps), C.c_void_p(stream or 0)))
        return self

    def set_nodes(self, d, lost):
        """Inject node displacements d (ny, nx, 2) and the lost mask (ny, nx); the fill runs on them."""
        d = _lib.f32c(d)
        lost = np.ascontiguousarray(lost, np.uint8)
        if d.shape != (self.ny, self.nx, 2) or lost.shape != (self.ny, self.nx):
            raise ValueError(f"set_nodes needs d ({self.ny}, {self.nx}, 2) and lost ({self.ny}, {self.nx})")
        check(_lib.load().ictr_flowgrid_set_nodes(self._h, fp(d), lost.ctypes.data_as(_lib.U8P)))
        return self

    def nodes(self):
        """(d after the fill (ny, nx, 2) float32, lost mask (ny, nx) bool)."""
        d = np.empty((self.ny, self.nx, 2), np.float32)
        lost = np.empty((self.ny, self.nx), np.uint8)
        check(_lib.load().ictr_flowgrid_nodes(self._h, fp(d), lost.ctypes.data_as(_lib.U8P)))
        return d, lost.astype(bool)

    def gather(self, xy):
        """func_get_transf_position(xy, F[:, :, 0], F[:, :, 1]) with F = dense(), bit for bit, without forming F."""
        xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        out = np.empty_like(xy)
        check(_lib.load().ictr_flowgrid_gather(self._h, _lib.dp(xy), xy.shape[0], _lib.dp(out)))
        return out

    def dense(self, out=None, on_device=False):
        """The (H, W, 2) float32 field of dense_flow. on_device: `out` is a device pointer that receives it."""
        if on_device:
            check(_lib.load().ictr_flowgrid_dense(self._h, C.c_void_p(out), 1))
            return out
        if out is None:
            out = np.empty((self.h, self.w, 2), np.float32)
        check(_lib.load().ictr_flowgrid_dense(self._h, out.ctypes.data_as(C.c_void_p), 0))
        return out


class PointTracker:
    """The loop of run_OF_point_track on the device (``ictr_pointtrack_*``): push the frames one by one, read the
    oftrack object back when it is wanted. Device memory is a ring of bsize block slots; blocks that left the window
    wait in a host store of the object."""

    def __init__(self, w, h, bsize=10, maxcorners=1000, lv_f=3, psz=15, step=4, maxiter=10, eps=0.01, quality=0.001,
                 mindist=5, win=3, th_flowvalid_ratio=0.2, th_flowvalid_abs=1.0):
        self._h = C.c_void_p()
        check(_lib.load().ictr_pointtrack_create(C.byref(self._h), int(w), int(h), int(bsize), int(maxcorners), int(lv_f),
                                                 int(psz), int(step), int(maxiter), float(eps), float(quality),
                                                 int(mindist), int(win), float(th_flowvalid_ratio),
                                                 float(th_flowvalid_abs)))
        self.w, self.h, self.bsize, self.maxcorners = int(w), int(h), int(bsize), int(maxcorners)
        self.th_flowvalid_ratio, self.th_flowvalid_abs = th_flowvalid_ratio, th_flowvalid_abs

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.load().ictr_pointtrack_destroy(self._h)
            self._h = None

    def push_frame(self, img):
        img = _lib.f32c(img)
        if img.shape != (self.h, self.w):
            raise ValueError(f"push_frame needs a {self.w}x{self.h} frame, got {img.shape[1]}x{img.shape[0]}")
        check(_lib.load().ictr_pointtrack_push_frame(self._h, fp(img)))

    @property
    def frcounter(self):
        n = C.c_int64()
        check(_lib.load().ictr_pointtrack_frcounter(self._h, C.byref(n)))
        return int(n.value)

    def read_block(self, b):
        """Block b as addframe holds it before compaction: (tracks (K,2,bsize) f32, valid (K,) bool, absmovement (K,)
        f64), K = its corner count (0: the frame had no corner)."""
        tr = np.empty((self.maxcorners, 2, self.bsize), np.float32)
        va = np.empty(self.maxcorners, np.uint8)
        am = np.empty(self.maxcorners, np.float64)
        n = C.c_int()
        check(_lib.load().ictr_pointtrack_read_block(self._h, int(b), fp(tr), va.ctypes.data_as(_lib.U8P), _lib.dp(am),
                                                     C.byref(n)))
        k = n.value
        return tr[:k].copy(), va[:k].astype(bool), am[:k].copy()

    def tracks(self):
        """The oftrack object that run_OF_point_track would hold now: tracks, tracks_valid, tracks_absmovement,
        frcounter; blocks that left the window compacted, frames without corners as None."""
        o = oftrack(self.bsize, self.w, self.h, self.th_flowvalid_ratio, self.th_flowvalid_abs)
        o.frcounter = self.frcounter
        for b in range(o.frcounter):
            tr, va, am = self.read_block(b)
            if len(tr) == 0:
                tr = va = am = None
            elif b <= o.frcounter - self.bsize:
                live = np.nonzero(va)[0]
                tr, va, am = tr[live], np.ones(len(live), bool), am[live]
            o.tracks.append(tr)
            o.tracks_valid.append(va)
            o.tracks_absmovement.append(am)
        return o


def run_OF_point_track_hip(frames, bsize=10, psz=15, lv_f=3, step=4, maxcorners=1000, th_flowvalid_ratio=0.2,
                           th_flowvalid_abs=1.0, savefile=None):
    """run_OF_point_track with every stage on the device (PointTracker): same parameters, the same oftrack object bit
    for bit on integer-valued frames (where the host corner picker's integral image is exact)."""
    h, w = np.asarray(frames[0]).shape
    pt = PointTracker(w, h, bsize, maxcorners, lv_f, psz, step, 10, 0.01, 0.001, 5, 3, th_flowvalid_ratio,
                      th_flowvalid_abs)
    for f in frames:
        pt.push_frame(f)
    tracker = pt.tracks()
    if savefile is not None:
        tracker.savetofile(savefile)
    return tracker
