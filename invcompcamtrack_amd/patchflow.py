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
           "good_features_hip", "FlowGrid", "PointTracker", "run_OF_point_track_hip", "refine_flow_host", "refine_flow",
           "FlowRefiner", "REFINE_DEFAULTS", "FR_STAGES", "densify_flow_host", "densify_flow", "FlowDensifier",
           "DENSIFY_DEFAULTS", "DZ_STAGES", "c2f_flow_host", "c2f_flow", "CoarseToFineFlow",
           "CoarseToFineFlowSet"]


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


def _grey_only(who, *pyrs):
    """Colour frames (three pyramids per frame) are CoarseToFineFlow(channels=3)'s alone; everything else stays grey."""
    for p in pyrs:
        if isinstance(p, (list, tuple)):
            raise ValueError(f"{who} takes grey frames, one pyramid per frame: colour frames (three pyramids) are "
                             "CoarseToFineFlow(channels=3)'s alone")


def track_points(pyr_a, pyr_b, pts, psz=15, lv_f=None, lv_l=0, maxiter=10, eps=0.01, dist=None, group=None, _local=None):
    """Track K points from frame A to frame B. pts: (K,2) level-0 pixel coordinates (x,y).
    Returns (new_pts (K,2) float32 with NaN rows for lost points, status (K,) bool, iters (K,) int32).

    dist (torch.distributed, initialised; optional `group`): BASELINE config 4's multi-GPU form -- every rank holds both
    frames (its own pyramids on its own GPU) and tracks the contiguous range partition_patches(K, world)[rank] of the K
    patches; rank 0 gathers the ranges in rank order and returns the full arrays, the other ranks return None. The
    result on rank 0 equals the single-process result bit for bit (a patch's arithmetic does not depend on what else
    is in its launch). `_local` replaces the GPU call in the CPU tests of the partition / gather logic."""
    _grey_only("track_points", pyr_a, pyr_b)
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
    _grey_only("track_disparity", pyr_a, pyr_b)
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
    return _dense_from_nodes((new - pts).reshape(len(ys), len(xs), 2), ~ok.reshape(len(ys), len(xs)), w, h, step)


def _dense_from_nodes(d, bad, w, h, step):
    """dense_flow from its node table on: d (ny, nx, 2) float32 (overwritten by the fill), bad (ny, nx) the lost nodes."""
    xs, ys = range(step // 2, w, step), range(step // 2, h, step)
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


# ---------------------------------------------------------------- a dense field on the device: its owner, its sources
def _dense_out(result, handle, w, h, out, on_device):
    """``dense(out, on_device)`` of every object here: ``result`` is its C function (handle, pointer, on_device)."""
    if on_device:
        check(result(handle, C.c_void_p(out), 1))
        return out
    if out is None:
        out = np.empty((h, w, 2), np.float32)
    check(result(handle, out.ctypes.data_as(C.c_void_p), 0))
    return out


class _DenseStage:
    """An object ``ictr_<_C>_*`` that owns an (H, W, 2) float32 result on the device for w x h frames: ``run`` (the
    subclass's) enqueues and returns, ``dense`` and ``stage`` wait. A subclass names its C prefix, its parameters with
    their defaults and its stage planes, and sends the parameters down in ``_set_params``."""
    _C, _DEFAULTS, _STAGES = None, {}, ()

    def __init__(self, w, h, **params):
        unknown = set(params) - set(self._DEFAULTS)
        if unknown:
            raise TypeError(f"{type(self).__name__}: unknown parameter(s) {sorted(unknown)}")
        self._h = C.c_void_p()
        check(self._c("create")(C.byref(self._h), int(w), int(h)))
        self.w, self.h = int(w), int(h)
        self.params = dict(self._DEFAULTS, **params)
        self._set_params()

    def _c(self, name):
        return getattr(_lib.load(), f"ictr_{self._C}_{name}")

    def __del__(self):
        if getattr(self, "_h", None):
            self._c("destroy")(self._h)
            self._h = None

    def dense(self, out=None, on_device=False):
        """The (H, W, 2) float32 result of the last run. on_device: `out` is a device pointer that receives it."""
        return _dense_out(self._c("result"), self._h, self.w, self.h, out, on_device)

    def device_ptr(self):
        return int(self._c("device_ptr")(self._h) or 0)

    def stage(self, name):
        """One (H, W) float32 plane of the last run: a name of the class's stages (FR_STAGES, DZ_STAGES)."""
        out = np.empty((self.h, self.w), np.float32)
        check(self._c("read_stage")(self._h, self._STAGES.index(name), fp(out)))
        return out

    def set_timing(self, on=True):
        check(self._c("set_timing")(self._h, int(bool(on))))


def _device_source(src, w, h, stages):
    """What a field source on the device is, for frames of w x h: (kind, device pointer, the object to keep alive until
    the reader has run, components), or None for anything else (a host array: its rules are the caller's). A FlowGrid
    (FIELD_GRID, its handle; never formed), an object of one of the classes ``stages`` that has run (its result buffer),
    or an object with ``data_ptr()`` (a torch tensor): float32, contiguous, on the GPU where it says where it is, (H, W)
    (FIELD_PLANE, 1 component) or (H, W, 2) (FIELD_FLOW, 2). A wrong size or shape is a ValueError, a wrong dtype,
    layout or residence a TypeError."""
    if isinstance(src, FlowGrid):
        return _lib.FIELD_GRID, src._h.value, src, 2
    if isinstance(src, stages):
        if (src.h, src.w) != (h, w):
            raise ValueError(f"a {type(src).__name__} of {src.w} x {src.h} where the frames are {w} x {h}")
        return _lib.FIELD_FLOW, src.device_ptr(), src, 2
    if not hasattr(src, "data_ptr"):
        return None
    if not str(src.dtype).endswith("float32") or not src.is_contiguous() or not getattr(src, "is_cuda", True):
        raise TypeError("a device field is a contiguous float32 tensor on the GPU")
    shape = tuple(src.shape)
    if shape not in ((h, w), (h, w, 2)):
        raise ValueError(f"a field is ({h}, {w}) or ({h}, {w}, 2), not {shape}")
    return (_lib.FIELD_PLANE if len(shape) == 2 else _lib.FIELD_FLOW), src.data_ptr(), src, len(shape) - 1


# ---------------------------------------------------------------- variational refinement of a dense field
REFINE_DEFAULTS = dict(alpha=16.0, gamma=13.0, delta=4.5, n_outer=8, n_sor=5, omega=1.6)
_FR_EPS, _FR_ZETA = 1e-3, 0.1
FR_STAGES = ("bw", "a11", "a12", "a22", "b1", "b2", "wr", "wd", "du", "dv", "u", "v")  # ictr_flowrefine_read_stage


def _fr_dx(a):
    """(a[x+1] - a[x-1]) / 2, and 0 in the first and last column."""
    out = np.zeros_like(a)
    out[:, 1:-1] = 0.5 * (a[:, 2:] - a[:, :-2])
    return out


def _fr_dy(a):
    out = np.zeros_like(a)
    out[1:-1, :] = 0.5 * (a[2:, :] - a[:-2, :])
    return out


def _fr_warp(B, px, py):
    """Step 1 at given positions: (bilinear(B) at the position clamped to the frame, the inside mask as 0 / 1)."""
    h, w = B.shape
    inside = ((px >= 0) & (px <= w - 1) & (py >= 0) & (py <= h - 1)).astype(B.dtype)
    pxc = np.fmin(np.fmax(px, 0), w - 1)  # fmax / fmin: a NaN position goes to 0, no index depends on it
    pyc = np.fmin(np.fmax(py, 0), h - 1)
    x0 = np.minimum(np.floor(pxc).astype(np.int64), w - 2)
    y0 = np.minimum(np.floor(pyc).astype(np.int64), h - 2)
    fx, fy = pxc - x0, pyc - y0
    bw = (((1 - fx) * (1 - fy)) * B[y0, x0] + (fx * (1 - fy)) * B[y0, x0 + 1] + ((1 - fx) * fy) * B[y0 + 1, x0]
          + (fx * fy) * B[y0 + 1, x0 + 1])
    return bw, inside


def _fr_coef(A, bw, inside, u, v, alpha, gamma, delta):
    """Steps 2-4: a11, a12, a22, b1, b2 and the weights of the edges to the right and down (0 where the edge would leave
    the frame)."""
    e2, z2 = _FR_EPS ** 2, _FR_ZETA ** 2
    Ix, Iy, Iz = _fr_dx(bw), _fr_dy(bw), bw - A
    Ixx, Ixy, Iyy = _fr_dx(Ix), _fr_dy(Ix), _fr_dy(Iy)
    Ixz, Iyz = Ix - _fr_dx(A), Iy - _fr_dy(A)
    n0 = 1 / (Ix * Ix + Iy * Iy + z2)
    w0 = delta * inside * n0 * 0.5 / np.sqrt(n0 * Iz * Iz + e2)
    n1 = 1 / (Ixx * Ixx + Ixy * Ixy + z2)
    n2 = 1 / (Ixy * Ixy + Iyy * Iyy + z2)
    wg = gamma * inside * 0.5 / np.sqrt(n1 * Ixz * Ixz + n2 * Iyz * Iyz + e2)
    a11 = w0 * Ix * Ix + wg * (n1 * Ixx * Ixx + n2 * Ixy * Ixy)
    a12 = w0 * Ix * Iy + wg * (n1 * Ixx * Ixy + n2 * Ixy * Iyy)
    a22 = w0 * Iy * Iy + wg * (n1 * Ixy * Ixy + n2 * Iyy * Iyy)
    b1 = -(w0 * Ix * Iz + wg * (n1 * Ixx * Ixz + n2 * Ixy * Iyz))
    b2 = -(w0 * Iy * Iz + wg * (n1 * Ixy * Ixz + n2 * Iyy * Iyz))
    s = alpha * 0.5 / np.sqrt(_fr_dx(u) ** 2 + _fr_dy(u) ** 2 + _fr_dx(v) ** 2 + _fr_dy(v) ** 2 + e2)
    wr, wd = np.zeros_like(s), np.zeros_like(s)
    wr[:, :-1] = 0.5 * (s[:, :-1] + s[:, 1:])
    wd[:-1, :] = 0.5 * (s[:-1, :] + s[1:, :])
    return a11, a12, a22, b1, b2, wr, wd


def _fr_coef_rgb(A, bw, inside, u, v, alpha, gamma, delta):
    """_fr_coef on colour frames: A, bw are three planes each. Steps 1 and 2 run per channel, n0_c, n1_c, n2_c are per
    channel; the two robust weights are joint over the channels and taken on the channel mean,
    q0 = delta inside / 2 / sqrt((1/3) sum_c n0_c Iz_c^2 + eps^2),
    qg = gamma inside / 2 / sqrt((1/3) sum_c (n1_c Ixz_c^2 + n2_c Iyz_c^2) + eps^2); the coefficients are channel means,
    a11 = (1/3) sum_c [q0 n0_c Ix_c^2 + qg (n1_c Ixx_c^2 + n2_c Ixy_c^2)] and a12, a22, b1, b2 likewise. Three equal
    channels give _fr_coef in real arithmetic. The smoothness term is unchanged."""
    e2, z2 = _FR_EPS ** 2, _FR_ZETA ** 2
    ch = []
    for c in range(3):
        Ix, Iy, Iz = _fr_dx(bw[c]), _fr_dy(bw[c]), bw[c] - A[c]
        Ixx, Ixy, Iyy = _fr_dx(Ix), _fr_dy(Ix), _fr_dy(Iy)
        Ixz, Iyz = Ix - _fr_dx(A[c]), Iy - _fr_dy(A[c])
        n0 = 1 / (Ix * Ix + Iy * Iy + z2)
        n1 = 1 / (Ixx * Ixx + Ixy * Ixy + z2)
        n2 = 1 / (Ixy * Ixy + Iyy * Iyy + z2)
        ch.append((Ix, Iy, Iz, Ixx, Ixy, Iyy, Ixz, Iyz, n0, n1, n2))
    q0 = delta * inside * 0.5 / np.sqrt(sum(n0 * Iz * Iz for (_, _, Iz, _, _, _, _, _, n0, _, _) in ch) / 3 + e2)
    qg = gamma * inside * 0.5 / np.sqrt(
        sum(n1 * Ixz * Ixz + n2 * Iyz * Iyz for (_, _, _, _, _, _, Ixz, Iyz, _, n1, n2) in ch) / 3 + e2)
    a11 = a12 = a22 = b1 = b2 = 0.0
    for Ix, Iy, Iz, Ixx, Ixy, Iyy, Ixz, Iyz, n0, n1, n2 in ch:
        a11 = a11 + (q0 * n0 * Ix * Ix + qg * (n1 * Ixx * Ixx + n2 * Ixy * Ixy))
        a12 = a12 + (q0 * n0 * Ix * Iy + qg * (n1 * Ixx * Ixy + n2 * Ixy * Iyy))
        a22 = a22 + (q0 * n0 * Iy * Iy + qg * (n1 * Ixy * Ixy + n2 * Iyy * Iyy))
        b1 = b1 + (q0 * n0 * Ix * Iz + qg * (n1 * Ixx * Ixz + n2 * Ixy * Iyz))
        b2 = b2 + (q0 * n0 * Iy * Iz + qg * (n1 * Ixy * Ixz + n2 * Iyy * Iyz))
    s = alpha * 0.5 / np.sqrt(_fr_dx(u) ** 2 + _fr_dy(u) ** 2 + _fr_dx(v) ** 2 + _fr_dy(v) ** 2 + e2)
    wr, wd = np.zeros_like(s), np.zeros_like(s)
    wr[:, :-1] = 0.5 * (s[:, :-1] + s[:, 1:])
    wd[:-1, :] = 0.5 * (s[:-1, :] + s[1:, :])
    return a11 / 3, a12 / 3, a22 / 3, -b1 / 3, -b2 / 3, wr, wd


def _fr_shift(a):
    """The four neighbours' values (left, right, up, down), 0 beyond the frame (where the edge weight is 0 too)."""
    p = np.pad(a, 1)
    return p[1:-1, :-2], p[1:-1, 2:], p[:-2, 1:-1], p[2:, 1:-1]


def _fr_half_sweep(colour, omega, x_only, u, v, du, dv, a11, a12, a22, b1, b2, wr, wd):
    """Step 5, one colour, in place on du / dv."""
    h, w = u.shape
    yy, xx = np.mgrid[0:h, 0:w]
    m = ((xx + yy) & 1) == colour
    wl, wu = _fr_shift(wr)[0], _fr_shift(wd)[2]
    sw = wl + wr + wu + wd
    ul, ur, uu, ud = _fr_shift(u + du)
    su = wl * ul + wr * ur + wu * uu + wd * ud
    dun = (1 - omega) * du + omega * (b1 - a12 * dv + su - sw * u) / (a11 + sw)
    du[m] = dun[m]
    if x_only:
        return
    vl, vr, vu, vd = _fr_shift(v + dv)
    sv = wl * vl + wr * vr + wu * vu + wd * vd
    dvn = (1 - omega) * dv + omega * (b2 - a12 * du + sv - sw * v) / (a22 + sw)
    dv[m] = dvn[m]


def refine_flow_host(img_a, img_b, flow, alpha=16.0, gamma=13.0, delta=4.5, n_outer=8, n_sor=5, omega=1.6, x_only=False,
                     _trace=None):
    """Variational refinement of the dense flow A -> B at level 0: the definition (build-defined; NumPy, f64 arithmetic
    on the f32 inputs; DESIGN.md §4 "Variational refinement of a dense field" states the rule). img_a, img_b: (H, W) grey
    frames, or three (H, W) planes each for colour frames (the joint robust weights of _fr_coef_rgb; "bw" in _trace is
    then (3, H, W)); flow: (H, W, 2). Returns (H, W, 2) float32. x_only (a stereo pair): only u moves, v keeps its input bits.
    n_outer = 0 returns the input's bits. _trace: a list that receives one dict of the stage planes per outer iteration
    (FR_STAGES' names, and "px", "py", the warp positions)."""
    f0 = np.ascontiguousarray(flow, np.float32)
    A = np.asarray(np.asarray(img_a, np.float32), np.float64)
    B = np.asarray(np.asarray(img_b, np.float32), np.float64)
    rgb = A.ndim == 3  # colour frames: three (H, W) planes each (DESIGN.md §4 "Colour"; _fr_coef_rgb states the rule)
    if rgb and (A.shape[0] != 3 or B.shape != A.shape):
        raise ValueError("refine_flow_host: colour frames are three (H, W) planes each")
    h, w = A.shape[-2:]
    if B.shape != A.shape or f0.shape != (h, w, 2) or w < 4 or h < 4:
        raise ValueError("refine_flow_host needs two (H, W) frames and an (H, W, 2) flow, H, W >= 4")
    if not (0 < omega < 2) or not alpha > 0 or min(gamma, delta, n_outer, n_sor) < 0:
        raise ValueError("refine_flow_host: negative parameter, alpha <= 0, or omega outside (0, 2)")
    if n_outer == 0:
        return f0.copy()
    u, v = f0[..., 0].astype(np.float64), f0[..., 1].astype(np.float64)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(n_outer):
        px, py = xx + u, yy + v
        if rgb:
            warped = [_fr_warp(B[c], px, py) for c in range(3)]
            bw, inside = np.stack([q[0] for q in warped]), warped[0][1]
            a11, a12, a22, b1, b2, wr, wd = _fr_coef_rgb(A, bw, inside, u, v, alpha, gamma, delta)
        else:
            bw, inside = _fr_warp(B, px, py)
            a11, a12, a22, b1, b2, wr, wd = _fr_coef(A, bw, inside, u, v, alpha, gamma, delta)
        du, dv = np.zeros_like(u), np.zeros_like(v)
        for _k in range(n_sor):
            for colour in (0, 1):
                _fr_half_sweep(colour, omega, x_only, u, v, du, dv, a11, a12, a22, b1, b2, wr, wd)
        if _trace is not None:
            _trace.append(dict(bw=bw, a11=a11, a12=a12, a22=a22, b1=b1, b2=b2, wr=wr, wd=wd, du=du.copy(), dv=dv.copy(),
                               u=u.copy(), v=v.copy(), px=px, py=py))
        u, v = u + du, v + dv
    out = np.empty((h, w, 2), np.float32)
    out[..., 0] = u
    out[..., 1] = f0[..., 1] if x_only else v
    return out


class FlowRefiner(_DenseStage):
    """refine_flow_host on the device (``ictr_flowrefine_*``) for w x h frames; parameters as REFINE_DEFAULTS. ``run``
    enqueues and returns; ``dense`` (the refined field) waits. ``stage``: a plane of the last outer iteration. The object
    is a device ICTR_FIELD_FLOW for the stereo track window."""
    _C, _DEFAULTS, _STAGES = "flowrefine", REFINE_DEFAULTS, FR_STAGES

    def _set_params(self):
        p = self.params
        check(self._c("set_params")(self._h, float(p["alpha"]), float(p["gamma"]), float(p["delta"]), int(p["n_outer"]),
                                    int(p["n_sor"]), float(p["omega"])))

    def _source(self, src):
        """-> (the _lib.Field of `src`, what must stay alive until ictr_flowrefine_run has returned)"""
        f = _lib.Field(kind=_lib.FIELD_FLOW, sign=1, on_device=0, x_only=0, data=None)
        dev = _device_source(src, self.w, self.h, (FlowDensifier, CoarseToFineFlow))
        if dev is None:
            keep = _lib.f32c(src)
            if keep.shape != (self.h, self.w, 2):
                raise ValueError(f"FlowRefiner.run needs an ({self.h}, {self.w}, 2) field, got {keep.shape}")
            f.data = keep.ctypes.data
            return f, keep
        f.kind, f.data, keep, components = dev
        if components != 2:
            raise ValueError(f"FlowRefiner.run needs a ({self.h}, {self.w}, 2) device field, not a plane")
        f.on_device = int(f.kind != _lib.FIELD_GRID)
        return f, keep

    def run(self, pyr_a, pyr_b, src, x_only=False, stream=None):
        """src: an (H, W, 2) host array (checked for finiteness, copied now), a FlowGrid that holds a field, a
        FlowDensifier or CoarseToFineFlow that has run (its buffer on the device, read when the run executes: run it on the
        same stream), or a
        device tensor / object with ``data_ptr()`` holding (H, W, 2) float32 (read when the run executes)."""
        _grey_only("FlowRefiner.run", pyr_a, pyr_b)
        f, _keep = self._source(src)
        check(self._c("run")(self._h, pyr_a._h, pyr_b._h, C.byref(f), int(bool(x_only)), C.c_void_p(stream or 0)))
        return self

    def _write_stage(self, name, plane):
        plane = _lib.f32c(plane)
        if plane.shape != (self.h, self.w):
            raise ValueError(f"a stage plane is ({self.h}, {self.w})")
        check(_lib.load().ictr_debug_flowrefine_write_stage(self._h, FR_STAGES.index(name), fp(plane)))

    def _half_sweep(self, colour, x_only=False):
        check(_lib.load().ictr_debug_flowrefine_half_sweep(self._h, int(colour), int(bool(x_only))))

    def kernel_ms(self):
        """(k_fr_warp, k_fr_coef, k_fr_sor, k_fr_init + k_fr_final) of the last run in ms; zeros when timing was off."""
        ms = np.zeros(4, np.float32)
        check(self._c("get_kernel_times")(self._h, fp(ms)))
        return ms


def refine_flow(pyr_a, pyr_b, flow, x_only=False, **params):
    """refine_flow_host's result from the device: host arrays in and out, one FlowRefiner for the call."""
    flow = _lib.f32c(flow)
    return FlowRefiner(pyr_a.w, pyr_a.h, **params).run(pyr_a, pyr_b, flow, x_only=x_only).dense()


# ---------------------------------------------------------------- photometric densification of a flow grid
DENSIFY_DEFAULTS = dict(minerr=2.0, power=1)
DZ_STAGES = ("count", "wsum")  # ictr_flowdensify_read_stage
DZ_MAX_PSZ = 32


def _dz_nodes(n_px, n_nodes, step, psz):
    """Per pixel coordinate 0 .. n_px - 1: (first, last) node index along the axis whose footprint covers it; a node at
    X = step // 2 + i step covers X - (psz - psz // 2) .. X + psz // 2 - 1, the pixels k_patchflow samples at an integer
    centre. last < first: no node."""
    x = np.arange(n_px)
    lo, hi, half = psz - psz // 2, psz // 2 - 1, step // 2
    first = np.maximum(-((-(x - hi - half)) // step), 0)
    last = np.minimum((x + lo - half) // step, n_nodes - 1)
    return first, last


def _dz_power(m, power):
    m2 = m * m
    return m if power == 1 else m2 if power == 2 else m2 * m if power == 3 else m2 * m2


def _dz_check(img_a, img_b, d, lost, step, psz, minerr, power):
    A, B = np.asarray(img_a, np.float32), np.asarray(img_b, np.float32)
    h, w = A.shape if A.ndim == 2 else (0, 0)
    if B.shape != A.shape or A.ndim != 2 or w < 2 or h < 2:
        raise ValueError("densify needs two (H, W) frames, H, W >= 2")
    if int(step) != step or step < 1 or step // 2 >= min(w, h):
        raise ValueError("densify: the grid needs a step >= 1 and at least one node")
    nx, ny = len(range(step // 2, w, step)), len(range(step // 2, h, step))
    d = np.ascontiguousarray(d, np.float32)
    lost = np.asarray(lost).astype(bool)
    if d.shape != (ny, nx, 2) or lost.shape != (ny, nx):
        raise ValueError(f"densify needs d ({ny}, {nx}, 2) and lost ({ny}, {nx})")
    if int(psz) != psz or not 1 <= psz <= DZ_MAX_PSZ:
        raise ValueError(f"densify: psz is 1 .. {DZ_MAX_PSZ}")
    if not (np.isfinite(minerr) and minerr > 0) or int(power) != power or not 1 <= power <= 4:
        raise ValueError("densify: minerr is finite and positive, power an integer 1 .. 4")
    return A, B, d, lost


def densify_flow_host(img_a, img_b, d, lost, step, psz, minerr=2.0, power=1, _stages=None, bias=None):
    """Photometric densification of a flow grid A -> B at level 0: the definition (build-defined; NumPy, f64 arithmetic on
    the f32 inputs; DESIGN.md §4 "Densification of a flow grid" states the rule). img_a, img_b: (H, W) grey frames; d
    (ny, nx, 2), lost (ny, nx): the node table of a grid of `step` (nodes at step // 2 + k step) tracked with patches of
    psz. Every pixel takes sum(wgt d) / sum(wgt) over the nodes that are not lost and whose patch covers it (_dz_nodes), in
    ascending node row, then column: a vote whose position (x, y) + d is not inside the frame is dropped; otherwise
    wgt = 1 / max(|Bw - A[y, x]|, minerr)^power with Bw by refine_flow_host's warp (_fr_warp). A pixel without a vote
    takes dense_flow's value. The sums are plain f64 sums of exact products, the quotient is rounded to f32 once.
    bias: an (ny, nx) array of per-node brightness offsets beta (the coarse-to-fine flow's node bias under patch-mean
    normalisation); the weight is then 1 / max(|Bw - A[y, x] - beta_node|, minerr)^power. None: the operations above.
    Colour frames (DESIGN.md §4 "Colour"): img_a, img_b are three (H, W) planes each and bias is None or (ny, nx, 3), one
    offset per channel. A vote warps the three channels of B at its one position, with one inside decision, and its weight
    is 1 / max(e, minerr)^power with e = (1/3) sum_c |Bw_c - A_c[y, x] - beta_c|: the channel mean, so that minerr keeps
    its meaning in grey levels. (The sum starts at 0.0 and adds the channels in order; for one channel 0.0 + |res| and the
    quotient by 1.0 are exact, so a grey frame's e is |res| to the bit.)
    Returns (H, W, 2) float32. _stages: a dict that receives "count" (votes taken, int), "wsum" (their summed weight,
    f64) and "edge" (the least distance of a pixel's vote positions to the inside boundary in px, inf without one)."""
    A32, B32 = np.asarray(img_a, np.float32), np.asarray(img_b, np.float32)
    colour = A32.ndim == 3
    if colour and (A32.shape[0] != 3 or B32.shape != A32.shape):
        raise ValueError("densify: colour frames are three (H, W) planes each")
    _, _, d, lost = _dz_check(A32[0] if colour else A32, B32[0] if colour else B32, d, lost, step, psz, minerr, power)
    h, w = A32.shape[-2:]
    A, B = A32.astype(np.float64).reshape(-1, h, w), B32.astype(np.float64).reshape(-1, h, w)
    nch = len(A)
    ny, nx = lost.shape
    i0, i1 = _dz_nodes(w, nx, step, psz)
    j0, j1 = _dz_nodes(h, ny, step, psz)
    d64 = d.astype(np.float64)
    if bias is not None:
        bias = np.asarray(bias, np.float64)
        if bias.shape != ((ny, nx, 3) if colour else (ny, nx)):
            raise ValueError(f"densify needs bias ({ny}, {nx}, 3)" if colour else f"densify needs bias ({ny}, {nx})")
        bias = bias.reshape(ny, nx, nch)
    yy, xx = np.mgrid[0:h, 0:w]
    su, sv, sw = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
    cnt = np.zeros((h, w), np.int64)
    edge = np.full((h, w), np.inf)
    for a in range(max(int((j1 - j0).max()) + 1, 0)):
        j, vj = np.minimum(j0 + a, ny - 1), j0 + a <= j1
        for b in range(max(int((i1 - i0).max()) + 1, 0)):
            i, vi = np.minimum(i0 + b, nx - 1), i0 + b <= i1
            votes = vj[:, None] & vi[None, :] & ~lost[j][:, i]
            dx, dy = d64[j][:, i, 0], d64[j][:, i, 1]
            px, py = xx + dx, yy + dy
            with np.errstate(invalid="ignore"):
                e = 0.0
                for c in range(nch):
                    bw, inside = _fr_warp(B[c], px, py)
                    res = bw - A[c] if bias is None else bw - A[c] - bias[j][:, i, c]
                    e = e + np.abs(res)
                e = e / float(nch)
                near = np.minimum(np.minimum(np.abs(px), np.abs(px - (w - 1))), np.minimum(np.abs(py), np.abs(py - (h - 1))))
                edge = np.where(votes & (near < edge), near, edge)
                ok = votes & (inside > 0)
                wgt = 1.0 / _dz_power(np.fmax(e, float(minerr)), power)
                su, sv, sw = np.where(ok, su + wgt * dx, su), np.where(ok, sv + wgt * dy, sv), np.where(ok, sw + wgt, sw)
            cnt += ok
    out = _dense_from_nodes(d.copy(), lost, w, h, step)
    with np.errstate(invalid="ignore", divide="ignore"):
        out[..., 0] = np.where(cnt > 0, su / sw, out[..., 0])
        out[..., 1] = np.where(cnt > 0, sv / sw, out[..., 1])
    if _stages is not None:
        _stages.update(count=cnt, wsum=sw, edge=edge)
    return out


class FlowDensifier(_DenseStage):
    """densify_flow_host on the device (``ictr_flowdensify_*``, one k_densify launch per field) for w x h frames;
    parameters as DENSIFY_DEFAULTS. ``run`` enqueues and returns; ``dense`` (the densified field) waits. The object is a
    device ICTR_FIELD_FLOW for FlowRefiner.run and for the stereo track window."""
    _C, _DEFAULTS, _STAGES = "flowdensify", DENSIFY_DEFAULTS, DZ_STAGES

    def _set_params(self):
        if int(self.params["power"]) != self.params["power"]:
            raise ValueError("FlowDensifier: power is an integer 1 .. 4")
        check(self._c("set_params")(self._h, float(self.params["minerr"]), int(self.params["power"])))

    def run(self, grid, pyr_a, pyr_b, psz=15, stream=None):
        """grid: a FlowGrid of the object's size that holds a field, tracked A -> B with patches of psz."""
        if not isinstance(grid, FlowGrid):
            raise TypeError("FlowDensifier.run needs a FlowGrid")
        _grey_only("FlowDensifier.run", pyr_a, pyr_b)
        check(self._c("run")(self._h, grid._h, pyr_a._h, pyr_b._h, int(psz), C.c_void_p(stream or 0)))
        return self

    def kernel_ms(self):
        """k_densify of the last run in ms; 0 when timing was off."""
        ms = np.zeros(1, np.float32)
        check(self._c("get_kernel_ms")(self._h, fp(ms)))
        return float(ms[0])


def densify_flow(pyr_a, pyr_b, grid, psz, **params):
    """densify_flow_host's result from the device: a FlowGrid in, a host array out, one FlowDensifier for the call."""
    return FlowDensifier(pyr_a.w, pyr_a.h, **params).run(grid, pyr_a, pyr_b, psz).dense()


# ---------------------------------------------------------------- coarse-to-fine dense flow
C2F_LOST, C2F_TRACKED, C2F_HELD_COND, C2F_HELD_VIEW, C2F_HELD_FAR = range(5)  # ICTR_C2F_*, a node's status byte


def _c2f_level_size(pyr, l):
    return pyr.img[l].shape[1] - 2 * pyr.pad, pyr.img[l].shape[0] - 2 * pyr.pad


def _c2f_sample(plane, pad, psz, x, y):
    """The (psz, psz) patch k_patchflow samples at the centre (x, y) of a plane padded by pad >= psz, in f64: taps
    (floor, floor + 1) both ways, weights from x - floor(x), y - floor(y)."""
    v = plane[pad - psz:, pad - psz:]
    fx, fy = np.floor(x), np.floor(y)
    r0, r1 = x - fx, y - fy
    row, col = int(fy) + 1 + psz // 2, int(fx) + 1 + psz // 2
    a, b = v[row:row + psz, col:col + psz], v[row:row + psz, col - 1:col - 1 + psz]
    c, d = v[row - 1:row - 1 + psz, col:col + psz], v[row - 1:row - 1 + psz, col - 1:col - 1 + psz]
    return ((r0 * r1) * a.astype(np.float64) + ((1 - r0) * r1) * b + (r0 * (1 - r1)) * c) + ((1 - r0) * (1 - r1)) * d


def _c2f_init(coarse, w, h, step, x_only=False):
    """Step 2 of c2f_flow_host: (ny, nx, 2) float32 starts of a level's nodes from the coarser level's field (None: the
    coarsest level, zeros). Nearest neighbour at (min(X >> 1, w' - 1), min(Y >> 1, h' - 1)), times 2: exact in f32.
    x_only: the y component of the coarser field is not read, and a start's y is +0.0."""
    xs, ys = np.arange(step // 2, w, step), np.arange(step // 2, h, step)
    if coarse is None:
        return np.zeros((len(ys), len(xs), 2), np.float32)
    coarse = np.asarray(coarse, np.float32)
    ch, cw = coarse.shape[:2]
    init = np.float32(2) * coarse[np.minimum(ys >> 1, ch - 1)][:, np.minimum(xs >> 1, cw - 1)]
    if x_only:
        init[..., 1] = np.float32(0)
    return init


def _c2f_channels(pyr):
    """A frame's pyramids as a list: one for a grey frame (a pyramid), three for a colour frame (a sequence of three)."""
    if hasattr(pyr, "img"):
        return [pyr]
    pyrs = list(pyr)
    if len(pyrs) != 3:
        raise ValueError(f"c2f flow: a colour frame is three pyramids, one per channel, not {len(pyrs)}")
    return pyrs


def _csum(vals):
    """The sum over the channels in their order (one channel: its value, untouched)."""
    s = vals[0]
    for v in vals[1:]:
        s = s + v
    return s


C2F_COST_L2, C2F_COST_HUBER = 0, 2  # ICTR_C2F_COST_*: the cost field of OF_DIS's parameter string as remembered (1 is L1)


def _c2f_cost(cost, huber_k, who="c2f flow"):
    """(ICTR_C2F_COST_* code, huber_k as a float) of the keywords cost ("l2" | "huber", or the code 0 | 2) and huber_k
    (finite and > 0, checked for both costs); ValueError otherwise, for L1 with the reason."""
    if cost in ("l1", "L1") or (not isinstance(cost, str) and cost == 1):
        raise ValueError(f"{who}: cost L1 (code 1) is not built: with H fixed its influence sign(r) has no scale; "
                         "use cost='huber' with a small huber_k")
    if isinstance(cost, str):
        code = {"l2": C2F_COST_L2, "huber": C2F_COST_HUBER}.get(cost)
    else:
        code = cost if cost in (C2F_COST_L2, C2F_COST_HUBER) and int(cost) == cost else None
    if code is None:
        raise ValueError(f"{who}: cost is {cost!r} ('l2' or 'huber')")
    try:
        k = float(huber_k)
    except (TypeError, ValueError):
        k = float("nan")
    if not (np.isfinite(k) and k > 0):
        raise ValueError(f"{who}: huber_k is {huber_k!r}; it must be finite and > 0")
    return int(code), k


def _c2f_clip(r, huber_k, clipped=None):
    """The Huber cost's residual: r clipped to [-huber_k, +huber_k] (the derivative of the Huber loss); None: r (L2).
    clipped: a two-item list that counts the residuals the clip changed and all residuals."""
    if huber_k is None:
        return r
    if clipped is not None:
        clipped[0] += int((np.abs(r) > huber_k).sum())
        clipped[1] += r.size
    return np.clip(r, -huber_k, huber_k)


def _c2f_search_host(pyr_a, pyr_b, l, init, step, psz, maxiter, eps, min_det, patnorm=False, huber_k=None, _clipped=None):
    """Step 3 of c2f_flow_host at level l from the starts `init` (ny, nx, 2) float32. patnorm: patch-mean normalisation,
    T <- T - mean(T) once and r = T - (I - mean(I)) in every iteration, nothing else changed. huber_k (None: the L2 cost):
    the Huber patch cost (DESIGN.md "Robust patch cost"), every pixel's and channel's residual r <- clip(r, -huber_k,
    +huber_k) in every iteration, after the means are removed under patnorm; T, Gx, Gy, H, the conditioning decision, the
    view tests, the step, the eps stop and the rejection are unchanged. _clipped: _c2f_clip's counter. A colour frame (three
    pyramids per frame, DESIGN.md "Colour"): T_c, Gx_c, Gy_c are sampled per channel, H = sum_c sum_px G_c G_c^T and
    b = sum_c sum_px G_c r_c with r_c = T_c - I_c (patnorm: each channel less its own means), one conditioning decision
    and one step per node; nothing else changes. Returns (d (ny, nx, 2) float32
    before the fill (NaN at a lost node), status (ny, nx) uint8, margins): margins is a dict of (ny, nx) f64 arrays, the
    least distance of a node's decisions from their thresholds (inf where the decision was not taken):
      "eps"   | |step| - eps | over the steps taken, in px
      "view"  distance of a tested position from the border it is tested against, in px
      "far"   | |p - init| - psz | at the rejection test, in px
      "det"   | det / tr^2 - min_det |"""
    pas, pbs = _c2f_channels(pyr_a), _c2f_channels(pyr_b)
    w, h = _c2f_level_size(pas[0], l)
    xs, ys = np.arange(step // 2, w, step), np.arange(step // 2, h, step)
    ny, nx = len(ys), len(xs)
    d = np.full((ny, nx, 2), np.nan, np.float32)
    status = np.zeros((ny, nx), np.uint8)
    m = {k: np.full((ny, nx), np.inf) for k in ("eps", "view", "far", "det")}

    def in_view(j, i, x, y):
        with np.errstate(invalid="ignore"):
            near = np.min(np.abs(np.array([x, y, x - w, y - h], np.float64)))
        if np.isfinite(near):
            m["view"][j, i] = min(m["view"][j, i], near)
        return bool(0 <= x <= w and 0 <= y <= h)

    for j, Y in enumerate(ys):
        for i, X in enumerate(xs):
            i0 = init[j, i].astype(np.float64)
            if not (np.isfinite(i0).all() and in_view(j, i, X + i0[0], Y + i0[1])):
                continue  # lost
            d[j, i] = init[j, i]
            T = [_c2f_sample(q.img[l], q.pad, psz, float(X), float(Y)) for q in pas]
            Gx = [_c2f_sample(q.dx[l], q.pad, psz, float(X), float(Y)) for q in pas]
            Gy = [_c2f_sample(q.dy[l], q.pad, psz, float(X), float(Y)) for q in pas]
            hxx, hxy, hyy = (_csum([(gx * gx).sum() for gx in Gx]), _csum([(gx * gy).sum() for gx, gy in zip(Gx, Gy)]),
                             _csum([(gy * gy).sum() for gy in Gy]))
            det, tr = hxx * hyy - hxy * hxy, hxx + hyy
            if tr > 0:
                m["det"][j, i] = abs(det / (tr * tr) - min_det)
            if not (det > min_det * tr * tr) or not (tr > 0):
                status[j, i] = C2F_HELD_COND
                continue
            if patnorm:
                T = [t - t.mean() for t in T]
            p = i0.copy()
            st = C2F_TRACKED
            for _ in range(maxiter):
                cx, cy = X + p[0], Y + p[1]
                if not in_view(j, i, cx, cy):
                    st = C2F_HELD_VIEW
                    break
                I = [_c2f_sample(q.img[l], q.pad, psz, cx, cy) for q in pbs]
                r = [_c2f_clip(t - (v - v.mean()) if patnorm else t - v, huber_k, _clipped) for t, v in zip(T, I)]
                bx, by = _csum([(g * e).sum() for g, e in zip(Gx, r)]), _csum([(g * e).sum() for g, e in zip(Gy, r)])
                dx, dy = (hyy * bx - hxy * by) / det, (hxx * by - hxy * bx) / det
                p += (dx, dy)
                n = np.hypot(dx, dy)
                m["eps"][j, i] = min(m["eps"][j, i], abs(n - eps))
                if n * n < eps * eps:
                    break
            if st == C2F_TRACKED:
                far = np.hypot(p[0] - i0[0], p[1] - i0[1])
                if np.isfinite(far):
                    m["far"][j, i] = abs(far - psz)
                if not (far * far <= psz * psz):
                    st = C2F_HELD_FAR
            status[j, i] = st
            if st == C2F_TRACKED:
                d[j, i] = p
    return d, status, m


def _c2f_search_x_host(pyr_a, pyr_b, l, init, step, psz, maxiter, eps, min_hx, patnorm=False, huber_k=None,
                       _clipped=None):
    """Step 3 of c2f_flow_host(x_only=True) at level l from the starts `init` (ny, nx, 2) float32 whose y is +0.0: the
    1-D rule of k_patchdisp at this level alone. hxx = sum Gx^2, hyy = sum Gy^2, tr = hxx + hyy; the node is held by
    conditioning iff not tr > 0 or not hxx > min_hx tr; an iteration tests the view at (X + p, Y), samples I there, takes
    dx = sum Gx (T - I) / hxx (patnorm: T - mean(T) and I - mean(I)), p += dx, and stops when dx^2 < eps^2; the rejection
    is not (p - init.x)^2 <= psz^2. y never moves: d = (p, +0.0) when tracked, (init.x, +0.0) when held. Returns what
    _c2f_search_host returns; margins["det"] is | hxx / tr - min_hx |, "eps" | |dx| - eps |, "far" | |p - init.x| - psz |.
    Colour frames (three pyramids per frame): hxx, hyy and sum Gx r are summed over the channels, as in _c2f_search_host.
    huber_k: the Huber patch cost, every residual clipped to [-huber_k, +huber_k] as in _c2f_search_host."""
    pas, pbs = _c2f_channels(pyr_a), _c2f_channels(pyr_b)
    w, h = _c2f_level_size(pas[0], l)
    xs, ys = np.arange(step // 2, w, step), np.arange(step // 2, h, step)
    ny, nx = len(ys), len(xs)
    d = np.full((ny, nx, 2), np.nan, np.float32)
    status = np.zeros((ny, nx), np.uint8)
    m = {k: np.full((ny, nx), np.inf) for k in ("eps", "view", "far", "det")}

    def in_view(j, i, x):
        near = min(abs(x), abs(x - w)) if np.isfinite(x) else np.inf
        if np.isfinite(near):
            m["view"][j, i] = min(m["view"][j, i], near)
        return bool(0 <= x <= w)

    for j, Y in enumerate(ys):
        for i, X in enumerate(xs):
            ix = float(init[j, i, 0])
            if not (np.isfinite(ix) and in_view(j, i, X + ix)):
                continue  # lost
            d[j, i] = (init[j, i, 0], np.float32(0))
            T = [_c2f_sample(q.img[l], q.pad, psz, float(X), float(Y)) for q in pas]
            Gx = [_c2f_sample(q.dx[l], q.pad, psz, float(X), float(Y)) for q in pas]
            Gy = [_c2f_sample(q.dy[l], q.pad, psz, float(X), float(Y)) for q in pas]
            hxx, hyy = _csum([(gx * gx).sum() for gx in Gx]), _csum([(gy * gy).sum() for gy in Gy])
            tr = hxx + hyy
            if tr > 0:
                m["det"][j, i] = abs(hxx / tr - min_hx)
            if not (tr > 0) or not (hxx > min_hx * tr):
                status[j, i] = C2F_HELD_COND
                continue
            if patnorm:
                T = [t - t.mean() for t in T]
            p = ix
            st = C2F_TRACKED
            for _ in range(maxiter):
                if not in_view(j, i, X + p):
                    st = C2F_HELD_VIEW
                    break
                I = [_c2f_sample(q.img[l], q.pad, psz, X + p, float(Y)) for q in pbs]
                r = [_c2f_clip(t - (v - v.mean()) if patnorm else t - v, huber_k, _clipped) for t, v in zip(T, I)]
                dx = _csum([(g * e).sum() for g, e in zip(Gx, r)]) / hxx
                p += dx
                m["eps"][j, i] = min(m["eps"][j, i], abs(abs(dx) - eps))
                if dx * dx < eps * eps:
                    break
            if st == C2F_TRACKED:
                far = abs(p - ix)
                if np.isfinite(far):
                    m["far"][j, i] = abs(far - psz)
                if not (far * far <= psz * psz):
                    st = C2F_HELD_FAR
            status[j, i] = st
            if st == C2F_TRACKED:
                d[j, i, 0] = p
    return d, status, m


def _c2f_bias_host(pyr_a, pyr_b, l, d, status, step, psz, margins=None):
    """The node bias of c2f_flow_host under patnorm at level l: (ny, nx) f64. A node with status != 0 has a final float32
    d (a tracked node's p, a held node's init); where its final position (X, Y) + d passes the search's view test,
    beta = mean(patch of B there) - mean(patch of A at (X, Y)), both sampled as the search samples them. Every other
    node has beta = 0: a tracked node may end up to psz out of view, and no tap then leaves a plane padded by psz.
    margins: _c2f_search_host's dict; the distance of this view decision from its border joins "view".
    Colour frames (three pyramids per frame): (ny, nx, 3), one offset per channel, at the same nodes."""
    pas, pbs = _c2f_channels(pyr_a), _c2f_channels(pyr_b)
    w, h = _c2f_level_size(pas[0], l)
    xs, ys = np.arange(step // 2, w, step), np.arange(step // 2, h, step)
    beta = np.zeros((len(ys), len(xs)) if len(pas) == 1 else (len(ys), len(xs), len(pas)))
    for j, Y in enumerate(ys):
        for i, X in enumerate(xs):
            if status[j, i] == C2F_LOST:
                continue
            x, y = X + float(d[j, i, 0]), Y + float(d[j, i, 1])
            near = min(abs(x), abs(y), abs(x - w), abs(y - h))
            if margins is not None and np.isfinite(near):
                margins["view"][j, i] = min(margins["view"][j, i], near)
            if not (0 <= x <= w and 0 <= y <= h):
                continue
            if len(pas) == 1:
                beta[j, i] = (_c2f_sample(pbs[0].img[l], pbs[0].pad, psz, x, y).mean()
                              - _c2f_sample(pas[0].img[l], pas[0].pad, psz, float(X), float(Y)).mean())
            else:
                for c, (qa, qb) in enumerate(zip(pas, pbs)):
                    beta[j, i, c] = (_c2f_sample(qb.img[l], qb.pad, psz, x, y).mean()
                                     - _c2f_sample(qa.img[l], qa.pad, psz, float(X), float(Y)).mean())
    return beta


def _c2f_check(pyr_a, pyr_b, step, psz, lv_f, refine, lv_l=0):
    if int(psz) != psz or not 1 <= psz <= 32:
        raise ValueError("c2f flow: psz is 1 .. 32")
    if int(step) != step or step < 1:
        raise ValueError("c2f flow: step is an integer >= 1")
    if pyr_a.pad < psz or pyr_b.pad < psz:
        raise ValueError(f"c2f flow: pyramid padding must be >= psz ({psz})")
    have = min(len(pyr_a.img), len(pyr_b.img)) - 1
    lv_f = have if lv_f is None else int(lv_f)
    if not 0 <= lv_f <= have:
        raise ValueError(f"c2f flow: lv_f is {lv_f}, the pyramids have levels 0 .. {have}")
    if refine is not None and not dict(REFINE_DEFAULTS, **refine)["alpha"] > 0:
        raise ValueError("c2f flow: the refinement needs alpha > 0")
    if int(lv_l) != lv_l or not 0 <= lv_l <= lv_f:
        raise ValueError(f"c2f flow: lv_l is {lv_l} (0 .. lv_f = {lv_f})")
    for l in range(int(lv_l), lv_f + 1):
        w, h = _c2f_level_size(pyr_a, l)
        if _c2f_level_size(pyr_b, l) != (w, h):
            raise ValueError(f"c2f flow: the two pyramids differ in size at level {l}")
        if w < 2 or h < 2:
            raise ValueError(f"c2f flow: level {l} is {w} x {h}, smaller than 2 px")
        if step // 2 >= w or step // 2 >= h:
            raise ValueError(f"c2f flow: level {l} ({w} x {h}) has no node at step {step}")
        if refine is not None and (w < 4 or h < 4):
            raise ValueError(f"c2f flow: level {l} is {w} x {h}, the refinement needs 4 x 4")
    return lv_f


def _c2f_plane(pyr, l):
    p = pyr.pad
    return np.ascontiguousarray(pyr.img[l][p:pyr.img[l].shape[0] - p, p:pyr.img[l].shape[1] - p])


def pyramid_level_size(w, h, lv):
    """(w_l, h_l) of level lv of a w x h pyramid: lv halvings, each rounded half to even (cvRound(v * 0.5))."""
    def half(v):
        q = v // 2
        return q if v % 2 == 0 or q % 2 == 0 else q + 1
    for _ in range(int(lv)):
        w, h = half(w), half(h)
    return w, h


def _upsample_check(field, w, h, lv):
    field = np.asarray(field)
    if int(lv) != lv or not 1 <= lv <= 15:
        raise ValueError(f"upsample_flow: lv is {lv} (1 .. 15)")
    if int(w) != w or int(h) != h or w < 1 or h < 1:
        raise ValueError("upsample_flow: w, h are integers >= 1")
    wl, hl = pyramid_level_size(int(w), int(h), int(lv))
    if wl < 1 or hl < 1:
        raise ValueError(f"upsample_flow: level {lv} of {w} x {h} is empty")
    if field.shape != (hl, wl, 2):
        raise ValueError(f"upsample_flow: the field is {field.shape}, level {lv} of {w} x {h} is ({hl}, {wl}, 2)")
    return np.ascontiguousarray(field, np.float32), wl, hl


def _upsample_taps(n, nl, s):
    """(i0, i1, r) of the n output positions along an axis whose level has nl samples: f64, every value exact."""
    f = np.clip((np.arange(n, dtype=np.float64) + 0.5) / s - 0.5, 0.0, nl - 1.0)
    i0 = np.floor(f).astype(np.int64)
    return i0, np.minimum(i0 + 1, nl - 1), f - i0


def upsample_flow_host(field, w, h, lv, x_only=False):
    """The field (h_l, w_l, 2) of level lv (1 .. 15) of a w x h pyramid at the frame's size: the definition (build-defined;
    f64 arithmetic on the f32 taps, rounded to f32 once; DESIGN.md §4 "A finest level above 0"). (w_l, h_l) must be
    pyramid_level_size(w, h, lv), else ValueError. With s = 2^lv, output pixel (x, y): fx = clamp((x + 0.5) / s - 0.5, 0,
    w_l - 1), x0 = floor(fx), x1 = min(x0 + 1, w_l - 1), rx = fx - x0, and fy, y0, y1, ry alike with h_l; per component
    top = (1 - rx) F[y0, x0] + rx F[y0, x1], bot = (1 - rx) F[y1, x0] + rx F[y1, x1], val = (1 - ry) top + ry bot, and the
    output is s val. These are cv::resize(INTER_LINEAR)'s half-pixel centres at the fixed factor 2^-lv (not w_l / w: odd
    halving makes w_l s larger or smaller than w, and the clamp takes care of the last columns and rows), and the
    vectors times s. x_only: the y component of `field` is not read, and the output's y is +0.0 to the bit."""
    F, wl, hl = _upsample_check(field, w, h, lv)
    s = float(1 << int(lv))
    x0, x1, rx = _upsample_taps(int(w), wl, s)
    y0, y1, ry = _upsample_taps(int(h), hl, s)
    rx, ry = rx[None, :], ry[:, None]
    out = np.zeros((int(h), int(w), 2), np.float32)
    for k in range(1 if x_only else 2):
        P = F[..., k].astype(np.float64)
        top = (1 - rx) * P[y0][:, x0] + rx * P[y0][:, x1]
        bot = (1 - rx) * P[y1][:, x0] + rx * P[y1][:, x1]
        out[..., k] = s * ((1 - ry) * top + ry * bot)
    return out


def upsample_flow(field, w, h, lv, x_only=False):
    """upsample_flow_host's result from the device (k_flow_upsample through ``ictr_flow_upsample``): a host array in, a
    host array (h, w, 2) float32 out; the call waits. The same size checks."""
    F, wl, hl = _upsample_check(field, w, h, lv)
    out = np.empty((int(h), int(w), 2), np.float32)
    check(_lib.load().ictr_flow_upsample(fp(F), wl, hl, int(lv), fp(out), int(w), int(h), int(bool(x_only)), 0, None))
    return out


def c2f_flow_host(pyr_a, pyr_b, step=4, psz=8, lv_f=None, maxiter=10, eps=0.01, min_det=1e-4, densify=None, refine=None,
                  _stages=None, patnorm=False, x_only=False, min_hx=1e-2, lv_l=0, cost="l2", huber_k=5.0):
    """Coarse-to-fine dense flow A -> B: the definition (build-defined; NumPy, f64 arithmetic on the f32 planes; DESIGN.md
    §4 "Coarse-to-fine dense flow" states the rule). pyr_a, pyr_b: host pyramids with ``.img / .dx / .dy[l]`` padded by
    ``.pad >= psz`` (oracle.Pyramid's shape). For l = lv_f .. 0: nodes at step // 2 + k step of the level's own size; a
    node starts at init = 2 U_{l+1}[min(Y >> 1, h' - 1), min(X >> 1, w' - 1)] ((0, 0) at lv_f); the search runs at this
    level only with k_patchflow's sampling, H, step and stopping rule from p = init and ends in a status (C2F_*): 0 lost
    (the start is out of view or not finite: no vote, filled from its neighbours), 1 tracked (d = p), 2 held by the
    conditioning test, 3 held because it left the view while iterating, 4 held because |p - init| > psz (or not finite);
    a held node keeps d = init, bit for bit, and votes. U_l = densify_flow_host(A_l, B_l, d, lost, step, psz, **densify),
    then with `refine` a dict U_l = refine_flow_host(A_l, B_l, U_l, **refine). Returns U_0 (H, W, 2) float32.
    patnorm: patch-mean normalisation, for frames whose brightness differs by a locally constant offset. The search
    removes the patch means (_c2f_search_host), every node gets its brightness offset beta (_c2f_bias_host), and the
    densifier's vote of a node weighs |Bw - A - beta| (densify_flow_host's bias). The refinement is unchanged: its
    brightness term still sees the offset.
    x_only: the 1-D form for a rectified stereo pair (DESIGN.md "The 1-D form"). A node starts from the x component of
    the coarser field alone, the search is _c2f_search_x_host (k_patchdisp's rule at the level, conditioning by min_hx; a
    held node's status values keep their meaning), the densifier is called unchanged on the table whose y is +0.0, and
    the refinement is refine_flow_host(..., x_only=True). Every level's field has +0.0 bits in its y component. It
    combines with patnorm, whose bias is taken at (X + d.x, Y).
    lv_l (0 .. lv_f; DESIGN.md "A finest level above 0"): the levels lv_f .. lv_l run as above (a level's field does not
    depend on finer levels), and the result is upsample_flow_host(U_lv_l, W, H, lv_l, x_only). With lv_l = 0 nothing is
    up-sampled. The size rules hold for the levels lv_l .. lv_f.
    Colour (DESIGN.md "Colour"): pyr_a and pyr_b are each a sequence of THREE pyramids, one per channel, equal in size,
    levels and padding. The nodes, the starts, the view tests, the eps stop, the rejection, the status values, the fill
    and the up-sampling are unchanged; the search sums H and b over the channels and takes one decision and one step per
    node (_c2f_search_host), the node bias under patnorm is (ny, nx, 3), one offset per channel (_c2f_bias_host), and a
    vote weighs the channel mean of the absolute residuals (densify_flow_host on three planes). Three equal channels
    give the grey rule in real arithmetic. The refinement takes the three planes per frame: its steps 1 and 2 run per
    channel and its two robust weights are joint over the channels (refine_flow_host, _fr_coef_rgb).
    cost ("l2", the default, or "huber"; DESIGN.md "Robust patch cost"): with "huber" the search clips every pixel's and
    channel's residual of every iteration to [-huber_k, +huber_k] (huber_k in grey levels on the frames' own scale, finite
    and > 0; its default 5.0 is a choice, not a measurement), after the patch means are removed under patnorm. That is
    the derivative of the Huber loss with H left as the template's. T, Gx, Gy, H, the conditioning decision, the view
    tests, the step, the eps stop, the rejection, the status values, the node bias, the densifier and the refinement are
    unchanged. L1 (OF_DIS's cost code 1) is refused: with H fixed its influence sign(r) has no scale.
    _stages: a list that receives one dict per level from lv_f down: "level", "init", "d" (after the fill), "status",
    "margins" (_c2f_search_host's), "field" (U_l), "bias" (the node bias, None without patnorm) and "clipped" (with
    cost="huber": the count of residuals the clip changed and of all residuals of the level's iterations)."""
    code, huber_k = _c2f_cost(cost, huber_k, "c2f_flow_host")
    hk = huber_k if code == C2F_COST_HUBER else None
    pas, pbs = _c2f_channels(pyr_a), _c2f_channels(pyr_b)
    if len(pas) != len(pbs):
        raise ValueError("c2f flow: one frame is grey and the other colour")
    if len(pas) == 3:
        geo = [[(q.pad, len(q.img)) + tuple(i.shape for i in q.img) for q in qs] for qs in (pas, pbs)]
        if any(g != gs[0] for gs in geo for g in gs):
            raise ValueError("c2f flow: the three pyramids of a frame differ in geometry")
    lv_f = _c2f_check(pas[0], pbs[0], step, psz, lv_f, refine, lv_l)
    lv_l = int(lv_l)
    U = None
    for l in range(lv_f, lv_l - 1, -1):
        w, h = _c2f_level_size(pas[0], l)
        init = _c2f_init(U, w, h, step, x_only)
        clipped = [0, 0]
        if x_only:
            d, status, margins = _c2f_search_x_host(pyr_a, pyr_b, l, init, step, psz, maxiter, eps, min_hx, patnorm, hk,
                                                    clipped)
        else:
            d, status, margins = _c2f_search_host(pyr_a, pyr_b, l, init, step, psz, maxiter, eps, min_det, patnorm, hk,
                                                  clipped)
        lost = status == C2F_LOST
        bias = _c2f_bias_host(pyr_a, pyr_b, l, d, status, step, psz, margins) if patnorm else None
        A, B = _c2f_plane(pas[0], l), _c2f_plane(pbs[0], l)
        if len(pas) == 3:
            A, B = np.stack([_c2f_plane(q, l) for q in pas]), np.stack([_c2f_plane(q, l) for q in pbs])
        U = densify_flow_host(A, B, np.where(lost[..., None], np.float32(0), d), lost, step, psz, bias=bias,
                              **(densify or {}))
        if refine is not None:
            U = refine_flow_host(A, B, U, x_only=bool(x_only), **refine)
        if _stages is not None:
            filled = d.copy()
            _dense_from_nodes(filled, lost, w, h, step)
            _stages.append(dict(level=l, init=init, d=filled, status=status, margins=margins, field=U, bias=bias,
                                clipped=tuple(clipped) if hk is not None else None))
    if lv_l > 0:
        w0, h0 = _c2f_level_size(pas[0], 0)
        return upsample_flow_host(U, w0, h0, lv_l, bool(x_only))
    return U


class CoarseToFineFlow:
    """c2f_flow_host on the device (``ictr_c2fflow_*``: k_c2f_level, the grid's fill, k_densify and optionally the
    refinement per level) for w x h frames and levels lv_f .. 0. densify / refine: the per-level parameters
    (DENSIFY_DEFAULTS' / REFINE_DEFAULTS' names; refine=None: no refinement). patnorm: c2f_flow_host's patch-mean
    normalisation (k_c2f_level's MEAN forms with the node bias, k_densify<true>). x_only: c2f_flow_host's 1-D form for a
    rectified stereo pair (k_c2f_level's XONLY forms, the refinement along x; v is +0.0 at every level). lv_l:
    c2f_flow_host's finest level (default 0); above 0 only the levels lv_f .. lv_l exist and run, and a run ends with
    k_flow_upsample from level lv_l's field into the object's w x h result plane, which ``dense`` and ``device_ptr`` then
    hand out. channels: 1 (grey frames, one pyramid each) or 3 (colour frames, c2f_flow_host's rule on triples: ``run``
    then takes two sequences of three pyramids, k_c2f_level's, k_densify's and k_fr_warp's NCH = 3 forms and
    k_fr_coef_rgb run, and ``level_bias`` is (ny, nx, 3)). cost, huber_k: c2f_flow_host's patch cost ("huber":
    k_c2f_level's ROBUST forms; ``.cost`` is "l2" or "huber", ``.huber_k`` the float the object holds). ``run`` enqueues and returns; ``dense``
    (the w x h field), ``level`` and ``level_bias`` wait. The object is a device ICTR_FIELD_FLOW wherever a FlowDensifier is one."""

    def __init__(self, w, h, lv_f, step=4, psz=8, maxiter=10, eps=0.01, densify=None, refine=None, patnorm=False,
                 x_only=False, lv_l=0, channels=1, cost="l2", huber_k=5.0):
        dz = dict(DENSIFY_DEFAULTS, **(densify or {}))
        code, huber_k = _c2f_cost(cost, huber_k, "CoarseToFineFlow")
        if channels not in (1, 3):
            raise ValueError(f"CoarseToFineFlow: channels is {channels} (1: grey, or 3: colour)")
        unknown = set(dz) - set(DENSIFY_DEFAULTS) | (set(refine or {}) - set(REFINE_DEFAULTS))
        if unknown:
            raise TypeError(f"CoarseToFineFlow: unknown parameter(s) {sorted(unknown)}")
        if int(dz["power"]) != dz["power"]:
            raise ValueError("CoarseToFineFlow: power is an integer 1 .. 4")
        L = _lib.load()
        self._h = C.c_void_p()
        if int(lv_l) != lv_l:
            raise ValueError("CoarseToFineFlow: lv_l is an integer 0 .. lv_f")
        check(L.ictr_c2fflow_create_lvl(C.byref(self._h), int(w), int(h), int(lv_f), int(lv_l), int(step), int(psz)))
        self.w, self.h, self.lv_f, self.step, self.psz = int(w), int(h), int(lv_f), int(step), int(psz)
        self.lv_l = int(lv_l)
        self.params = dict(maxiter=int(maxiter), eps=float(eps), densify=dz,
                           refine=None if refine is None else dict(REFINE_DEFAULTS, **refine))
        check(L.ictr_c2fflow_set_params(self._h, int(maxiter), float(eps), float(dz["minerr"]), int(dz["power"])))
        if refine is not None:
            r = self.params["refine"]
            check(L.ictr_c2fflow_set_refine(self._h, 1, float(r["alpha"]), float(r["gamma"]), float(r["delta"]),
                                            int(r["n_outer"]), int(r["n_sor"]), float(r["omega"])))
        self.patnorm = bool(patnorm)
        if self.patnorm:
            check(L.ictr_c2fflow_set_patnorm(self._h, 1))
        self.x_only = bool(x_only)
        if self.x_only:
            check(L.ictr_c2fflow_set_x_only(self._h, 1))
        self.channels = int(channels)
        if self.channels != 1:
            check(L.ictr_c2fflow_set_channels(self._h, self.channels))
        if code != C2F_COST_L2:  # (an L2 object makes the calls it made before the cost existed)
            check(L.ictr_c2fflow_set_cost(self._h, code, huber_k))

    @property
    def cost(self):
        return "huber" if self._get_cost()[0] == C2F_COST_HUBER else "l2"

    @property
    def huber_k(self):
        return self._get_cost()[1]

    def _get_cost(self):
        code, k = C.c_int(), C.c_float()
        check(_lib.load().ictr_c2fflow_get_cost(self._h, C.byref(code), C.byref(k)))
        return int(code.value), float(k.value)

    def set_cost(self, cost="l2", huber_k=5.0):
        """The patch cost of the runs that follow; a refused call leaves the object as it was."""
        code, k = _c2f_cost(cost, huber_k, "CoarseToFineFlow.set_cost")
        check(_lib.load().ictr_c2fflow_set_cost(self._h, code, k))

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.load().ictr_c2fflow_destroy(self._h)
            self._h = None

    def run(self, pyr_a, pyr_b, stream=None):
        """channels == 3: pyr_a and pyr_b are each a sequence of three device pyramids, one per channel."""
        if self.channels == 3:
            trip = []
            for p in (pyr_a, pyr_b):
                if hasattr(p, "_h") or len(p) != 3:
                    raise ValueError("CoarseToFineFlow.run: with channels=3 a frame is three pyramids, one per channel")
                trip.append((C.c_void_p * 3)(*[q._h.value for q in p]))
            check(_lib.load().ictr_c2fflow_run_rgb(self._h, trip[0], trip[1], C.c_void_p(stream or 0)))
            return self
        if not hasattr(pyr_a, "_h") or not hasattr(pyr_b, "_h"):
            raise ValueError("CoarseToFineFlow.run: with channels=1 a frame is one pyramid (colour needs channels=3)")
        check(_lib.load().ictr_c2fflow_run(self._h, pyr_a._h, pyr_b._h, C.c_void_p(stream or 0)))
        return self

    def dense(self, out=None, on_device=False):
        """The (H, W, 2) float32 field of the last run. on_device: `out` is a device pointer that receives it."""
        return _dense_out(_lib.load().ictr_c2fflow_result, self._h, self.w, self.h, out, on_device)

    def device_ptr(self):
        return int(_lib.load().ictr_c2fflow_device_ptr(self._h) or 0)

    def level_dims(self, l):
        """(w, h, nx, ny) of level l."""
        v = [C.c_int() for _ in range(4)]
        check(_lib.load().ictr_c2fflow_level_dims(self._h, int(l), *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def level(self, l):
        """Level l of the last run: (field (h_l, w_l, 2) float32, d after the fill (ny, nx, 2) float32, status (ny, nx)
        uint8)."""
        w, h, nx, ny = self.level_dims(l)
        field, d = np.empty((h, w, 2), np.float32), np.empty((ny, nx, 2), np.float32)
        status = np.empty((ny, nx), np.uint8)
        check(_lib.load().ictr_c2fflow_read_level(self._h, int(l), fp(field), fp(d), status.ctypes.data_as(_lib.U8P)))
        return field, d, status

    def level_bias(self, l):
        """The node bias (ny, nx) float32 of level l of the last run, (ny, nx, 3) with channels=3; patnorm only."""
        _, _, nx, ny = self.level_dims(l)
        if self.channels == 3:
            bias = np.empty((ny, nx, 3), np.float32)
            check(_lib.load().ictr_c2fflow_read_level_bias_rgb(self._h, int(l), fp(bias)))
            return bias
        bias = np.empty((ny, nx), np.float32)
        check(_lib.load().ictr_c2fflow_read_level_bias(self._h, int(l), fp(bias)))
        return bias

    def set_timing(self, on=True):
        check(_lib.load().ictr_c2fflow_set_timing(self._h, int(bool(on))))

    def kernel_ms(self):
        """(lv_f + 1, 3) ms of the last run: per level from 0 the search with its fill, the densification, the refinement;
        zeros when timing was off, and in the rows below lv_l."""
        ms = np.zeros((self.lv_f + 1, 3), np.float32)
        check(_lib.load().ictr_c2fflow_get_kernel_ms(self._h, fp(ms)))
        return ms

    def upsample_ms(self):
        """ms of k_flow_upsample in the last run; 0 when timing was off or lv_l = 0."""
        ms = C.c_float()
        check(_lib.load().ictr_c2fflow_get_upsample_ms(self._h, C.byref(ms)))
        return float(ms.value)


C2FSET_MAX = 8  # ICTR_C2FSET_MAX


class CoarseToFineFlowSet:
    """1 .. 8 CoarseToFineFlow objects of equal shape and parameters run in lockstep (``ictr_c2fset_*``): per level and
    stage one launch covers all members, the member index a grid dimension. ``run(pairs)`` leaves every member in the
    state its own ``run(*pairs[m])`` would have left it in, bit for bit (``dense``, ``level``, ``level_bias``,
    ``device_ptr``); only the stage times are the set's (``kernel_ms``), a member's are zeros after a lockstep run. The
    set keeps its members alive. Members are compared at every run: they may be reconfigured between runs, together."""

    def __init__(self, flows):
        flows = list(flows)
        if not 1 <= len(flows) <= C2FSET_MAX:
            raise ValueError(f"CoarseToFineFlowSet: {len(flows)} members (1 .. {C2FSET_MAX})")
        for i, f in enumerate(flows):
            if not isinstance(f, CoarseToFineFlow):
                raise TypeError(f"CoarseToFineFlowSet: member {i} is a {type(f).__name__}, not a CoarseToFineFlow")
            if any(f is g for g in flows[:i]):
                raise ValueError(f"CoarseToFineFlowSet: member {i} is the same object as member "
                                 f"{[g is f for g in flows].index(True)}")
        self.members = tuple(flows)
        self._h = C.c_void_p()
        arr = (C.c_void_p * len(flows))(*[f._h.value for f in flows])
        check(_lib.load().ictr_c2fset_create(C.byref(self._h), arr, len(flows)))

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.load().ictr_c2fset_destroy(self._h)
            self._h = None

    def __len__(self):
        n = C.c_int()
        check(_lib.load().ictr_c2fset_size(self._h, C.byref(n)))
        return int(n.value)

    def run(self, pairs, stream=None):
        """pairs: one (pyr_a, pyr_b) per member; with colour members each of the two is a sequence of three pyramids.
        Two members may read the same pyramid. Enqueues and returns."""
        pairs = list(pairs)
        n, nch = len(self.members), self.members[0].channels
        if len(pairs) != n:
            raise ValueError(f"CoarseToFineFlowSet.run: {len(pairs)} pairs for {n} members")
        tabs = ([], [])
        for m, pair in enumerate(pairs):
            if hasattr(pair, "_h") or len(pair) != 2:
                raise ValueError(f"CoarseToFineFlowSet.run: pair {m} is not a (pyr_a, pyr_b)")
            for tab, p in zip(tabs, pair):
                if nch == 3:
                    if hasattr(p, "_h") or len(p) != 3:
                        raise ValueError(f"CoarseToFineFlowSet.run: pair {m}: with channels=3 a frame is three pyramids, "
                                         "one per channel")
                    tab.extend(q._h.value for q in p)
                else:
                    if not hasattr(p, "_h"):
                        raise ValueError(f"CoarseToFineFlowSet.run: pair {m}: with channels=1 a frame is one pyramid "
                                         "(colour needs channels=3)")
                    tab.append(p._h.value)
        a, b = ((C.c_void_p * len(t))(*t) for t in tabs)
        fn = _lib.load().ictr_c2fset_run_rgb if nch == 3 else _lib.load().ictr_c2fset_run
        check(fn(self._h, a, b, C.c_void_p(stream or 0)))
        return self

    def operations(self):
        """Kernel launches plus memsets the last run enqueued: the same for any number of members."""
        n = C.c_int()
        check(_lib.load().ictr_c2fset_last_operations(self._h, C.byref(n)))
        return int(n.value)

    def set_timing(self, on=True):
        check(_lib.load().ictr_c2fset_set_timing(self._h, int(bool(on))))

    def kernel_ms(self):
        """(lv_f + 1, 3) ms of the last run, each for the whole set: per level from 0 the search with its fill, the
        densification, the refinement; zeros when timing was off, and in the rows below lv_l."""
        ms = np.zeros((self.members[0].lv_f + 1, 3), np.float32)
        check(_lib.load().ictr_c2fset_get_kernel_ms(self._h, fp(ms), None))
        return ms

    def upsample_ms(self):
        """ms of the lockstep k_flow_upsample in the last run; 0 when timing was off or lv_l = 0."""
        ms, up = np.zeros((self.members[0].lv_f + 1, 3), np.float32), C.c_float()
        check(_lib.load().ictr_c2fset_get_kernel_ms(self._h, fp(ms), C.byref(up)))
        return float(up.value)


def c2f_flow(pyr_a, pyr_b, step=4, psz=8, lv_f=None, **params):
    """c2f_flow_host's result from the device: device pyramids in, a host array out, one CoarseToFineFlow for the call
    (params: its keywords, patnorm, x_only, lv_l, cost and huber_k among them)."""
    first = pyr_a if hasattr(pyr_a, "_h") else pyr_a[0]
    if first is not pyr_a:
        params.setdefault("channels", 3)
    lv_f = first.lv_f if lv_f is None else lv_f
    return CoarseToFineFlow(first.w, first.h, lv_f, step, psz, **params).run(pyr_a, pyr_b).dense()


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
        _grey_only("FlowGrid.compute", pyr_a, pyr_b)
        lv_f = pyr_a.lv_f if lv_f is None else lv_f
        check(_lib.load().ictr_flowgrid_compute(self._h, pyr_a._h, pyr_b._h, int(psz), int(lv_f), int(maxiter),
                                                float(eps), C.c_void_p(stream or 0)))
        return self

    def compute_x(self, pyr_a, pyr_b, psz=15, lv_f=None, maxiter=10, eps=0.01, stream=None):
        """compute for a rectified stereo pair: the nodes are tracked along x only (k_patchdisp); every y displacement
        of the grid is +0.0. The field equals dense_disparity's. Enqueued, no host wait."""
        _grey_only("FlowGrid.compute_x", pyr_a, pyr_b)
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
        return _dense_out(_lib.load().ictr_flowgrid_dense, self._h, self.w, self.h, out, on_device)


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
        if img.ndim == 3:
            raise ValueError("PointTracker.push_frame takes grey (h, w) frames: colour frames are "
                             "CoarseToFineFlow(channels=3)'s alone")
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
