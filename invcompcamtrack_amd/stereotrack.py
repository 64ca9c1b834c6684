"""The checked stereo track window of a sequence (misc_src/run_test_OF_track.py:170-223).

Every start point (by default every pixel of the first left frame) is sent to the right frame through the disparity and
checked back, then carried frame by frame through the left and the right flow; eight consistency tests run per frame, a
point that fails once loses its whole row, the survivors are compacted in start order into the script's block
``xy_t (M, 4, bsize)`` = left x, y and right x, y per frame, which fsplit.pairs_from_stereo_tracks and
camfit.observations_from_stereo_tracks read.

  stereo_track_window_host   the definition: the script's lines in NumPy's operation order, float64
  StereoTrackWindow          the same on the device (``ictr_stereotrack_*``), one step's fields resident at a time
  stereo_track_window        the host function's signature on the device
  StereoPointTracker         frames in: pyramids and flow grids per frame, handed to the window as grid fields

The rules, quirks included (DESIGN.md §4 "Stereo track window"):
  gather   func_get_transf_position: four-tap range test (NaN and out-of-range coordinates fail it and give NaN),
           weights w0..w3 = fx fy, (1-fx) fy, fx (1-fy), (1-fx)(1-fy) on the taps (y1,x1), (y1,x0), (y0,x1), (y0,x0), each
           field value widened, multiplied by its weight, summed left to right, added to the coordinate
  frame 0  xy_r = gather(xy_l, -disp_lr[0]) (x only), back = gather(xy_r, disp_rl[0]) (x only); kept when
           |xy_l - back| / |xy_r - xy_l| < th_ratio and |xy_l - back| < th_abs
  frame fr six gathers and eight tests (TESTS below); NaN and x/0 compare false, so a point with zero motion or zero
           disparity is dropped
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import FIELD_FLOW, FIELD_GRID, FIELD_PLANE, check  # FIELD_*: include/ictr.h ICTR_FIELD_*

__all__ = ["stereo_track_window_host", "stereo_track_window", "StereoTrackWindow", "StereoPointTracker", "field", "TESTS",
           "FIELD_PLANE", "FIELD_FLOW", "FIELD_GRID"]

# bits 1-8 of a `reasons` mask, in the script's order (run_test_OF_track.py:208-215); bit 0: a gather of that frame failed
# its range test (or met a NaN). Frame 0 has two tests only: its ratio test is reported as bit 2 and its absolute test as
# bit 6, the tests of the later frames that compare the same pair of positions (left against left-through-right-and-back).
TESTS = ("range", "ratio rf/rf_verif_d", "ratio lf/lf_verif_d", "ratio l/l_verif_f", "ratio r/r_verif_f",
         "abs rf/rf_verif_d", "abs lf/lf_verif_d", "abs l/l_verif_f", "abs r/r_verif_f")


def _gather(xy, du, dv=None):
    """func_get_transf_position(xy, du[, dv]) (run_test_OF_track.py:37-67); xy (N, 2) float64, du / dv (H, W) float64."""
    H, W = du.shape
    fl = np.floor(xy)
    with np.errstate(invalid="ignore"):
        ok = (fl[:, 0] >= 0) & (fl[:, 1] >= 0) & (fl[:, 0] + 1 < W) & (fl[:, 1] + 1 < H)  # NaN fails, as its int cast does
    idx = np.nonzero(ok)[0]
    res = np.full(xy.shape, np.nan)
    res[idx] = xy[idx]
    x0, y0 = fl[idx, 0].astype(np.int64), fl[idx, 1].astype(np.int64)
    x1, y1 = x0 + 1, y0 + 1
    fx, fy = xy[idx, 0] - fl[idx, 0], xy[idx, 1] - fl[idx, 1]
    w0, w1, w2, w3 = fx * fy, (1 - fx) * fy, fx * (1 - fy), (1 - fx) * (1 - fy)
    res[idx, 0] += du[y1, x1] * w0 + du[y1, x0] * w1 + du[y0, x1] * w2 + du[y0, x0] * w3
    if dv is not None:
        res[idx, 1] += dv[y1, x1] * w0 + dv[y1, x0] * w1 + dv[y0, x1] * w2 + dv[y0, x0] * w3
    return res


def _norm(d):
    return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])  # np.linalg.norm(d, axis=1) of a real (N, 2) array


def _f64(a):
    return np.asarray(a, np.float64)


def _start_points(w, h):
    """The script's meshgrid order: x fastest."""
    xs, ys = np.meshgrid(np.arange(w), np.arange(h))
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64)


def _mask_of(positions, tests):
    """reasons mask of one frame: positions = the gathered (N, 2) arrays, tests = [(bit, passed, operand arrays)]."""
    bad = np.zeros(positions[0].shape[0], bool)
    for p in positions:
        bad |= np.isnan(p).any(1)
    mask = bad.astype(np.uint16)
    for bit, passed, ops in tests:
        fin = np.ones(bad.shape, bool)
        for p in ops:
            fin &= ~np.isnan(p).any(1)
        mask |= ((~passed & fin).astype(np.uint16) << bit)
    return mask


def stereo_track_window_host(disp_lr, disp_rl, flow_l, flow_r, xy0=None, th_ratio=0.2, th_abs=1.0, reasons=False):
    """run_test_OF_track.py:170-223 in float64, NumPy's operation order.

    disp_lr[fr], disp_rl[fr]: (H, W) planes (the script's imgs_d[fr][0], imgs_d[fr][1]) for fr = 0 .. bsize-1;
    flow_l[fr], flow_r[fr]: (fwd, bwd) fields (H, W, 2) of the pair fr -> fr+1, the first bsize-1 are read.
    xy0: (N, 2) float64 start points, default every pixel in meshgrid order.
    Returns (xy_t (M, 4, bsize) float64, rows (M,) int64 = the start indices kept); with reasons=True also a dict
    ``frame`` (N,) int32 (the frame a start point was dropped at, -1: kept) and ``mask`` (N,) uint16 (bits of TESTS)."""
    bsize = len(disp_lr)
    if bsize < 1 or len(disp_rl) != bsize:
        raise ValueError("disp_lr and disp_rl need one plane per frame, at least one frame")
    if len(flow_l) < bsize - 1 or len(flow_r) < bsize - 1:
        raise ValueError("flow_l and flow_r need bsize - 1 (fwd, bwd) pairs")
    h, w = np.shape(disp_lr[0])
    xy_l = _start_points(w, h) if xy0 is None else np.array(xy0, np.float64).reshape(-1, 2)
    n = xy_l.shape[0]
    xy_t = np.full((n, 4, bsize), np.nan)
    r_frame = np.full(n, -1, np.int32)
    r_mask = np.zeros(n, np.uint16)
    with np.errstate(invalid="ignore", divide="ignore"):
        xy_r = _gather(xy_l, -_f64(disp_lr[0]))
        back = _gather(xy_r, _f64(disp_rl[0]))
        err, base = _norm(xy_l - back), _norm(xy_r - xy_l)
        t_ratio, t_abs = err / base < th_ratio, err < th_abs
        ok = t_ratio & t_abs
        idx = np.nonzero(ok)[0]
        xy_t[idx, :, 0] = np.hstack((xy_l, xy_r))[idx]
        if reasons:
            m = _mask_of([xy_l, xy_r, back], [(2, t_ratio, (xy_l, xy_r, back)), (6, t_abs, (xy_l, back))])
            r_frame[~ok], r_mask[~ok] = 0, m[~ok]
        for fr in range(1, bsize):
            xy_l, xy_r = xy_t[:, 0:2, fr - 1], xy_t[:, 2:4, fr - 1]
            lf, lb = _f64(flow_l[fr - 1][0]), _f64(flow_l[fr - 1][1])
            rf, rb = _f64(flow_r[fr - 1][0]), _f64(flow_r[fr - 1][1])
            xy_lf = _gather(xy_l, lf[:, :, 0], lf[:, :, 1])
            xy_rf = _gather(xy_r, rf[:, :, 0], rf[:, :, 1])
            xy_rf_verif_d = _gather(xy_lf, -_f64(disp_lr[fr]))
            xy_lf_verif_d = _gather(xy_rf, _f64(disp_rl[fr]))
            xy_l_verif_f = _gather(xy_lf, lb[:, :, 0], lb[:, :, 1])
            xy_r_verif_f = _gather(xy_rf, rb[:, :, 0], rb[:, :, 1])
            e1, e2 = _norm(xy_rf - xy_rf_verif_d), _norm(xy_lf - xy_lf_verif_d)
            e3, e4 = _norm(xy_l - xy_l_verif_f), _norm(xy_r - xy_r_verif_f)
            d12, d3, d4 = _norm(xy_rf - xy_lf), _norm(xy_l - xy_lf), _norm(xy_r - xy_rf)
            t = [e1 / d12 < th_ratio, e2 / d12 < th_ratio, e3 / d3 < th_ratio, e4 / d4 < th_ratio,
                 e1 < th_abs, e2 < th_abs, e3 < th_abs, e4 < th_abs]
            ok = t[0] & t[1] & t[2] & t[3] & t[4] & t[5] & t[6] & t[7]
            if reasons:
                alive = r_frame < 0
                ops = [(xy_rf, xy_rf_verif_d, xy_lf), (xy_lf, xy_lf_verif_d, xy_rf), (xy_l, xy_l_verif_f, xy_lf),
                       (xy_r, xy_r_verif_f, xy_rf), (xy_rf, xy_rf_verif_d), (xy_lf, xy_lf_verif_d), (xy_l, xy_l_verif_f),
                       (xy_r, xy_r_verif_f)]
                m = _mask_of([xy_lf, xy_rf, xy_rf_verif_d, xy_lf_verif_d, xy_l_verif_f, xy_r_verif_f],
                             [(k + 1, t[k], ops[k]) for k in range(8)])
                drop = alive & ~ok
                r_frame[drop], r_mask[drop] = fr, m[drop]
            idx = np.nonzero(ok)[0]
            xy_t[idx, :, fr] = np.hstack((xy_lf, xy_rf))[idx]
            xy_t[np.nonzero(~ok)[0], :, :] = np.nan
    rows = np.nonzero(~np.isnan(xy_t[:, 0, 0]))[0].astype(np.int64)
    out = np.ascontiguousarray(xy_t[rows])
    if reasons:
        return out, rows, dict(frame=r_frame, mask=r_mask)
    return out, rows


# ---------------------------------------------------------------- the device
class field:
    """A displacement field with an exact sign for StereoTrackWindow: ``data`` is a float32 array (H, W) (a plane, moves x
    only) or (H, W, 2) (a flow) in host memory, a torch tensor of one of those shapes on the device, or a FlowGrid (its
    dense field is never formed), or a FlowRefiner or FlowDensifier that has run (its field on the device). float64
    arrays are accepted only where every value is a float32 value. In a stereo slot (lr, rl) a flow or a grid moves x
    only."""

    def __init__(self, data, sign=1):
        if sign not in (1, -1):
            raise ValueError("a field's sign is +1 or -1")
        self.data, self.sign = data, int(sign)


def _exact_f32(a):
    a = np.asarray(a)
    if a.dtype == np.float32:
        return np.ascontiguousarray(a)
    if a.dtype != np.float64:
        raise TypeError(f"a field is float32 (or float32-valued float64), not {a.dtype}")
    b = a.astype(np.float32)
    if not np.array_equal(b.astype(np.float64), a, equal_nan=True):
        raise ValueError("a float64 field with values that float32 cannot hold is refused, not rounded")
    return np.ascontiguousarray(b)


def _descriptor(f, stereo, w, h):
    """-> (_lib.Field, what must stay alive until the step has run)"""
    from .patchflow import CoarseToFineFlow, FlowDensifier, FlowRefiner, _device_source
    f = f if isinstance(f, field) else field(f)
    d = _lib.Field(sign=f.sign, x_only=int(stereo))
    # a grid, a stage's result buffer (read when the step runs, behind its run) or a tensor; else a host array
    dev = _device_source(f.data, w, h, (FlowRefiner, FlowDensifier, CoarseToFineFlow))
    if dev is not None:
        d.kind, d.data, keep, _ = dev
        d.on_device = int(d.kind != FIELD_GRID)
        return d, keep
    keep = _exact_f32(f.data)
    if keep.shape not in ((h, w), (h, w, 2)):
        raise ValueError(f"a field is ({h}, {w}) or ({h}, {w}, 2), not {keep.shape}")
    d.kind, d.data = (FIELD_PLANE if keep.ndim == 2 else FIELD_FLOW), keep.ctypes.data
    return d, keep


class StereoTrackWindow:
    """The window on the device (``ictr_stereotrack_*``): open(lr, rl) with the fields of frame 0, advance(...) once per
    later frame with the pair's four flows and the frame's two stereo fields, then count() and read(). Only one step's
    fields are resident; the state is [bsize][4][N] float64 on the device. ``lr`` is the field that moves a left point to
    the right frame: the script's ``-imgs_d[fr][0]`` is ``field(disp_lr, sign=-1)``, a left -> right FlowGrid is itself."""

    def __init__(self, w, h, bsize, th_ratio=0.2, th_abs=1.0):
        self._h = C.c_void_p()
        check(_lib.load().ictr_stereotrack_create(C.byref(self._h), int(w), int(h), int(bsize), float(th_ratio),
                                                  float(th_abs)))
        self.w, self.h, self.bsize = int(w), int(h), int(bsize)
        self._keep, self._m, self._counted = [], None, None

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.load().ictr_stereotrack_destroy(self._h)
            self._h = None

    def open(self, lr, rl, xy0=None):
        ds = [_descriptor(f, True, self.w, self.h) for f in (lr, rl)]
        self._keep, self._m, self._counted = [k for _, k in ds], None, None
        n, p = 0, None
        if xy0 is not None:
            xy0 = np.ascontiguousarray(xy0, np.float64).reshape(-1, 2)
            n, p = xy0.shape[0], _lib.dp(xy0)
        check(_lib.load().ictr_stereotrack_open(self._h, p, n, C.byref(ds[0][0]), C.byref(ds[1][0])))
        return self

    def advance(self, l_fwd, l_bwd, r_fwd, r_bwd, lr_next, rl_next):
        ds = [_descriptor(f, k >= 4, self.w, self.h) for k, f in enumerate((l_fwd, l_bwd, r_fwd, r_bwd, lr_next, rl_next))]
        self._keep = [k for _, k in ds]  # device fields are read when the step runs; the previous step's are done by then
        check(_lib.load().ictr_stereotrack_advance(self._h, *[C.byref(d) for d, _ in ds]))
        return self

    def count(self):
        m = C.c_int64()
        check(_lib.load().ictr_stereotrack_count(self._h, C.byref(m)))
        self._m = self._counted = int(m.value)
        self._keep = []
        return self._m

    @property
    def survivors(self):
        """M of the counted window (it stays counted through read() and a hand-over), None before count()."""
        return self._counted

    def read(self):
        """(xy_t (M, 4, bsize) float64, rows (M,) int64); count() runs first if it has not."""
        m = self._m if self._m is not None else (self._counted if self._counted is not None else self.count())
        self._m = None
        xy_t = np.empty((m, 4, self.bsize), np.float64)
        rows = np.empty(m, np.int64)
        check(_lib.load().ictr_stereotrack_read(self._h, _lib.dp(xy_t), rows.ctypes.data_as(C.POINTER(C.c_int64))))
        return xy_t, rows

    def set_timing(self, on=True):
        check(_lib.load().ictr_stereotrack_set_timing(self._h, int(on)))

    def kernel_times(self):
        """ms of the last window read: (open and advance kernels, compaction kernels)."""
        ms = np.zeros(2, np.float32)
        check(_lib.load().ictr_stereotrack_get_kernel_times(self._h, _lib.fp(ms)))
        return float(ms[0]), float(ms[1])


def stereo_track_window(disp_lr, disp_rl, flow_l, flow_r, xy0=None, th_ratio=0.2, th_abs=1.0, window=None):
    """stereo_track_window_host on the device, bit for bit: the same arguments (float32 fields in host memory or torch
    tensors on the device; a ``flow`` entry is a (fwd, bwd) pair or a (2, H, W, 2) array), the same (xy_t, rows).
    ``window``: a StereoTrackWindow of the right size to reuse."""
    bsize = len(disp_lr)
    if bsize < 1 or len(disp_rl) != bsize:
        raise ValueError("disp_lr and disp_rl need one plane per frame, at least one frame")
    if len(flow_l) < bsize - 1 or len(flow_r) < bsize - 1:
        raise ValueError("flow_l and flow_r need bsize - 1 (fwd, bwd) pairs")
    h, w = tuple(disp_lr[0].shape)
    win = window if window is not None else StereoTrackWindow(w, h, bsize, th_ratio, th_abs)
    win.open(field(disp_lr[0], -1), disp_rl[0], xy0)
    for fr in range(1, bsize):
        win.advance(flow_l[fr - 1][0], flow_l[fr - 1][1], flow_r[fr - 1][0], flow_r[fr - 1][1], field(disp_lr[fr], -1),
                    disp_rl[fr])
    win.count()
    return win.read()


class StereoPointTracker:
    """Frames in, window out: the script's loop (run_test_OF_track.py:74-110 and 170-223) composed from the device stages.
    Per stereo frame the two pyramids and the two stereo FlowGrids (left -> right, right -> left, used x only), per frame
    pair the four temporal grids; the grid handles go to a StereoTrackWindow. No dense field is formed and the host reads
    nothing back before window(). keep_grids=True keeps every frame's grids in ``grids`` (a list of dicts lr, rl and, from
    the second frame on, l_fwd, l_bwd, r_fwd, r_bwd) for inspection; otherwise two sets are reused in turn.
    disparity="2d" (the default) computes the stereo grids with the 2-D tracker and drops y; "1d" computes them with the
    1-D search along x (FlowGrid.compute_x), which keeps vertical edges and is not misled by tilted 1-D structure.
    refine=None: the grids go to the window as they are. refine=dict (parameters of patchflow.FlowRefiner, {} for its
    defaults): every grid's dense field is refined per pixel on the device (the stereo fields with x_only) and the
    refiners go to the window in the grids' place; keep_grids=True keeps them too, in ``refiners`` (same layout).
    densify=None: nothing is made or launched. densify=dict (parameters of patchflow.FlowDensifier, {} for its defaults):
    every grid is densified photometrically on the device (grid -> densify -> refine): with refine the refiners read the
    densifiers, without it the window does; keep_grids=True keeps them in ``densifiers`` (same layout).
    flow="grid" (the default) is all of the above. flow="c2f" computes the six fields of a frame with
    patchflow.CoarseToFineFlow objects instead (the stereo ones 2-D, y dropped by the window): no grid, densifier or
    refiner of the tracker's own is made; densify and refine are then the per-level parameters (densify=None: the
    densifier's defaults), and keep_grids=True keeps the objects in ``flows`` (same layout). disparity="1d" is refused
    with flow="c2f": its stereo fields are 2-D; the 1-D form is flow="c2f-1d". flow="c2f-1d" is flow="c2f" with the
    stereo pair (lr, rl) computed by CoarseToFineFlow(x_only=True), the 1-D search along x per level (vertical edges
    kept, tilted structure not misleading, v = +0.0), and the four temporal fields 2-D as before; patnorm, densify,
    refine and keep_grids behave as with flow="c2f", and `disparity` is not consulted. patnorm=True switches on the coarse-to-fine objects' patch-mean
    normalisation (CoarseToFineFlow's patnorm: for a right camera or a next frame of another brightness); it
    needs flow="c2f" or "c2f-1d" and is refused with flow="grid", whose whole-pyramid kernels have no such form.
    lv_l (default 0) is the finest level of every coarse-to-fine object of both sets (CoarseToFineFlow's lv_l: the levels
    lv_f .. lv_l run and the field of level lv_l is up-sampled to the frame); above 0 it likewise needs flow="c2f" or
    "c2f-1d". colour=True (likewise flow="c2f" or "c2f-1d" alone): push_frames takes (h, w, 3) frames and holds three
    pyramids per side, one per channel, and every object is a CoarseToFineFlow(channels=3); the fields the window reads
    are the same w x h flow planes. cost="huber" (with huber_k, default 5.0 grey levels) searches every coarse-to-fine
    field with the Huber patch cost (CoarseToFineFlow's cost and huber_k); it likewise needs flow="c2f" or "c2f-1d" and is
    refused with flow="grid", whose whole-pyramid kernels have no such form. lockstep=True (likewise flow="c2f" or
    "c2f-1d" alone; default False) runs a frame's coarse-to-fine objects as patchflow.CoarseToFineFlowSet objects, one
    launch per level and stage for all of them: with flow="c2f" one set of the six fields (of the two stereo ones at the
    window's first frame), with flow="c2f-1d" a set of the two stereo fields (x_only) and a set of the four temporal
    ones. The fields, and with them the window, are the same bit for bit."""

    def __init__(self, w, h, bsize=14, step=4, psz=15, lv_f=3, maxiter=10, eps=0.01, th_ratio=0.2, th_abs=1.0,
                 xy0=None, keep_grids=False, disparity="2d", refine=None, densify=None, flow="grid", patnorm=False,
                 lv_l=0, colour=False, cost="l2", huber_k=5.0, lockstep=False):
        if disparity not in ("2d", "1d"):
            raise ValueError(f"disparity is '2d' (the 2-D tracker, y dropped) or '1d' (the 1-D search), not {disparity!r}")
        if flow not in ("grid", "c2f", "c2f-1d"):
            raise ValueError("flow is 'grid' (a FlowGrid per field), 'c2f' (a CoarseToFineFlow per field) or 'c2f-1d' (the "
                             f"same with the stereo pair searched along x only), not {flow!r}")
        if flow == "c2f" and disparity == "1d":
            raise ValueError("flow='c2f' with disparity='1d': the 1-D form of the coarse-to-fine flow is flow='c2f-1d'")
        if patnorm and flow not in ("c2f", "c2f-1d"):
            raise ValueError("patnorm=True needs flow='c2f': patch-mean normalisation is built for the coarse-to-fine flow "
                             "alone, not for the flow grids of flow='grid'")
        if lv_l and flow not in ("c2f", "c2f-1d"):
            raise ValueError("lv_l > 0 needs flow='c2f' or 'c2f-1d': a finest level above 0 is built for the coarse-to-fine "
                             "flow alone, not for the flow grids of flow='grid'")
        if colour and flow not in ("c2f", "c2f-1d"):
            raise ValueError("colour=True needs flow='c2f' or 'c2f-1d': colour frames are built for the coarse-to-fine flow "
                             "alone, not for the flow grids of flow='grid'")
        from .patchflow import C2F_COST_HUBER, _c2f_cost
        code, self.huber_k = _c2f_cost(cost, huber_k, "StereoPointTracker")
        self.cost = "huber" if code == C2F_COST_HUBER else "l2"
        if self.cost == "huber" and flow not in ("c2f", "c2f-1d"):
            raise ValueError("cost='huber' needs flow='c2f' or 'c2f-1d': the robust patch cost is built for the "
                             "coarse-to-fine flow alone, not for the flow grids of flow='grid'")
        if lockstep and flow not in ("c2f", "c2f-1d"):
            raise ValueError("lockstep=True needs flow='c2f' or 'c2f-1d': lockstep sets are built for the coarse-to-fine "
                             "flow alone, not for the flow grids of flow='grid'")
        self.lockstep = bool(lockstep)
        self._locksets = {}  # lockstep=True: the sets by their members
        self.flow = flow
        self.colour = bool(colour)
        self.lv_l = int(lv_l)
        self.patnorm = bool(patnorm)
        self.flows = []
        self._fsets = [None, None]
        self._xsets = [None, None]  # flow="c2f-1d": the stereo pair's objects
        self.disparity = disparity
        self.refine = None if refine is None else dict(refine)
        self.refiners = []
        self._rsets = [None, None]
        self.densify = None if densify is None else dict(densify)
        self.densifiers = []
        self._dsets = [None, None]
        self.w, self.h, self.bsize = int(w), int(h), int(bsize)
        self.step, self.psz, self.lv_f, self.maxiter, self.eps = int(step), int(psz), int(lv_f), int(maxiter), float(eps)
        self.xy0, self.keep_grids = xy0, bool(keep_grids)
        self.win = StereoTrackWindow(w, h, bsize, th_ratio, th_abs)
        self.nframes = 0
        self.grids = []
        self._pyr = [None, None]  # (left, right) of the previous frame and of the one before, reused in turn
        self._sets = [None, None]

    def _set(self, cache, k, make, names=("lr", "rl", "l_fwd", "l_bwd", "r_fwd", "r_bwd")):
        """Frame k's six objects of one kind, by name: new ones when the grids are kept, else one of the two sets of
        `cache`, reused in turn."""
        if self.keep_grids:
            return {n: make() for n in names}
        if cache[k & 1] is None:
            cache[k & 1] = {n: make() for n in names}
        return cache[k & 1]

    def push_frames(self, left, right):
        from .patchflow import FlowDensifier, FlowGrid, FlowRefiner
        from .tracker import Pyramid
        k = self.nframes
        if k >= self.bsize:
            raise ValueError(f"the window holds {self.bsize} frames")
        imgs = [_lib.f32c(left), _lib.f32c(right)]
        if self.colour:  # three pyramids per side, one per channel, rebuilt in place like the grey ones
            for im in imgs:
                if im.shape != (self.h, self.w, 3):
                    raise ValueError(f"push_frames needs ({self.h}, {self.w}, 3) colour frames with colour=True, got "
                                     f"{im.shape}")
            chans = [[np.ascontiguousarray(im[..., c]) for c in range(3)] for im in imgs]
            slot = self._pyr[k & 1]
            if slot is None:
                slot = self._pyr[k & 1] = [[Pyramid(ch, self.lv_f, self.psz, True) for ch in side] for side in chans]
            else:
                for ps, side in zip(slot, chans):
                    for p, ch in zip(ps, side):
                        p.rebuild(ch)
        else:
            for im in imgs:
                if im.shape != (self.h, self.w):
                    raise ValueError(f"push_frames needs {self.w}x{self.h} frames, got {im.shape[1]}x{im.shape[0]}")
            slot = self._pyr[k & 1]
            if slot is None:
                slot = self._pyr[k & 1] = [Pyramid(im, self.lv_f, self.psz, True) for im in imgs]
            else:
                for p, im in zip(slot, imgs):
                    p.rebuild(im)
        pl, pr = slot
        kw = dict(psz=self.psz, lv_f=self.lv_f, maxiter=self.maxiter, eps=self.eps)
        # the frame's fields (name, A, B, x_only): the stereo pair, then from the second frame on the four temporal ones
        fields = [("lr", pl, pr, True), ("rl", pr, pl, True)]
        if k:
            ql, qr = self._pyr[(k - 1) & 1]
            fields += [("l_fwd", ql, pl, False), ("l_bwd", pl, ql, False), ("r_fwd", qr, pr, False),
                       ("r_bwd", pr, qr, False)]
        if self.flow in ("c2f", "c2f-1d"):
            return self._push_c2f(k, fields)
        g = self._set(self._sets, k, lambda: FlowGrid(self.w, self.h, self.step))
        z = r = None  # made when the stereo group reaches them
        for group in (fields[:2], fields[2:]):  # within each group: grid, then densify, then refine
            for n, a, b, x_only in group:
                (g[n].compute_x if x_only and self.disparity == "1d" else g[n].compute)(a, b, **kw)
            if self.densify is not None:
                z = z or self._set(self._dsets, k, lambda: FlowDensifier(self.w, self.h, **self.densify))
                for n, a, b, _ in group:
                    z[n].run(g[n], a, b, self.psz)
            if self.refine is not None:
                r = r or self._set(self._rsets, k, lambda: FlowRefiner(self.w, self.h, **self.refine))
                for n, a, b, x_only in group:
                    r[n].run(a, b, (z or g)[n], x_only=x_only)
        f = r or z or g  # what the window reads: the grids, their densifiers, or the refiners of either
        if k == 0:
            self.win.open(f["lr"], f["rl"], self.xy0)
        else:
            self.win.advance(f["l_fwd"], f["l_bwd"], f["r_fwd"], f["r_bwd"], f["lr"], f["rl"])
        if self.keep_grids:
            for kept, s in ((self.grids, g), (self.refiners, r), (self.densifiers, z)):
                if s is not None:
                    kept.append(s if k else {n: s[n] for n in ("lr", "rl")})
        self.nframes = k + 1

    def _push_c2f(self, k, fields):
        """push_frames with flow="c2f" or "c2f-1d": one CoarseToFineFlow per field, handed to the window. With "c2f-1d"
        the stereo pair's objects search along x only; they are a set of their own."""
        from .patchflow import CoarseToFineFlow

        def make(x_only=False):
            return CoarseToFineFlow(self.w, self.h, self.lv_f, self.step, self.psz, self.maxiter, self.eps,
                                    densify=self.densify, refine=self.refine, patnorm=self.patnorm, x_only=x_only,
                                    lv_l=self.lv_l, channels=3 if self.colour else 1, cost=self.cost,
                                    huber_k=self.huber_k)

        if self.flow == "c2f-1d":
            c = dict(self._set(self._fsets, k, make, ("l_fwd", "l_bwd", "r_fwd", "r_bwd")))
            c.update(self._set(self._xsets, k, lambda: make(True), ("lr", "rl")))
        else:
            c = self._set(self._fsets, k, make)
        if self.lockstep and self.keep_grids:  # every frame has new objects: the sets of earlier frames are not needed again
            self._locksets.clear()
        if self.lockstep:  # the stereo pair apart where its objects differ (x_only) from the temporal ones
            groups = (fields[:2], fields[2:]) if self.flow == "c2f-1d" else (fields,)
            for group in groups:
                if group:
                    self._lockset([c[n] for n, _, _, _ in group]).run([(a, b) for _, a, b, _ in group])
        else:
            for n, a, b, _ in fields:
                c[n].run(a, b)
        if k == 0:
            self.win.open(c["lr"], c["rl"], self.xy0)
        else:
            self.win.advance(c["l_fwd"], c["l_bwd"], c["r_fwd"], c["r_bwd"], c["lr"], c["rl"])
        if self.keep_grids:
            self.flows.append(c if k else {n: c[n] for n in ("lr", "rl")})
        self.nframes = k + 1

    def _lockset(self, flows):
        """The CoarseToFineFlowSet of these objects: made once per group of objects (which it keeps alive)."""
        from .patchflow import CoarseToFineFlowSet
        key = tuple(id(f) for f in flows)
        if key not in self._locksets:
            self._locksets[key] = CoarseToFineFlowSet(flows)
        return self._locksets[key]

    def window(self):
        """(xy_t (M, 4, bsize), rows (M,)) once bsize frames have been pushed."""
        if self.nframes != self.bsize:
            raise ValueError(f"{self.nframes} of {self.bsize} frames pushed")
        return self.win.read()

    def cameras(self, cam, baseline, **kw):
        """Frames in, cameras out: the counted window handed to windowcams.cameras_from_window on the device (its
        arguments and its dict); xy_t is never formed."""
        from .windowcams import cameras_from_window
        if self.nframes != self.bsize:
            raise ValueError(f"{self.nframes} of {self.bsize} frames pushed")
        return cameras_from_window(self.win, cam, baseline, **kw)
