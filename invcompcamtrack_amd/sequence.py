"""Frame-to-frame sequence tracking (run_odometer_test.m:172-250): frame t -> t+1 for every t of a video, each pair
started from the pose just found for frame t, with the step between two pairs on the device (ictr_sequence_*).

Per pair t -> t+1, with p_t the tracked pose of frame t (p_0 given):

1. cull -- every world point projected at level 0 in f64 with G(p_t) (the library's f64 exp map); kept iff
   ``1 <= u <= w`` and ``1 <= v <= h`` (the script's bounds literally, ``w, h`` the unpadded frame size). There is NO
   depth test: the reference has none.
2. subsample -- the survivors of ranks 0, s, 2s, ... in world-index order, then Set3Dpoints' cap: the first
   ``min(count, maxpttrack)``. The script passes the selected count itself as maxpttrack; here the cap is fixed when
   the tracker is made, and ``npts == cap`` in the result shows a pair where it bit.
3. Set3Dpoints + SetPose(p_t, pyr_t, pyr_t+1) + TrackPose, as a fresh run_io_reprojection_test process would.
4. no point selected (a deviation: the reference would divide by zero) -- p_t+1 = p_t, npts = iters = 0.

``SequenceTracker`` runs it on the GPU in one enqueue; ``track_sequence_host_loop`` is the same loop through the
public per-pair API (the comparison path for tests and timings); ``select_points`` restates steps 1-2 in NumPy.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._hostmath import se3_exp_d
from ._lib import check, dp, f64c
from .tracker import Pyramid, TrackBatch

__all__ = ["SequenceTracker", "track_sequence", "select_points", "track_sequence_host_loop", "selection_hash"]


def _cam_params(cam):
    """(fx, fy, cx, cy, w, h) at level 0 as float64: a CamClass or a dict with fc, cc, wh."""
    if isinstance(cam, dict):
        fc, cc = np.asarray(cam["fc"], np.float32), np.asarray(cam["cc"], np.float32)
        w, h = (int(v) for v in cam["wh"])
        return float(fc[0]), float(fc[1]), float(cc[0]), float(cc[1]), w, h
    return (float(cam.getfx(0)), float(cam.getfy(0)), float(cam.getcx(0)), float(cam.getcy(0)), int(cam._wh[0]),
            int(cam._wh[1]))


def select_points(pts3d_world, p, cam, stride=10, cap=None):
    """Steps 1-2 for one pair: world indices (int64, world order) of the points the pair tracks."""
    X = np.asarray(pts3d_world, np.float64).reshape(3, -1)
    fx, fy, cx, cy, w, h = _cam_params(cam)
    G = se3_exp_d(p).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):  # (a NaN or infinite coordinate fails every comparison)
        xc = G[0] * X[0] + G[1] * X[1] + G[2] * X[2] + G[3]
        yc = G[4] * X[0] + G[5] * X[1] + G[6] * X[2] + G[7]
        zc = G[8] * X[0] + G[9] * X[1] + G[10] * X[2] + G[11]
        u = fx * xc / zc + cx
        v = fy * yc / zc + cy
    keep = np.nonzero((u >= 1.0) & (u <= w) & (v >= 1.0) & (v <= h))[0]
    sel = keep[::int(stride)]
    return sel if cap is None else sel[:int(cap)]


def _mix(z):
    z = (z + np.uint64(0x9E3779B97F4A7C15))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def selection_hash(sel):
    """The device's hash of one pair's selection: sum of splitmix64((k << 32) | index_k) modulo 2^64."""
    sel = np.asarray(sel, np.uint64)
    if sel.size == 0:
        return 0
    with np.errstate(over="ignore"):
        z = (np.arange(sel.size, dtype=np.uint64) << np.uint64(32)) | sel
        return int(np.sum(_mix(z), dtype=np.uint64))


class SequenceTracker:
    """The whole sequence on the device: per pair one pyramid build, the selection launches and one one-launch tracking
    on one stream; the host is not involved between pairs. ``op.maxpttrack`` is the cap and decides the launch form
    (``last_team``)."""

    def __init__(self, cam, op, pts3d_world, stride=10):
        X = f64c(np.asarray(pts3d_world, np.float64).reshape(3, -1))
        self.cam, self.op, self.stride, self.nworld = cam, op, int(stride), X.shape[1]
        L = _lib.load()
        self._h = C.c_void_p()
        check(L.ictr_sequence_create(C.byref(self._h), cam._h, C.byref(op), self.nworld, self.stride))
        check(L.ictr_sequence_set_points(self._h, dp(X)))
        self._n = 0
        self._keep = None

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.load().ictr_sequence_destroy(self._h)
            self._h = None

    @property
    def last_team(self):
        """Workgroups per tracking launch: 1 = the single-workgroup form, > 1 = the team form."""
        return _lib.load().ictr_sequence_last_team(self._h)

    def set_robust(self, flags):
        check(_lib.load().ictr_sequence_set_robust(self._h, int(flags), 0.0))

    def track_async(self, frames, p0, stream=None):
        """frames: numpy (N, h, w) float32 or a CPU tensor (copied to the device once), or a tensor of that shape on the
        current GPU (borrowed until wait). stream: a torch stream or a raw hipStream_t (int); None = the null stream."""
        L = _lib.load()
        if hasattr(frames, "data_ptr") and getattr(frames, "is_cuda", False):
            import torch
            if frames.dim() != 3:
                raise ValueError("frames must be (N, h, w)")
            if not frames.is_contiguous() or frames.dtype != torch.float32:
                raise ValueError("device frames must be a contiguous float32 tensor")
            if frames.device.index != torch.cuda.current_device():
                raise ValueError(f"device frames live on cuda:{frames.device.index}, the tracker runs on "
                                 f"cuda:{torch.cuda.current_device()}")
            n, h, w = frames.shape
            check(L.ictr_sequence_set_frames(self._h, C.c_void_p(frames.data_ptr()), n, w, h, 1))
            self._keep = frames
        else:  # host memory (numpy, or a CPU tensor): copied to the device once
            f = frames.numpy() if hasattr(frames, "numpy") and hasattr(frames, "data_ptr") else frames
            f = np.asarray(f, np.float32)
            if f.ndim != 3:
                raise ValueError("frames must be (N, h, w)")
            f = np.ascontiguousarray(f)
            n, h, w = f.shape
            check(L.ictr_sequence_set_frames(self._h, f.ctypes.data_as(C.c_void_p), n, w, h, 0))
            self._keep = None
        sp = getattr(stream, "cuda_stream", stream)
        check(L.ictr_sequence_set_stream(self._h, C.c_void_p(sp or 0)))
        check(L.ictr_sequence_track_async(self._h, dp(f64c(p0))))
        self._n = int(n)

    def wait(self):
        """dict(poses (N, 6) f64, npts (N-1,) int32, iters (N-1,) int32)."""
        n = self._n
        if n < 2:  # nothing enqueued: the library's own message
            check(_lib.load().ictr_sequence_wait(self._h, None, None, None))
        poses = np.zeros((n, 6), np.float64)
        npts = np.zeros(n - 1, np.int32)
        iters = np.zeros(n - 1, np.int32)
        ip = C.POINTER(C.c_int32)
        check(_lib.load().ictr_sequence_wait(self._h, dp(poses), npts.ctypes.data_as(ip), iters.ctypes.data_as(ip)))
        self._keep = None
        return dict(poses=poses, npts=npts, iters=iters)

    def selection_hashes(self):
        out = np.zeros(max(self._n - 1, 1), np.uint64)
        check(_lib.load().ictr_sequence_selection_hashes(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def last_selection(self):
        """Inspection, after wait: what the last pair's selection left on the device -- dict(npts int, sel (npts,) int32
        world indices, ms (3,) f64, varval f64, pt3d (3, M) f32 with M = op.maxpttrack: the normalised points, zero
        behind npts)."""
        M = int(self.op.maxpttrack)
        n = C.c_int32(0)
        sel = np.full(M, -1, np.int32)
        ms = np.zeros(3, np.float64)
        vv = C.c_double(0.0)
        pt3d = np.zeros((3, M), np.float32)
        check(_lib.load().ictr_sequence_last_selection(self._h, C.byref(n), sel.ctypes.data_as(C.POINTER(C.c_int32)),
                                                       dp(ms), C.byref(vv), pt3d.ctypes.data_as(_lib.FP)))
        return dict(npts=int(n.value), sel=sel[:n.value].copy(), ms=ms, varval=float(vv.value), pt3d=pt3d)


def track_sequence(cam, op, pts3d_world, frames, p0, stride=10, stream=None):
    """track_async + wait on a fresh SequenceTracker."""
    s = SequenceTracker(cam, op, pts3d_world, stride)
    s.track_async(frames, p0, stream)
    return s.wait()


def track_sequence_host_loop(cam, op, pts3d_world, frames, p0, stride=10, return_selection=False, engine=None):
    """The same sequence as a host loop through the public per-pair API (select in NumPy, Set3Dpoints, SetPose,
    TrackPose with a blocking read-back per pair). Same result dict as SequenceTracker.wait.

    frames: numpy (N, h, w) float32 (each frame is uploaded when its pyramid is built), or a tensor of that shape on the
    GPU (the pyramids are built from device memory). Each frame's pyramid is built once, into a ring of two pyramids.
    engine: a TrackBatch of one problem to reuse (made here when None)."""
    X = np.asarray(pts3d_world, np.float64).reshape(3, -1)
    on_device = hasattr(frames, "data_ptr") and getattr(frames, "is_cuda", False)
    if on_device:
        n, h, w = frames.shape
        step = h * w * 4

        def build(k, pyr=None):
            ptr = frames.data_ptr() + k * step
            if pyr is None:
                return Pyramid(None, op.lv_f, op.psz, True, device_ptr=ptr, wh=(w, h))
            return pyr.rebuild(device_ptr=ptr)
    else:
        frames = [np.ascontiguousarray(f, np.float32) for f in frames]
        n = len(frames)

        def build(k, pyr=None):
            return Pyramid(frames[k], op.lv_f, op.psz, True) if pyr is None else pyr.rebuild(frames[k])
    eng = TrackBatch(cam, op, 1) if engine is None else engine
    poses = np.zeros((n, 6), np.float64)
    npts = np.zeros(n - 1, np.int32)
    iters = np.zeros(n - 1, np.int32)
    sels = []
    poses[0] = np.asarray(p0, np.float64)
    ring = [build(0), build(1)]
    for t in range(n - 1):
        ref, new = ring[t % 2], ring[(t + 1) % 2]
        if t > 0:
            build(t + 1, new)  # (the previous pair's tracking has been read back: nothing reads this pyramid any more)
        sel = select_points(X, poses[t], cam, stride, op.maxpttrack)
        sels.append(sel)
        if sel.size == 0:
            poses[t + 1] = poses[t]
        else:
            pts = np.ascontiguousarray(X[:, sel])
            eng.Set3Dpoints(0, pts)
            eng.SetPose(0, poses[t], ref, new)
            eng.track_async()
            poses[t + 1] = eng.poses()[0]
            iters[t] = eng.iterations()[0]
            npts[t] = sel.size
    out = dict(poses=poses, npts=npts, iters=iters)
    if return_selection:
        out["selection"] = sels
    return out
