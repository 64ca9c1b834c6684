"""What the device objects of the window stages share (CameraFitter, BundleAdjuster, CameraRansac): the checked forms of
their inputs, points ``X`` (3, N), observations ``xy`` ((S,) F, 2, N), a mask as inlier words, a camera ``(fc, cc)``, and
the base class that carries their setters, host arrays or a counted StereoTrackWindow alike, over ``ictr_<prefix>_*``
(csrc/ictr_wininputs.h is the same block on the C side)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, dp, f64c

_U64P = C.POINTER(C.c_uint64)


def _as_points(X):
    a = f64c(X)
    if a.ndim != 2 or a.shape[0] != 3 or a.shape[1] < 1:
        raise ValueError(f"X must be (3, N), got {a.shape}")
    return a


def _as_obs(xy, n, frames=(1, None), sides=False):
    """xy as (F, 2, n), where (2, n) is one frame, or with sides as (S, F, 2, n), S = 1 or 2, where (F, 2, n) is one
    side; frames: the lowest and the highest F (None: no limit)."""
    a = f64c(xy)
    if a.ndim == (3 if sides else 2):
        a = a[None]
    if sides:
        if a.ndim != 4 or a.shape[0] not in (1, 2) or a.shape[2] != 2 or a.shape[3] != n:
            raise ValueError(f"xy must be (S, F, 2, {n}) with S = 1 or 2, got {a.shape}")
    elif a.ndim != 3 or a.shape[1] != 2 or a.shape[2] != n:
        raise ValueError(f"xy must be (F, 2, {n}), got {a.shape}")
    lo, hi = frames
    if hi is not None and not lo <= a.shape[-3] <= hi:
        raise ValueError(f"{a.shape[-3]} frames ({lo} .. {hi})")
    return a


def _as_cam(cam):
    fc, cc = cam
    fc, cc = f64c(fc).reshape(-1), f64c(cc).reshape(-1)
    if fc.size != 2 or cc.size != 2:
        raise ValueError("cam must be (fc (2,), cc (2,))")
    return float(fc[0]), float(fc[1]), float(cc[0]), float(cc[1])


def _pack_words(mask):
    """bool (N,) as inlier words uint64 (ceil(N / 64),): point i is bit i % 64 of word i // 64, the bits past N clear."""
    n = mask.size
    bits = np.zeros((n + 63) // 64 * 64, np.uint8)
    bits[:n] = mask
    return np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view(np.uint64).copy()


def _words_of(mask, n):
    """The inlier words of a mask: None, bool (N,), or uint64 words already (ceil(N / 64),)."""
    if mask is None:
        return None
    m = np.asarray(mask)
    nwords = (n + 63) // 64
    if m.dtype == np.uint64:
        if m.shape != (nwords,):
            raise ValueError(f"{m.shape} mask words for {n} points")
        return np.ascontiguousarray(m)
    if m.dtype != bool or m.shape != (n,):
        raise ValueError(f"mask must be bool ({n},) or uint64 ({nwords},)")
    return _pack_words(m)


def _stream(stream):
    return C.c_void_p(getattr(stream, "cuda_stream", stream) or 0)


class _WindowInputs:
    """One ictr_<_PREFIX> object for N points seen in F frames (from S sides where the object has sides). A subclass
    names its C prefix, the noun of its messages, the kinds of kernel_times and its own form of _as_obs."""
    _PREFIX = _NOUN = None
    _KINDS = ()
    _as_obs = staticmethod(_as_obs)

    def _c(self, entry, debug=False):
        return getattr(_lib.load(), f"ictr_debug_{self._PREFIX}_{entry}" if debug else f"ictr_{self._PREFIX}_{entry}")

    def _create(self, n, nframes, nsides=None):
        self._h = C.c_void_p()
        sides = () if nsides is None else (int(nsides),)
        check(self._c("create")(C.byref(self._h), int(n), int(nframes), *sides))
        self.n, self.nframes, self.nwords = int(n), int(nframes), (int(n) + 63) // 64
        if sides:
            self.nsides = sides[0]
        self._obs_shape = sides + (self.nframes, 2, self.n)

    def __del__(self):
        if getattr(self, "_h", None):
            self._c("destroy")(self._h)
            self._h = None

    def set_points(self, X):
        a = _as_points(X)
        if a.shape[1] != self.n:
            raise ValueError(f"X {a.shape}, the {self._NOUN} was made for (3, {self.n})")
        check(self._c("set_points")(self._h, dp(a)))

    def set_observations(self, xy):
        a = self._as_obs(xy, self.n)
        if a.shape != self._obs_shape:
            raise ValueError(f"xy {a.shape}, the {self._NOUN} was made for {self._obs_shape}")
        check(self._c("set_observations")(self._h, dp(a)))

    def set_mask(self, mask=None):
        w = _words_of(mask, self.n)
        check(self._c("set_mask")(self._h, None if w is None else w.ctypes.data_as(_U64P)))

    def set_camera(self, cam):
        fx, fy, cx, cy = _as_cam(cam)
        check(self._c("set_camera")(self._h, dp(np.array([fx, fy])), dp(np.array([cx, cy]))))

    def set_points_from_window(self, win, baseline):
        """points_from_first_view(depth_from_disparity(...)) of a counted StereoTrackWindow, on the device, with the
        camera of set_camera, which comes first."""
        check(self._c("set_points_from_window")(self._h, win._h, float(baseline)))

    def set_observations_from_window(self, win):
        """observations_from_stereo_tracks of a counted StereoTrackWindow, on the device: the left side and, for an
        object of two sides, the right one."""
        check(self._c("set_observations_from_window")(self._h, win._h))

    def debug_inputs(self):
        """Inspection (ictr_debug_<prefix>_inputs): dict X (3, N), xy ((S,) F, 2, N), words (ceil(N / 64),) as they stand
        on the device."""
        X, xy, words = np.zeros((3, self.n)), np.zeros(self._obs_shape), np.zeros(self.nwords, np.uint64)
        check(self._c("inputs", debug=True)(self._h, dp(X), dp(xy), words.ctypes.data_as(_U64P)))
        return dict(X=X, xy=xy, words=words)

    def set_timing(self, on=True):
        """Record device time stamps around the launches of the next runs (kernel_times)."""
        check(self._c("set_timing")(self._h, int(bool(on))))

    def kernel_times(self):
        """ms of the last waited run per kernel kind (_KINDS), summed over its launches."""
        ms = np.zeros(len(self._KINDS), np.float32)
        check(self._c("get_kernel_times")(self._h, ms.ctypes.data_as(_lib.FP)))
        return dict(zip(self._KINDS, (float(v) for v in ms)))


class _MaskedWindowInputs(_WindowInputs):
    """... whose mask can come from another object's last run on the device."""

    def set_mask_from_fsplit(self, splitter, stream=None):
        """The inlier words of the StaticSplitter's last run, waited for or in flight, copied on the device on `stream`
        (the stream of that run)."""
        check(self._c("set_mask_from_fsplit")(self._h, splitter._h, _stream(stream)))

    def set_mask_from_camransac(self, ransac, stream=None):
        """The winner's inlier words of the CameraRansac's last run, waited for or in flight, copied on the device on
        `stream` (the stream of that run)."""
        check(self._c("set_mask_from_camransac")(self._h, ransac._h, _stream(stream)))
