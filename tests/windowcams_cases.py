"""Inputs and host references of the window hand-over tests, computed once and shared (read-only) between
test_windowcams_cpu.py and test_gpu_windowcams.py: the golden windows of tests/golden/stereotrack_golden.npz with the camera
of camfit_cases, at the threshold where the split keeps a real share of the points (0.03 px) and at the default."""
import functools

import numpy as np

import camfit_cases as K
from invcompcamtrack_amd import windowcams as W
from test_stereotrack_cpu import fields, golden

WINDOWS = ["small_disp", "large_disp", "odd_long", "two_frames"]
TIGHT = 0.03  # px: the winning trial is not trial 0 and the mask is not all ones
KEYS = ("m", "words", "mask", "inliers", "best_trial", "best_count", "draws", "F", "dd", "G", "p", "cost", "damp", "iters",
        "status", "n", "err_left", "err_right")


def freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def host(name, thresh=2.0):
    """window_cameras_host of a golden window, with its tracks."""
    return freeze(W.window_cameras_host(*fields(golden()[name]), K.CAM, K.BASELINE, thresh=thresh, tracks=True))


def same(got, want, what="", keys=KEYS):
    """Every key equal in type, shape and bytes."""
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (what, k)
