"""f32 NumPy restatement of k_patchdisp (csrc/ictr_patchflow.hip) for test_patchdisp_cpu.py. The kernel is k_patchflow's
walk down the pyramid around pf_level_search's 1-D rule; so is this file: patchflow_f32.track_points with x_only, whose
level_search states that rule (shape = (NPL, WPP) or None for one serial sum, see there). It is written from the kernel and
shares no code with the oracle (patchdisp_np.py).

defect (None or one of DEFECTS + TAP_DEFECTS) injects one mistake the tests must be able to see: patchflow_f32's six and
its two tap defects, and three of the 1-D rule itself ("solve by tr" and "y follows x" in level_search, "no doubling" in
the walk).
"""
from __future__ import annotations

from patchflow_f32 import DEFECTS as _SHARED
from patchflow_f32 import TAP_DEFECTS  # noqa: F401  (the two failure forms of a rounded-up first tap, in _taps)
from patchflow_f32 import track_points

DEFECTS = _SHARED + ("solve by tr", "y follows x", "no doubling")


def track_disparity(pyr_a, pyr_b, pts, psz, lv_f, lv_l=0, maxiter=10, eps=0.01, min_hx=1e-2, shape=None, defect=None):
    """k_patchdisp for one patch after the other: x moves, y keeps the input's bits. pyr_*: oracle.Pyramid."""
    return track_points(pyr_a, pyr_b, pts, psz, lv_f, lv_l, maxiter, eps, min_hx, shape, defect, x_only=True)
