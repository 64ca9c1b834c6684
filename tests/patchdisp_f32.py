"""f32 NumPy restatement of k_patchdisp (csrc/ictr_patchflow.hip) for test_patchdisp_cpu.py: the kernel's operations in
their order, every one rounded to f32 (the build has -ffp-contract=off), in a selectable summation shape. It is written
from the kernel and shares no code with the oracle (patchdisp_np.py). The kernel takes its taps, blend and sums from the
functions k_patchflow takes them from (pf_taps, pf_blend, wave_sum_dpp, the wave-order LDS sum); so does this file, from
their restatement in patchflow_f32.py (_taps, _fetch, _sum; shape = (NPL, WPP) or None for one serial sum, see there).

defect (None or one of DEFECTS + TAP_DEFECTS) injects one mistake the tests must be able to see: patchflow_f32's six and
its two tap defects, which act in the shared functions, and three of the 1-D rule itself.
"""
from __future__ import annotations

import numpy as np

from patchflow_f32 import DEFECTS as _SHARED
from patchflow_f32 import TAP_DEFECTS  # noqa: F401  (the two failure forms of a rounded-up first tap, in _taps)
from patchflow_f32 import ONE, ZERO, _fetch, _sum, _taps, f32

DEFECTS = _SHARED + ("solve by tr", "y follows x", "no doubling")


def track_disparity(pyr_a, pyr_b, pts, psz, lv_f, lv_l=0, maxiter=10, eps=0.01, min_hx=1e-2, shape=None, defect=None):
    """The kernel's control flow for one patch after the other. pyr_*: oracle.Pyramid."""
    pts = np.asarray(pts, f32)
    K, P = len(pts), psz
    out = np.full((K, 2), np.nan, f32)
    status, iters = np.zeros(K, bool), np.zeros(K, np.int32)
    sh = pyr_a.pad - P
    eps2, min_hx = f32(f32(eps) * f32(eps)), f32(min_hx)
    q = np.arange(P * P)
    keep = np.ones(P * P, bool)
    if defect == "drop last column":
        keep = q % P != P - 1
    elif defect == "drop last row":
        keep = q // P != P - 1

    def view(plane):
        return plane[sh:, sh:] if sh else plane

    def in_view(x, y, w, h):
        return x >= 0 and y >= 0 and x <= w and y <= h

    for k in range(K):
        x0, y0 = pts[k]
        ok = bool(x0 == x0 and y0 == y0)
        px = ZERO
        nit = 0
        for l in range(lv_f, lv_l - 1, -1):
            if not ok:
                break
            if l != lv_f and defect != "no doubling":
                px = f32(px * f32(2))
            scale = f32(1 / 2 ** l)
            wl, hl = f32(pyr_a.img[l].shape[1] - 2 * pyr_a.pad), f32(pyr_a.img[l].shape[0] - 2 * pyr_a.pad)
            xl, yl = f32(x0 * scale), f32(y0 * scale)
            if not in_view(xl, yl, wl, hl):
                ok = False
                break
            ta = _taps(xl, yl, P, defect)
            T = np.where(keep, _fetch(view(pyr_a.img[l]), ta, P), ZERO)
            Gx = np.where(keep, _fetch(view(pyr_a.dx[l]), ta, P), ZERO)
            Gy = np.where(keep, _fetch(view(pyr_a.dy[l]), ta, P), ZERO)
            hxx, hyy = _sum(Gx * Gx, shape, defect), _sum(Gy * Gy, shape, defect)
            tr = f32(hxx + hyy)
            if not (tr > 0) or not (hxx > f32(min_hx * tr)):
                ok = False
                break
            with np.errstate(over="ignore"):
                ihx = f32(ONE / (tr if defect == "solve by tr" else hxx))
            for _ in range(maxiter):
                cx = f32(xl + px)
                cy = f32(yl + px) if defect == "y follows x" else yl
                if not in_view(cx, cy, wl, hl):
                    ok = False
                    break
                r = np.where(keep, T - _fetch(view(pyr_b.img[l]), _taps(cx, cy, P, defect), P), ZERO)
                bx = _sum(Gx * r, shape, defect)
                dx = f32(bx * ihx)
                px = f32(px + dx)
                nit += 1
                if f32(dx * dx) < eps2:
                    break
        if ok:
            s = f32(ONE / f32(1 / 2 ** (lv_f if defect == "rescale by lv_f" else lv_l)))
            out[k] = (f32(x0 + f32(px * s)), y0)
        status[k], iters[k] = ok, nit
    return out, status, iters
