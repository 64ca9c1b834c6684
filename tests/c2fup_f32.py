"""The up-sampling that finishes a coarse-to-fine run whose finest level is above 0, as csrc/ictr_c2fflow.hip computes it,
restated in NumPy float32: k_flow_upsample<XONLY> and the launcher's sequence of an object made with lv_l. Written from the
kernel: per output pixel the source position (x + 0.5) 2^-lv - 0.5 clamped to the level, the cast that is its floor, the
second tap clamped, rx and 1 - rx (all exact in f32), then per component the six products and three sums in the kernel's
order, each rounded to f32, and the product with 2^lv (exact). x_only: the y component is not read and is written as +0.0.

A run with lv_l is c2fflow_f32.run's (patnorm_f32's, c2fdisp_f32's) stages down to level lv_l and this on that stage's
field. The CPU module measures its distance to patchflow.upsample_flow_host (the definition, f64); the GPU tests demand its
bits of the device.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32


def _taps(n, nl, inv_s):
    f = np.minimum(np.maximum((np.arange(n).astype(f32) + f32(0.5)) * inv_s - f32(0.5), f32(0)), f32(nl - 1))
    assert f.dtype == f32
    i0 = f.astype(np.int64)
    r = f - i0.astype(f32)
    return i0, np.minimum(i0 + 1, nl - 1), r, f32(1) - r


def upsample(field, w, h, lv, x_only=False):
    """k_flow_upsample<x_only>: (h_l, w_l, 2) f32 -> (h, w, 2) f32."""
    F = np.ascontiguousarray(field, f32)
    hl, wl = F.shape[:2]
    s = f32(1 << lv)
    inv_s = f32(1) / s
    x0, x1, rx, qx = _taps(w, wl, inv_s)
    y0, y1, ry, qy = _taps(h, hl, inv_s)
    rx, qx, ry, qy = rx[None, :], qx[None, :], ry[:, None], qy[:, None]
    out = np.zeros((h, w, 2), f32)
    for k in range(1 if x_only else 2):
        P = F[..., k]
        top = qx * P[y0][:, x0] + rx * P[y0][:, x1]
        bot = qx * P[y1][:, x0] + rx * P[y1][:, x1]
        val = s * (qy * top + ry * bot)
        assert val.dtype == f32
        out[..., k] = val
    return out


def run(pyr_a, pyr_b, step=4, psz=8, lv_f=2, lv_l=0, maxiter=10, eps=0.01, densify=None, refine=None, patnorm=False,
        x_only=False, stages=None):
    """ictr_c2fflow_run of an object made with lv_l: the (H, W, 2) f32 result. stages: a list that receives the tuples of
    the levels lv_f .. lv_l (the module's that restates the form: level, field, d, status[, bias])."""
    st = []
    if x_only:
        import c2fdisp_f32 as R
        field = R.run(pyr_a, pyr_b, step, psz, lv_f, maxiter, eps, densify, refine, patnorm=patnorm, stages=st)
    elif patnorm:
        import patnorm_f32 as R
        field = R.run(pyr_a, pyr_b, step, psz, lv_f, maxiter, eps, densify, refine, stages=st)
    else:
        import c2fflow_f32 as R
        field = R.run(pyr_a, pyr_b, step, psz, lv_f, maxiter, eps, densify, refine, stages=st)
    kept = [s for s in st if s[0] >= lv_l]
    if stages is not None:
        stages.extend(kept)
    if lv_l == 0:
        return field
    w, h = (pyr_a.img[0].shape[1] - 2 * pyr_a.pad, pyr_a.img[0].shape[0] - 2 * pyr_a.pad)
    return upsample(kept[-1][1], w, h, lv_l, x_only)
