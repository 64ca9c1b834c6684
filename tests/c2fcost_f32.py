"""The Huber patch cost of the coarse-to-fine dense flow as the device computes it, restated in NumPy float32: the ROBUST
forms of pf_level_search_ch (csrc/ictr_patchflow_dev.h) and of k_c2f_level (csrc/ictr_c2fflow_dev.h, instantiated by
csrc/ictr_c2fflow_robust.hip), for one channel or three. Written from the kernels.

Without patnorm the L2 iteration with one more operation per tap: r = T_c - I_c, r <- fminf(fmaxf(r, -k), k), then the
two products; the channels 0, 1, 2 into the same accumulators and ONE reduction, as c2frgb_f32.sum_ch states it (one
channel: patchflow_f32._sum's bits).
With patnorm the direct form in two passes: sum I_c per channel first (a single-channel sum each), mi_c = sum I_c / n,
then r = T'_c - (I_c - mi_c) with (I_c - mi_c) rounded first, the clip, the products and one reduction of b. The L2 MEAN
forms' sums of Gx and Gy and their b = s + mi sum G do not occur. T, Gx, Gy, H (with the sums of T_c behind it), the
conditioning decision, the view tests, the solve, the stop, the rejection and the bias tail are the L2 forms'.

The unchanged pieces are imported: taps, fetch and the sum shapes (patchflow_f32.py, c2frgb_f32.sum_ch), the start and the
fill (c2fflow_f32.py), the densifiers (densify_f32.py, patnorm_f32.py, c2frgb_f32.py), the refinements (flowrefine_f32.py,
c2frgb_f32.py) and the up-sampling (c2fup_f32.py). What is restated here is the search and the node loop around it.

The CPU module measures its distance to patchflow.c2f_flow_host(cost="huber") (the definition, f64); the GPU tests demand
its bits of the device.

`defect` injects one mistake a kernel of this shape can make; test_c2fcost_cpu.py shows that each is seen:
  "no clip"            the residual is not clipped (the L2 cost)
  "clip before mean"   patnorm: the clip is applied to T' - I, and the frame mean is added afterwards
  "k squared"          the clip is at k^2
"""
from __future__ import annotations

import numpy as np

import c2fflow_f32 as C2
import c2frgb_f32 as RGB
import c2fup_f32 as UP
import densify_f32 as DZ
import flowrefine_f32 as FR
import patnorm_f32 as PNF
from patchflow_f32 import ONE, STOP_COND, STOP_NONE, STOP_VIEW, ZERO, _fetch, _sum, _taps, f32

DEFECTS = ("no clip", "clip before mean", "k squared")
LOST, TRACKED, HELD_COND, HELD_VIEW, HELD_FAR = range(5)
MIN_DET, MIN_HX = 1e-4, 1e-2


def _clip(r, k):
    """fminf(fmaxf(r, -k), k) on finite residuals."""
    out = np.minimum(np.maximum(r, f32(-k)), k)
    assert out.dtype == f32
    return out


def level_search_robust(A, vb, wl, hl, xl, yl, px, py, P, maxiter, eps2, min_cond, x_only, mean, shape, k, defect=None,
                        clipped=None):
    """pf_level_search_ch<NPL, WPP, x_only, mean, len(A), SW, true> for one patch. A: per channel (va, vax, vay), vb: per
    channel the plane of frame B, all views padded by exactly P; k the f32 clip. Returns (px, py, iterations, STOP_*,
    [mean(T_c)]). clipped: a two-item list that counts the residuals the clip changed and all residuals."""
    nch = len(A)
    n = f32(P * P)
    k = f32(k * k) if defect == "k squared" else f32(k)
    ta = _taps(xl, yl, P, None)
    T = [_fetch(a[0], ta, P) for a in A]
    Gx = [_fetch(a[1], ta, P) for a in A]
    Gy = [_fetch(a[2], ta, P) for a in A]
    hxx, hyy = RGB.sum_ch([g * g for g in Gx], shape), RGB.sum_ch([g * g for g in Gy], shape)
    mean_t = [ZERO] * nch
    if mean:
        mean_t = [f32(_sum(T[c], shape, None) / n) for c in range(nch)]
        T = [T[c] - mean_t[c] for c in range(nch)]
    tr = f32(hxx + hyy)
    if x_only:
        refused = not (tr > 0) or not (hxx > f32(min_cond * tr))
        div = hxx
    else:
        hxy = RGB.sum_ch([Gx[c] * Gy[c] for c in range(nch)], shape)
        div = f32(f32(hxx * hyy) - f32(hxy * hxy))
        refused = not (div > f32(f32(min_cond * tr) * tr)) or not (tr > 0)
    if refused:
        return px, py, 0, STOP_COND, mean_t
    with np.errstate(over="ignore"):
        inv = f32(ONE / div)
    for nit in range(maxiter):
        cx, cy = f32(xl + px), (yl if x_only else f32(yl + py))
        if not (cx >= 0 and cy >= 0 and cx <= wl and cy <= hl):
            return px, py, nit, STOP_VIEW, mean_t
        tb = _taps(cx, cy, P, None)
        I = [_fetch(v, tb, P) for v in vb]
        if mean and defect == "clip before mean":
            r = [_clip(T[c] - I[c], k) + f32(_sum(I[c], shape, None) / n) for c in range(nch)]
        elif mean:  # pass 1: sum I_c, one reduction; pass 2: the mean-free window's residual
            mi = [f32(_sum(I[c], shape, None) / n) for c in range(nch)]
            r = [T[c] - (I[c] - mi[c]) for c in range(nch)]
        else:
            r = [T[c] - I[c] for c in range(nch)]
        assert r[0].dtype == f32
        if clipped is not None:
            clipped[0] += int(sum((np.abs(e) > k).sum() for e in r))
            clipped[1] += nch * P * P
        if defect not in ("no clip", "clip before mean"):
            r = [_clip(e, k) for e in r]
        bx = RGB.sum_ch([Gx[c] * r[c] for c in range(nch)], shape)
        by = ZERO if x_only else RGB.sum_ch([Gy[c] * r[c] for c in range(nch)], shape)
        if x_only:
            dx, dy = f32(bx * inv), ZERO
            step2 = f32(dx * dx)
        else:
            dx = f32(f32(f32(hyy * bx) - f32(hxy * by)) * inv)
            dy = f32(f32(f32(hxx * by) - f32(hxy * bx)) * inv)
            step2 = f32(f32(dx * dx) + f32(dy * dy))
        px, py = f32(px + dx), f32(py + dy)
        if step2 < eps2:
            return px, py, nit + 1, STOP_NONE, mean_t
    return px, py, maxiter, STOP_NONE, mean_t


def _as_list(pyr):
    return [pyr] if hasattr(pyr, "img") else list(pyr)


def search(pyr_a, pyr_b, l, init, step, psz, maxiter=10, eps=0.01, patnorm=False, x_only=False, huber_k=5.0, defect=None,
           clipped=None):
    """k_c2f_level<NPL, WPP, patnorm, x_only, NCH, true> for one node after the other; a frame is one pyramid or a list of
    three. Returns (d before the fill (ny, nx, 2) f32, NaN at a lost node; lost (ny, nx) bool; status (ny, nx) uint8; bias
    (ny, nx) f32, (ny, nx, 3) on three channels, None without patnorm)."""
    pas, pbs = _as_list(pyr_a), _as_list(pyr_b)
    nch = len(pas)
    P = psz
    shape = C2.form_shape(P)
    w, h = C2.level_size(pas[0], l)
    wl, hl = f32(w), f32(h)
    xs, ys = np.arange(step // 2, w, step), np.arange(step // 2, h, step)
    ny, nx = len(ys), len(xs)
    A = [tuple(q[p.pad - P:, p.pad - P:] for q in (p.img[l], p.dx[l], p.dy[l])) for p in pas]
    vb = [p.img[l][p.pad - P:, p.pad - P:] for p in pbs]
    eps2, min_cond = f32(f32(eps) * f32(eps)), f32(MIN_HX if x_only else MIN_DET)
    far2 = f32(P * P)
    d = np.full((ny, nx, 2), np.nan, f32)
    status = np.zeros((ny, nx), np.uint8)
    bias = np.zeros((ny, nx, nch), f32) if patnorm else None

    for j, Y in enumerate(ys):
        for i, X in enumerate(xs):
            xl, yl = f32(X), f32(Y)
            ix, iy = init[j, i]
            sx, sy = f32(xl + ix), f32(yl + iy)
            if not (np.isfinite(ix) and np.isfinite(iy) and sx >= 0 and sy >= 0 and sx <= wl and sy <= hl):
                continue
            px, py, _, why, mean_t = level_search_robust(A, vb, wl, hl, xl, yl, ix, iy, P, maxiter, eps2, min_cond, x_only,
                                                         patnorm, shape, huber_k, defect, clipped)
            st = {STOP_NONE: TRACKED, STOP_COND: HELD_COND, STOP_VIEW: HELD_VIEW}[why]
            if st == TRACKED:
                ex, ey = f32(px - ix), f32(py - iy)
                far = f32(ex * ex) if x_only else f32(f32(ex * ex) + f32(ey * ey))
                if not (far <= far2):
                    st = HELD_FAR
            held = st >= HELD_COND
            status[j, i] = st
            d[j, i] = (ix, iy) if held else (px, py)
            if patnorm:  # the tail: one more window pass of B at the final position, per channel
                fx, fy = f32(xl + d[j, i, 0]), f32(yl + d[j, i, 1])
                if fx >= 0 and fy >= 0 and fx <= wl and fy <= hl:
                    tb = _taps(fx, fy, P, None)
                    for c in range(nch):
                        sb = _sum(_fetch(vb[c], tb, P), shape, None)
                        bias[j, i, c] = f32(f32(sb / f32(P * P)) - mean_t[c])
    if patnorm and nch == 1:
        bias = bias[..., 0]
    return d, status == LOST, status, bias


def level(pyr_a, pyr_b, l, coarse, step, psz, maxiter=10, eps=0.01, patnorm=False, x_only=False, huber_k=5.0, refine=None,
          defect=None, init=None):
    """One level as a run with the Huber cost enqueues it: (field (h, w, 2), d after the fill, status, bias or None). Only
    the search differs from the L2 run: the fill, the densifier and the refinement are the imported ones."""
    pas, pbs = _as_list(pyr_a), _as_list(pyr_b)
    w, h = C2.level_size(pas[0], l)
    if init is None:
        init = C2.init_of(coarse, w, h, step).copy()
        if x_only:
            init[..., 1] = ZERO
    d, lost, status, bias = search(pyr_a, pyr_b, l, init, step, psz, maxiter, eps, patnorm, x_only, huber_k, defect)
    filled = C2.fill(d, lost)
    if len(pas) == 3:
        A, B = RGB.planes(pas, l), RGB.planes(pbs, l)
        field = RGB.densify(A, B, filled, lost, bias, step, psz)
        if refine is not None:
            field = RGB.refine(A, B, field, x_only=x_only, **refine)
    else:
        A, B = C2.plane(pas[0], l), C2.plane(pbs[0], l)
        field = PNF.densify(A, B, filled, lost, bias, step, psz) if patnorm else DZ.densify(A, B, filled, lost, step, psz)
        if refine is not None:
            field = FR.refine(A, B, field, x_only=x_only, **refine)
    return field, filled, status, bias


def run(pyr_a, pyr_b, step=4, psz=8, lv_f=2, lv_l=0, maxiter=10, eps=0.01, patnorm=False, x_only=False, huber_k=5.0,
        refine=None, defect=None, stages=None):
    """ictr_c2fflow_run / _run_rgb of an object with ictr_c2fflow_set_cost(ICTR_C2F_COST_HUBER, huber_k): the (H, W, 2) f32
    result. stages: a list that receives (level, field, d, status, bias) per level from lv_f down to lv_l."""
    field = None
    for l in range(lv_f, lv_l - 1, -1):
        field, d, status, bias = level(pyr_a, pyr_b, l, field, step, psz, maxiter, eps, patnorm, x_only, huber_k, refine,
                                       defect)
        if stages is not None:
            stages.append((l, field, d, status, bias))
    if lv_l == 0:
        return field
    w, h = C2.level_size(_as_list(pyr_a)[0], 0)
    return UP.upsample(field, w, h, lv_l, x_only)
