"""The 1-D (x only) form of the coarse-to-fine dense flow as csrc/ictr_c2fflow.hip computes it, restated in NumPy float32:
k_c2f_level<NPL, WPP, MEAN, true> and the launcher's per-level sequence with the object's x_only switch set. Written from
the kernel: the start is the x component of one record of the coarser field times two (y is not read and is +0.0), the
search is pf_level_search's XONLY rule at this level (patchflow_f32.level_search with x_only; with patnorm its MEAN form,
level_search_mean_x here: the sum of T joins hxx and hyy, the sum of Gx is taken once, an iteration has ONE reduction of
(sum Gx (T' - I), sum I) and bx = s + (sum I / n) sum Gx), the rejection is scalar, the bias tail stays in the node's row,
and y is written as +0.0. The unchanged pieces are those of c2fflow_f32.py (start, fill), densify_f32.py / patnorm_f32.py
(the densifier, plain and biased, which gets no switch) and flowrefine_f32.py (the refinement, with x_only).

The CPU module measures its distance to patchflow.c2f_flow_host(x_only=True) (the definition, f64); the GPU tests demand
its bits of the device.

`defect` injects one mistake a kernel of this shape can make; test_c2fdisp_cpu.py shows that each is seen:
  "init not doubled"   the start is the coarser field's x, not twice it
  "det conditioning"   the 2-D test det > min_det tr^2 decides instead of hxx > min_hx tr (seen on vertical stripes)
  "far psz"            the rejection compares the squared distance with psz, not psz^2
  "y follows x"        the search moves y (patchflow_f32.level_search's defect of that name)
  "beta at start"      patnorm: beta is taken at the node's start, not at its final position
  "frame mean kept"    patnorm: the (sum I / n) sum Gx term is dropped, bx = s
"""
from __future__ import annotations

import numpy as np

import c2fflow_f32 as C2
import densify_f32 as DZ
import flowrefine_f32 as FR
import patnorm_f32 as PNF
from patchflow_f32 import ONE, STOP_COND, STOP_NONE, STOP_VIEW, ZERO, _fetch, _sum, _taps, f32, level_search

DEFECTS = ("init not doubled", "det conditioning", "far psz", "y follows x", "beta at start", "frame mean kept")
PATNORM_DEFECTS = DEFECTS[4:]   # seen only with patnorm on
LOST, TRACKED, HELD_COND, HELD_VIEW, HELD_FAR = range(5)
MIN_HX, MIN_DET = 1e-2, 1e-4


def level_search_mean_x(va, vax, vay, vb, wl, hl, xl, yl, px, P, maxiter, eps2, min_cond, shape, defect=None):
    """pf_level_search<NPL, WPP, true, true> for one patch. Returns (px, iterations, STOP_*, mean(T))."""
    n = f32(P * P)
    ta = _taps(xl, yl, P, None)
    T, Gx, Gy = (_fetch(v, ta, P) for v in (va, vax, vay))
    hxx, hyy, st = _sum(Gx * Gx, shape, None), _sum(Gy * Gy, shape, None), _sum(T, shape, None)
    mean_t = f32(st / n)
    T = T - mean_t
    assert T.dtype == f32
    tr = f32(hxx + hyy)
    if not (tr > 0) or not (hxx > f32(min_cond * tr)):
        return px, 0, STOP_COND, mean_t
    sgx = _sum(Gx, shape, None)
    with np.errstate(over="ignore"):
        inv = f32(ONE / hxx)
    for nit in range(maxiter):
        cx = f32(xl + px)
        if not (cx >= 0 and yl >= 0 and cx <= wl and yl <= hl):
            return px, nit, STOP_VIEW, mean_t
        I = _fetch(vb, _taps(cx, yl, P, None), P)
        bx, si = _sum(Gx * (T - I), shape, None), _sum(I, shape, None)
        if defect != "frame mean kept":
            bx = f32(bx + f32(f32(si / n) * sgx))
        dx = f32(bx * inv)
        px = f32(px + dx)
        if f32(dx * dx) < eps2:
            return px, nit + 1, STOP_NONE, mean_t
    return px, maxiter, STOP_NONE, mean_t


def init_of(coarse, w, h, step, defect=None):
    """(ny, nx, 2) f32: the kernel's start per node, x from the coarser field and y = +0.0; coarse None at the coarsest
    level."""
    init = C2.init_of(coarse, w, h, step, "init not doubled" if defect == "init not doubled" else None).copy()
    init[..., 1] = ZERO
    return init


def search(pyr_a, pyr_b, l, init, step, psz, maxiter=10, eps=0.01, patnorm=False, defect=None):
    """k_c2f_level<NPL, WPP, patnorm, true> for one node after the other: (d before the fill (ny, nx, 2) f32, NaN at a
    lost node; lost (ny, nx) bool; status (ny, nx) uint8; bias (ny, nx) f32, None without patnorm)."""
    P = psz
    shape = C2.form_shape(P)
    w, h = C2.level_size(pyr_a, l)
    wl, hl = f32(w), f32(h)
    xs, ys = np.arange(step // 2, w, step), np.arange(step // 2, h, step)
    ny, nx = len(ys), len(xs)
    sh, shb = pyr_a.pad - P, pyr_b.pad - P
    va, vax, vay = (p[sh:, sh:] for p in (pyr_a.img[l], pyr_a.dx[l], pyr_a.dy[l]))
    vb = pyr_b.img[l][shb:, shb:]
    eps2, min_hx = f32(f32(eps) * f32(eps)), f32(MIN_HX)
    far2 = f32(P) if defect == "far psz" else f32(P * P)
    d = np.full((ny, nx, 2), np.nan, f32)
    status = np.zeros((ny, nx), np.uint8)
    bias = np.zeros((ny, nx), f32) if patnorm else None

    for j, Y in enumerate(ys):
        for i, X in enumerate(xs):
            xl, yl = f32(X), f32(Y)
            ix = init[j, i, 0]
            sx = f32(xl + ix)
            if not (np.isfinite(ix) and sx >= 0 and yl >= 0 and sx <= wl and yl <= hl):
                continue
            refused = False
            if defect == "det conditioning":
                Gx, Gy = (_fetch(v, _taps(xl, yl, P, None), P) for v in (vax, vay))
                hxx, hxy, hyy = (_sum(t, shape, None) for t in (Gx * Gx, Gx * Gy, Gy * Gy))
                tr = f32(hxx + hyy)
                det = f32(f32(hxx * hyy) - f32(hxy * hxy))
                refused = not (det > f32(f32(f32(MIN_DET) * tr) * tr)) or not (tr > 0)
            mean_t = ZERO
            if refused:
                px, why = ix, STOP_COND
                if patnorm:
                    mean_t = f32(_sum(_fetch(va, _taps(xl, yl, P, None), P), shape, None) / f32(P * P))
            elif patnorm:
                px, _, why, mean_t = level_search_mean_x(va, vax, vay, vb, wl, hl, xl, yl, ix, P, maxiter, eps2, min_hx,
                                                         shape, defect)
            else:
                px, _, _, why = level_search(va, vax, vay, vb, wl, hl, xl, yl, ix, ZERO, P, maxiter, eps2, min_hx,
                                             x_only=True, shape=shape,
                                             defect="y follows x" if defect == "y follows x" else None)
            st = {STOP_NONE: TRACKED, STOP_COND: HELD_COND, STOP_VIEW: HELD_VIEW}[why]
            if st == TRACKED:
                ex = f32(px - ix)
                if not (f32(ex * ex) <= far2):
                    st = HELD_FAR
            held = st >= HELD_COND
            status[j, i] = st
            d[j, i] = (ix if held else px, ZERO)
            if patnorm:  # the tail: one more window pass of B at the final position, in the node's row
                fx = f32(xl + (ix if defect == "beta at start" else d[j, i, 0]))
                if fx >= 0 and yl >= 0 and fx <= wl and yl <= hl:
                    sb = _sum(_fetch(vb, _taps(fx, yl, P, None), P), shape, None)
                    bias[j, i] = f32(f32(sb / f32(P * P)) - mean_t)
    return d, status == LOST, status, bias


def level(pyr_a, pyr_b, l, coarse, step, psz, maxiter=10, eps=0.01, densify=None, refine=None, patnorm=False, defect=None,
          init=None):
    """One level as ictr_c2fflow_run enqueues it with x_only set: (field (h, w, 2), d after the fill, status, bias)."""
    w, h = C2.level_size(pyr_a, l)
    if init is None:
        init = init_of(coarse, w, h, step, defect)
    d, lost, status, bias = search(pyr_a, pyr_b, l, init, step, psz, maxiter, eps, patnorm, defect)
    filled = C2.fill(d, lost)
    A, B = C2.plane(pyr_a, l), C2.plane(pyr_b, l)
    dz = dict(dict(minerr=2.0, power=1), **(densify or {}))
    if patnorm:
        field = PNF.densify(A, B, filled, lost, bias, step, psz, dz["minerr"], dz["power"])
    else:
        field = DZ.densify(A, B, filled, lost, step, psz, dz["minerr"], dz["power"])
    if refine is not None:
        field = FR.refine(A, B, field, x_only=True, **refine)
    return field, filled, status, bias


def run(pyr_a, pyr_b, step=4, psz=8, lv_f=2, maxiter=10, eps=0.01, densify=None, refine=None, patnorm=False, defect=None,
        stages=None):
    """ictr_c2fflow_run with x_only set: level 0's field (H, W, 2) f32. stages: a list that receives (level, field, d,
    status, bias) per level from lv_f down."""
    field = None
    for l in range(lv_f, -1, -1):
        field, d, status, bias = level(pyr_a, pyr_b, l, field, step, psz, maxiter, eps, densify, refine, patnorm, defect)
        if stages is not None:
            stages.append((l, field, d, status, bias))
    return field
