"""Patch-mean normalisation of the coarse-to-fine dense flow as the device computes it, restated in NumPy float32: the
MEAN forms of pf_level_search (csrc/ictr_patchflow_dev.h) and k_c2f_level with its bias tail (csrc/ictr_c2fflow.hip), and
k_densify<true, 1> (csrc/ictr_densify.hip). Written from the kernels: the sum of T joins the three sums of H, the sums of Gx
and Gy are taken once, an iteration has ONE reduction of (sum Gx (T' - I), sum Gy (T' - I), sum I) and
b = s + (sum I / n) sum G; the bias is sum(B at the final position) / n - sum(T) / n. The unchanged pieces (taps, fetch, the
sum shapes, the fill, the warp, the refinement) are those of patchflow_f32.py, c2fflow_f32.py, densify_f32.py.

The CPU module measures its distance to patchflow.c2f_flow_host(patnorm=True) (the definition, f64); the GPU tests demand
its bits of the device.

`defect` injects one mistake a kernel of this shape can make; test_patnorm_cpu.py shows that each is seen:
  "template mean kept"   T is not reduced by its mean
  "frame mean kept"      the frame window's mean is not added back: b = s
  "beta sign"            beta = mean(T) - mean(B)
  "beta at start"        beta is taken at the node's start, not at its final position
  "beta out of view"     a node whose final position is out of view keeps the beta of its position clamped into view
  "vote ignores beta"    the densifier weighs |Bw - A|
"""
from __future__ import annotations

import numpy as np

import c2fflow_f32 as C2
import densify_f32 as DZ
import flowrefine_f32 as FR
from patchflow_f32 import ONE, STOP_COND, STOP_NONE, STOP_VIEW, ZERO, _fetch, _sum, _taps, f32

DEFECTS = ("template mean kept", "frame mean kept", "beta sign", "beta at start", "beta out of view", "vote ignores beta")
LOST, TRACKED, HELD_COND, HELD_VIEW, HELD_FAR = range(5)
F = np.float32


def level_search_mean(va, vax, vay, vb, wl, hl, xl, yl, px, py, P, maxiter, eps2, min_cond, shape, defect=None):
    """pf_level_search<NPL, WPP, false, true> for one patch. Returns (px, py, iterations, STOP_*, mean(T))."""
    n = f32(P * P)
    ta = _taps(xl, yl, P, None)
    T, Gx, Gy = (_fetch(v, ta, P) for v in (va, vax, vay))
    hxx, hxy, hyy, st = _sum(Gx * Gx, shape, None), _sum(Gx * Gy, shape, None), _sum(Gy * Gy, shape, None), _sum(T, shape, None)
    mean_t = f32(st / n)
    if defect != "template mean kept":
        T = T - mean_t
    assert T.dtype == f32
    tr = f32(hxx + hyy)
    det = f32(f32(hxx * hyy) - f32(hxy * hxy))
    if not (det > f32(f32(min_cond * tr) * tr)) or not (tr > 0):
        return px, py, 0, STOP_COND, mean_t
    sgx, sgy = _sum(Gx, shape, None), _sum(Gy, shape, None)
    with np.errstate(over="ignore"):
        inv = f32(ONE / det)
    for nit in range(maxiter):
        cx, cy = f32(xl + px), f32(yl + py)
        if not (cx >= 0 and cy >= 0 and cx <= wl and cy <= hl):
            return px, py, nit, STOP_VIEW, mean_t
        I = _fetch(vb, _taps(cx, cy, P, None), P)
        r = T - I
        bx, by, si = _sum(Gx * r, shape, None), _sum(Gy * r, shape, None), _sum(I, shape, None)
        if defect != "frame mean kept":
            mi = f32(si / n)
            bx, by = f32(bx + f32(mi * sgx)), f32(by + f32(mi * sgy))
        dx = f32(f32(f32(hyy * bx) - f32(hxy * by)) * inv)
        dy = f32(f32(f32(hxx * by) - f32(hxy * bx)) * inv)
        step2 = f32(f32(dx * dx) + f32(dy * dy))
        px, py = f32(px + dx), f32(py + dy)
        if step2 < eps2:
            return px, py, nit + 1, STOP_NONE, mean_t
    return px, py, maxiter, STOP_NONE, mean_t


def search(pyr_a, pyr_b, l, init, step, psz, maxiter=10, eps=0.01, min_det=1e-4, defect=None):
    """k_c2f_level<NPL, WPP, true> for one node after the other: (d before the fill (ny, nx, 2) f32, NaN at a lost node;
    lost (ny, nx) bool; status (ny, nx) uint8; bias (ny, nx) f32)."""
    P = psz
    shape = C2.form_shape(P)
    w, h = C2.level_size(pyr_a, l)
    wl, hl = f32(w), f32(h)
    xs, ys = np.arange(step // 2, w, step), np.arange(step // 2, h, step)
    ny, nx = len(ys), len(xs)
    sh, shb = pyr_a.pad - P, pyr_b.pad - P
    va, vax, vay = (p[sh:, sh:] for p in (pyr_a.img[l], pyr_a.dx[l], pyr_a.dy[l]))
    vb = pyr_b.img[l][shb:, shb:]
    eps2, min_det = f32(f32(eps) * f32(eps)), f32(min_det)
    far2 = f32(P * P)
    d = np.full((ny, nx, 2), np.nan, f32)
    status = np.zeros((ny, nx), np.uint8)
    bias = np.zeros((ny, nx), f32)

    for j, Y in enumerate(ys):
        for i, X in enumerate(xs):
            xl, yl = f32(X), f32(Y)
            ix, iy = init[j, i]
            sx, sy = f32(xl + ix), f32(yl + iy)
            if not (np.isfinite(ix) and np.isfinite(iy) and sx >= 0 and sy >= 0 and sx <= wl and sy <= hl):
                continue
            px, py, _, why, mean_t = level_search_mean(va, vax, vay, vb, wl, hl, xl, yl, ix, iy, P, maxiter, eps2, min_det,
                                                       shape, defect)
            st = {STOP_NONE: TRACKED, STOP_COND: HELD_COND, STOP_VIEW: HELD_VIEW}[why]
            if st == TRACKED:
                ex, ey = f32(px - ix), f32(py - iy)
                if not (f32(f32(ex * ex) + f32(ey * ey)) <= far2):
                    st = HELD_FAR
            held = st >= HELD_COND
            status[j, i] = st
            d[j, i] = (ix, iy) if held else (px, py)
            # the tail: one more window pass of B at the final position
            qx, qy = (ix, iy) if defect == "beta at start" else d[j, i]
            fx, fy = f32(xl + qx), f32(yl + qy)
            votes = fx >= 0 and fy >= 0 and fx <= wl and fy <= hl
            if not votes and defect == "beta out of view":
                fx, fy, votes = min(max(fx, ZERO), wl), min(max(fy, ZERO), hl), True
            if votes:
                sb = _sum(_fetch(vb, _taps(fx, fy, P, None), P), shape, None)
                beta = f32(f32(sb / f32(P * P)) - mean_t)
                bias[j, i] = -beta if defect == "beta sign" else beta
    return d, status == LOST, status, bias


def densify(img_a, img_b, d_filled, lost, bias, step, psz, minerr=2.0, power=1, defect=None):
    """k_densify<true, 1>: densify_f32.densify with the node's beta taken off the residual, r = (Bw - A) - beta."""
    A, B = np.ascontiguousarray(img_a, F), np.ascontiguousarray(img_b, F)
    d = np.ascontiguousarray(d_filled, F)
    beta = np.zeros_like(bias) if defect == "vote ignores beta" else np.ascontiguousarray(bias, F)
    lost = np.asarray(lost).astype(bool)
    h, w = A.shape
    ny, nx = lost.shape
    half = step // 2
    lo, hi = psz - psz // 2, psz // 2 - 1
    xs, ys = np.arange(w), np.arange(h)
    i0, i1 = DZ.first_node(xs - hi - half, step), DZ.last_node(xs + lo - half, step, nx)
    j0, j1 = DZ.first_node(ys - hi - half, step), DZ.last_node(ys + lo - half, step, ny)
    rec = d.copy()
    rec[lost, 0] = np.nan
    yy, xx = np.mgrid[0:h, 0:w]
    xf, yf = xx.astype(F), yy.astype(F)
    su, sv, sw = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
    d0x, d0y = np.zeros((h, w), F), np.zeros((h, w), F)
    cnt = np.zeros((h, w), np.int32)
    me = F(minerr)
    na, nb = max(int((j1 - j0).max()) + 1, 0), max(int((i1 - i0).max()) + 1, 0)
    with np.errstate(invalid="ignore"):
        for a in range(na):
            jr = j0 + a
            vj = jr <= j1
            j = np.clip(jr, 0, ny - 1)
            for b in range(nb):
                ir = i0 + b
                vi = ir <= i1
                i = np.clip(ir, 0, nx - 1)
                dx, dy = rec[j][:, i, 0], rec[j][:, i, 1]
                px, py = xf + dx, yf + dy
                inside = (px >= F(0)) & (px <= F(w - 1)) & (py >= F(0)) & (py <= F(h - 1))
                ok = vj[:, None] & vi[None, :] & inside
                r = (DZ.bilinear(B, px, py) - A) - beta[j][:, i]
                m = np.fmax(np.abs(r), me)
                m2 = m * m
                mp = m if power == 1 else m2 if power == 2 else m2 * m if power == 3 else m2 * m2
                wgt = F(1) / mp
                first = ok & (cnt == 0)
                d0x, d0y = np.where(first, dx, d0x), np.where(first, dy, d0y)
                su = np.where(ok, su + wgt * (dx - d0x), su)
                sv = np.where(ok, sv + wgt * (dy - d0y), sv)
                sw = np.where(ok, sw + wgt, sw)
                cnt += ok
    out = DZ.fg_value(d, w, h, step)
    with np.errstate(invalid="ignore", divide="ignore"):
        out[..., 0] = np.where(cnt > 0, d0x + su / sw, out[..., 0])
        out[..., 1] = np.where(cnt > 0, d0y + sv / sw, out[..., 1])
    assert out.dtype == F and su.dtype == F and sw.dtype == F
    return out


def level(pyr_a, pyr_b, l, coarse, step, psz, maxiter=10, eps=0.01, densify_params=None, refine=None, defect=None,
          init=None):
    """One level as ictr_c2fflow_run enqueues it with patnorm on: (field (h, w, 2), d after the fill, status, bias)."""
    w, h = C2.level_size(pyr_a, l)
    if init is None:
        init = C2.init_of(coarse, w, h, step)
    d, lost, status, bias = search(pyr_a, pyr_b, l, init, step, psz, maxiter, eps, defect=defect)
    filled = C2.fill(d, lost)
    A, B = C2.plane(pyr_a, l), C2.plane(pyr_b, l)
    dz = dict(dict(minerr=2.0, power=1), **(densify_params or {}))
    field = densify(A, B, filled, lost, bias, step, psz, dz["minerr"], dz["power"], defect)
    if refine is not None:
        field = FR.refine(A, B, field, **refine)
    return field, filled, status, bias


def run(pyr_a, pyr_b, step=4, psz=8, lv_f=2, maxiter=10, eps=0.01, densify_params=None, refine=None, defect=None,
        stages=None):
    """ictr_c2fflow_run with patnorm on: level 0's field (H, W, 2) f32. stages: a list that receives (level, field, d,
    status, bias) per level from lv_f down."""
    field = None
    for l in range(lv_f, -1, -1):
        field, d, status, bias = level(pyr_a, pyr_b, l, field, step, psz, maxiter, eps, densify_params, refine, defect)
        if stages is not None:
            stages.append((l, field, d, status, bias))
    return field
