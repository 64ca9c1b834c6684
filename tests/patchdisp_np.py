"""f64 oracle of the 1-D (x only) patch search k_patchdisp (csrc/ictr_patchflow.hip): the statement of record of its rule.

TEST INFRASTRUCTURE ONLY. Written on oracle.np_patchflow's _sample, _Template and _level_size (imported, not edited), so
the patches are the 2-D oracle's patches and the pyramid convention (a plane padded by more than psz is read through a
view) is the same. Everything that is not listed here is np_patchflow.track_points':

    per level     p *= 2 below lv_f; xl = x0 scale, yl = y0 scale; in-view test on (xl, yl); T, Gx, Gy at (xl, yl)
    conditioning  hxx = sum Gx^2, hyy = sum Gy^2, tr = hxx + hyy (hxy is not formed);
                  lost iff !(tr > 0) or !(hxx > min_hx tr), min_hx = 1e-2
    iteration     cx = xl + p; in-view test on (cx, yl); I at (cx, yl); r = T - I; bx = sum Gx r; dx = bx / hxx;
                  p += dx; ++nit; stop when dx^2 < eps^2. y never moves.
    output        (x0 + p 2^lv_l, y0) with y0's input bits; lost: (NaN, NaN), status 0

Error bound of an f32 evaluation of one step, first order, u = 2^-24, for a form that adds L pixels per lane with WPP
waves per patch. d hxx, d bx and the sum constant L + 7 + (WPP - 1) are np_patchflow's (its docstring); the solve is one
reciprocal and one product:

    dx = bx * (1 / hxx):    d dx = d bx / hxx + |bx| d hxx / hxx^2 + 2 u |dx|
"""
from __future__ import annotations

import numpy as np

from oracle.np_patchflow import U, _level_size, _sample, _Template, f32

MIN_HX = 1e-2


def form_of(psz):
    """(NPL, WPP) of launch_patchdisp: by the patch size alone."""
    npl = (psz * psz + 63) // 64
    return (8, 2) if npl > 4 else (1 if npl <= 1 else 4, 1)


def _step(t, plane_b, pad, cx, yl, psz):
    """dx and its bound for the template t against frame B sampled at (cx, yl)."""
    I, aI = _sample(plane_b, cx, yl, psz, pad)
    aGx = np.abs(t.Gx)
    r = t.T - I
    ar = np.abs(r)
    er = t.eT + 3 * U * aI + U * ar
    bx = (t.Gx * r).sum()
    dbx = (t.eGx * ar + aGx * er).sum() + t.S * (aGx * ar).sum()
    dx = bx / t.hxx
    ex = dbx / t.hxx + abs(bx) * t.dhxx / (t.hxx * t.hxx) + 2 * U * abs(dx)
    return dx, ex


def _kept(t, min_hx):
    return bool(t.tr > 0) and bool(t.hxx > min_hx * t.tr)


def track_disparity(pyr_a, pyr_b, pts, psz, lv_f, lv_l=0, maxiter=10, eps=0.01, min_hx=MIN_HX, detail=False, nsum=24):
    """pyr_*: oracle.Pyramid (host planes, padded by pad >= psz). pts (K,2). Returns (new (K,2) f32 with NaN, status,
    iters), and with detail=True a fourth value: a dict of per-point (K,) f64 arrays
      view   smallest distance of a tested cx from the border it is tested against (0, w_l), from the second test of a
             run on (xl is exact in f32 and the first cx of a run is xl + 0). inf if none.
      view0  the same over every test of x, the exact ones included
      hx     smallest |hxx / tr - min_hx| over the levels reached (inf where tr == 0)
      eps    smallest |dx^2 - eps^2| over the steps taken;  eps_px: smallest | |dx| - eps |
      bound  sum over the steps taken of the one-step bound * 2^level, for sums of nsum = L + c terms
    """
    pts = np.asarray(pts, f32)
    K = len(pts)
    out = np.full((K, 2), np.nan, f32)
    status = np.zeros(K, bool)
    iters = np.zeros(K, np.int32)
    d = {k: np.full(K, np.inf) for k in ("view", "view0", "hx", "eps", "eps_px")}
    d["bound"] = np.zeros(K)

    def border(k, x, wl, exact):
        m = float(min(abs(np.float64(x)), abs(np.float64(x) - wl)))
        d["view0"][k] = min(d["view0"][k], m)
        if not exact:
            d["view"][k] = min(d["view"][k], m)

    for k in range(K):
        x0, y0 = pts[k]
        if not (np.isfinite(x0) and np.isfinite(y0)):
            continue
        p = f32(0)
        ok, nit, first = True, 0, True
        for l in range(lv_f, lv_l - 1, -1):
            if l != lv_f:
                p = f32(p * f32(2))
            sc = f32(0.5 ** l)
            wl, hl = _level_size(pyr_a, l)
            xl, yl = f32(x0 * sc), f32(y0 * sc)
            border(k, xl, wl, True)
            if not (0 <= xl <= wl and 0 <= yl <= hl):
                ok = False
                break
            t = _Template(pyr_a, l, xl, yl, psz, nsum)
            if t.tr > 0:
                d["hx"][k] = min(d["hx"][k], abs(t.hxx / t.tr - min_hx))
            if not _kept(t, min_hx):
                ok = False
                break
            for _ in range(maxiter):
                cx = f32(xl + p)
                border(k, cx, wl, first)
                first = False
                if not (0 <= cx <= wl):
                    ok = False
                    break
                dx, ex = _step(t, pyr_b.img[l], pyr_b.pad, cx, yl, psz)
                p = f32(p + dx)
                nit += 1
                d["eps"][k] = min(d["eps"][k], abs(dx * dx - eps * eps))
                d["eps_px"][k] = min(d["eps_px"][k], abs(abs(dx) - eps))
                d["bound"][k] += ex * 2.0 ** l
                if dx * dx < eps * eps:
                    break
            if not ok:
                break
        if ok:
            out[k] = (x0 + p * f32(2.0 ** lv_l), y0)
        status[k], iters[k] = ok, nit
    return (out, status, iters, d) if detail else (out, status, iters)


def one_step(pyr_a, pyr_b, pts, psz, level, L, wpp=1, min_hx=MIN_HX):
    """The step bx / hxx of every point at one level from p = 0, in f64 on the f32 patch values, and the bound of an f32
    evaluation that adds L pixels per lane with wpp waves per patch. Returns (step (K,) f64, bound (K,) f64, hxx / tr
    (K,) f64); NaN for points that are not finite, out of view at the level or refused by the conditioning test."""
    pts = np.asarray(pts, f32)
    K = len(pts)
    step, bound, cond = np.full(K, np.nan), np.full(K, np.nan), np.full(K, np.nan)
    sc = f32(0.5 ** level)
    wl, hl = _level_size(pyr_a, level)
    for k in range(K):
        x0, y0 = pts[k]
        if not (np.isfinite(x0) and np.isfinite(y0)):
            continue
        xl, yl = f32(x0 * sc), f32(y0 * sc)
        if not (0 <= xl <= wl and 0 <= yl <= hl):
            continue
        t = _Template(pyr_a, level, xl, yl, psz, L + 7 + (wpp - 1))
        if t.tr > 0:
            cond[k] = t.hxx / t.tr
        if not _kept(t, min_hx):
            continue
        step[k], bound[k] = _step(t, pyr_b.img[level], pyr_b.pad, xl, yl, psz)
    return step, bound, cond
