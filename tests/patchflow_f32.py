"""f32 NumPy restatement of the patch searches: level_search is pf_level_search (csrc/ictr_patchflow_dev.h), the search at
one pyramid level that k_patchflow, k_patchdisp and k_c2f_level share, 2-D or along x only; track_points is the walk of
k_patchflow and k_patchdisp around it (patchdisp_f32.py, c2fflow_f32.py hold what their kernels keep). The kernel's
per-pixel expressions in their order, every operation rounded to f32 (the build has -ffp-contract=off: no fused
multiply-add), and a selectable summation shape. It is written from the kernels, not from oracle/np_patchflow.py or
patchdisp_np.py, and shares no code with them.

shape = (NPL, WPP): pixel q of the patch belongs to wave (q // 64) % WPP, lane q % 64, slot q // (64 WPP); a lane adds its
slots serially from 0, the 64 lanes meet in a pairwise tree (wave_sum_dpp: 1, 2, half row, row, then (r0 + r1) + (r2 + r3)),
the WPP wave totals are added in wave order from 0.  shape = None: one serial sum over the pixels in q order.

defect (None or one of DEFECTS + TAP_DEFECTS) injects one mistake the tests must be able to see.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
ONE, ZERO = f32(1), f32(0)
DEFECTS = ("drop last column", "drop last row", "swap w1 w2", "half of P-1", "omit second wave", "rescale by lv_f")
# the two ways in which a first tap taken by rounding up x plus a small constant leaves the pair (floor, floor + 1) that
# the weights are taken for; injected like DEFECTS, seen by the truth and continuity checks of the far frames
TAP_DEFECTS = ("tap pair one back at large integers", "tap pair one ahead just below small integers")


def _first_tap(x, defect):
    """floor(x) + 1: the kernel's first tap (the second is floor(x))."""
    fl = np.floor(x)
    p = int(fl) + 1
    if defect == "tap pair one back at large integers" and x == fl and x >= 256:
        p -= 1                                    # taps (x - 1, x), all the weight on x - 1
    if defect == "tap pair one ahead just below small integers" and x != fl and fl + 1 <= 64 \
            and np.nextafter(x, f32(np.inf)) == fl + 1:
        p += 1                                    # taps (n, n + 1) for x = n - 1 ulp, weight ~1 on n + 1
    return p


def _taps(x, y, P, defect):
    x, y = f32(x), f32(y)
    p0, p1 = _first_tap(x, defect), _first_tap(y, defect)
    r0, r1 = f32(x - np.floor(x)), f32(y - np.floor(y))
    w0, w1, w2, w3 = f32(r0 * r1), f32(f32(ONE - r0) * r1), f32(r0 * f32(ONE - r1)), f32(f32(ONE - r0) * f32(ONE - r1))
    if defect == "swap w1 w2":
        w1, w2 = w2, w1
    half = (P - 1) // 2 if defect == "half of P-1" else P // 2
    return (w0, w1, w2, w3), p1 + half, p0 + half


def _fetch(plane, taps, P):
    """(P*P,) f32 in q order: t.w0 * (x, y) + t.w1 * (x-1, y) + t.w2 * (x, y-1) + t.w3 * (x-1, y-1), left to right."""
    (w0, w1, w2, w3), row, col = taps
    a = plane[row:row + P, col:col + P]
    b = plane[row:row + P, col - 1:col - 1 + P]
    c = plane[row - 1:row - 1 + P, col:col + P]
    d = plane[row - 1:row - 1 + P, col - 1:col - 1 + P]
    v = ((w0 * a + w1 * b) + w2 * c) + w3 * d
    assert v.dtype == f32
    return v.ravel()


def _sum(terms, shape, defect):
    """One patch sum of (P*P,) f32 terms in the given shape."""
    n = len(terms)
    if shape is None:
        acc = ZERO
        for t in terms:
            acc = f32(acc + t)
        return acc
    npl, wpp = shape
    assert n <= 64 * npl * wpp
    slots = np.zeros(64 * npl * wpp, f32)
    slots[:n] = terms
    slots = slots.reshape(npl, wpp, 64)           # [slot i][wave][lane]: q = wave * 64 + lane + 64 * wpp * i
    acc = np.zeros((wpp, 64), f32)
    for i in range(npl):
        acc = acc + slots[i]
    for _ in range(6):
        acc = acc[:, 0::2] + acc[:, 1::2]
    assert acc.dtype == f32 and acc.shape == (wpp, 1)
    if wpp == 1:
        return acc[0, 0]
    tot = ZERO
    for q in range(1 if defect == "omit second wave" else wpp):
        tot = f32(tot + acc[q, 0])
    return tot


STOP_NONE, STOP_COND, STOP_VIEW = range(3)    # why a patch stopped being tracked at a level (pf_level_search's result)


def level_search(va, vax, vay, vb, wl, hl, xl, yl, px, py, P, maxiter, eps2, min_cond, x_only=False, shape=None,
                 defect=None):
    """pf_level_search for one patch: the search at (xl, yl) of one level from the displacement (px, py), on the level's
    planes of frame A (image, gradients) and B as views padded by exactly P, (wl, hl) the level's unpadded size in f32.
    x_only is the 1-D rule of k_patchdisp: hxx and hyy alone, refused iff not tr > 0 or not hxx > min_cond tr, the solve
    bx * (1 / hxx), y never moves. Returns (px, py, iterations, STOP_*)."""
    def in_view(x, y):
        return x >= 0 and y >= 0 and x <= wl and y <= hl

    q = np.arange(P * P)
    keep = q % P != P - 1 if defect == "drop last column" else q // P != P - 1 if defect == "drop last row" else q >= 0
    ta = _taps(xl, yl, P, defect)
    T, Gx, Gy = (np.where(keep, _fetch(v, ta, P), ZERO) for v in (va, vax, vay))
    hxx, hyy = _sum(Gx * Gx, shape, defect), _sum(Gy * Gy, shape, defect)
    tr = f32(hxx + hyy)
    if x_only:
        lost = not (tr > 0) or not (hxx > f32(min_cond * tr))
        div = tr if defect == "solve by tr" else hxx
    else:
        hxy = _sum(Gx * Gy, shape, defect)
        div = det = f32(f32(hxx * hyy) - f32(hxy * hxy))
        lost = not (det > f32(f32(min_cond * tr) * tr)) or not (tr > 0)
    if lost:
        return px, py, 0, STOP_COND
    with np.errstate(over="ignore"):
        inv = f32(ONE / div)
    for nit in range(maxiter):
        cx, cy = f32(xl + px), f32(yl + py)
        if x_only:
            cy = f32(yl + px) if defect == "y follows x" else yl
        if not in_view(cx, cy):
            return px, py, nit, STOP_VIEW
        r = np.where(keep, T - _fetch(vb, _taps(cx, cy, P, defect), P), ZERO)
        bx = _sum(Gx * r, shape, defect)
        if x_only:
            dx, dy = f32(bx * inv), ZERO
            step2 = f32(dx * dx)
        else:
            by = _sum(Gy * r, shape, defect)
            dx = f32(f32(f32(hyy * bx) - f32(hxy * by)) * inv)
            dy = f32(f32(f32(hxx * by) - f32(hxy * bx)) * inv)
            step2 = f32(f32(dx * dx) + f32(dy * dy))
        px, py = f32(px + dx), f32(py + dy)
        if step2 < eps2:
            return px, py, nit + 1, STOP_NONE
    return px, py, maxiter, STOP_NONE


def track_points(pyr_a, pyr_b, pts, psz, lv_f, lv_l=0, maxiter=10, eps=0.01, min_cond=1e-4, shape=None, defect=None,
                 x_only=False):
    """The control flow of k_patchflow (x_only: of k_patchdisp) for one patch after the other: the point, the walk down
    the pyramid with the doubling and the level-entry view test, the rescale. pyr_*: oracle.Pyramid."""
    pts = np.asarray(pts, f32)
    K, P = len(pts), psz
    out = np.full((K, 2), np.nan, f32)
    status, iters = np.zeros(K, bool), np.zeros(K, np.int32)
    sh = pyr_a.pad - P
    eps2, min_cond = f32(f32(eps) * f32(eps)), f32(min_cond)
    for k in range(K):
        x0, y0 = pts[k]
        ok = bool(x0 == x0 and y0 == y0)
        px = py = ZERO
        nit = 0
        for l in range(lv_f, lv_l - 1, -1):
            if not ok:
                break
            if l != lv_f and defect != "no doubling":
                px, py = f32(px * f32(2)), f32(py * f32(2))
            scale = f32(1 / 2 ** l)
            wl, hl = f32(pyr_a.img[l].shape[1] - 2 * pyr_a.pad), f32(pyr_a.img[l].shape[0] - 2 * pyr_a.pad)
            xl, yl = f32(x0 * scale), f32(y0 * scale)
            if not (xl >= 0 and yl >= 0 and xl <= wl and yl <= hl):
                ok = False
                break
            planes = (p[sh:, sh:] for p in (pyr_a.img[l], pyr_a.dx[l], pyr_a.dy[l], pyr_b.img[l]))
            px, py, n, why = level_search(*planes, wl, hl, xl, yl, px, py, P, maxiter, eps2, min_cond, x_only, shape, defect)
            nit += n
            ok = why == STOP_NONE
        if ok:
            s = f32(ONE / f32(1 / 2 ** (lv_f if defect == "rescale by lv_f" else lv_l)))
            out[k] = (f32(x0 + f32(px * s)), y0 if x_only else f32(y0 + f32(py * s)))
        status[k], iters[k] = ok, nit
    return out, status, iters
