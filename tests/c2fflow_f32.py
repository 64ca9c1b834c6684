"""The coarse-to-fine dense flow as csrc/ictr_c2fflow.hip computes it, restated in NumPy float32. It is written from the
kernel k_c2f_level and its launcher, not from the host function: the node position from the node index, the start as one
record of the coarser field times two, the search at this level alone, the hold rules with their f32 comparisons, and
what is written. It composes, unchanged, the pieces the other stages are restated with:

  patchflow_f32.level_search            pf_level_search: k_patchflow's search at one level, in the form's sum shape
  densify_f32.densify                   k_densify on the level's planes
  flowrefine_f32.refine                 the refinement launches on the level's planes

The CPU module measures its distance to patchflow.c2f_flow_host (the definition, f64); the GPU tests demand its bits of
the device.

`defect` injects one mistake a kernel of this shape can make; test_c2fflow_cpu.py shows that each is seen:
  "init not doubled"   the start is the coarser field's value, not twice it
  "init row up"        the coarser row is (Y + 1) >> 1
  "no clamp"           min(Y >> 1, h' - 1) is not taken: row h' of the coarser field is read (the memory behind it, zeros)
  "held lost"          a held node is marked lost: it does not vote and is filled from its neighbours
  "far psz"            the rejection compares the squared distance with psz, not psz^2
  "held keeps p"       a held node writes the p it had reached, not its start
"""
from __future__ import annotations

import numpy as np

import densify_f32 as DZ
import flowrefine_f32 as FR
from patchflow_f32 import STOP_COND, STOP_NONE, STOP_VIEW, f32, level_search

DEFECTS = ("init not doubled", "init row up", "no clamp", "held lost", "far psz", "held keeps p")
LOST, TRACKED, HELD_COND, HELD_VIEW, HELD_FAR = range(5)


def form_shape(psz):
    """(NPL, WPP) of launch_c2f_level for a patch size: up to 4 pixels per lane one wave per node, above that two."""
    npl = (psz * psz + 63) // 64
    return (8, 2) if npl > 4 else (1 if npl <= 1 else 4, 1)


def level_size(pyr, l):
    return pyr.img[l].shape[1] - 2 * pyr.pad, pyr.img[l].shape[0] - 2 * pyr.pad


def plane(pyr, l):
    """The level's unpadded image plane (what ictr_pyramid_level0 addresses)."""
    p = pyr.pad
    return np.ascontiguousarray(pyr.img[l][p:pyr.img[l].shape[0] - p, p:pyr.img[l].shape[1] - p])


def init_of(coarse, w, h, step, defect=None):
    """(ny, nx, 2) f32: the kernel's start per node; coarse None at the coarsest level."""
    xs, ys = np.arange(step // 2, w, step), np.arange(step // 2, h, step)
    if coarse is None:
        return np.zeros((len(ys), len(xs), 2), f32)
    ch, cw = coarse.shape[:2]
    mem = np.concatenate([np.ascontiguousarray(coarse, f32).reshape(-1, 2), np.zeros((cw + 1, 2), f32)])
    rows = (ys + 1) >> 1 if defect == "init row up" else ys >> 1
    if defect != "no clamp":
        rows = np.minimum(rows, ch - 1)
    cols = np.minimum(xs >> 1, cw - 1)
    c = mem[rows[:, None] * cw + cols[None, :]]
    return c if defect == "init not doubled" else f32(2) * c


def search(pyr_a, pyr_b, l, init, step, psz, maxiter=10, eps=0.01, min_det=1e-4, defect=None):
    """k_c2f_level for one node after the other: (d before the fill (ny, nx, 2) f32, NaN at a lost node; lost (ny, nx)
    bool; status (ny, nx) uint8)."""
    P = psz
    shape = form_shape(P)
    w, h = level_size(pyr_a, l)
    wl, hl = f32(w), f32(h)
    xs, ys = np.arange(step // 2, w, step), np.arange(step // 2, h, step)
    ny, nx = len(ys), len(xs)
    sh = pyr_a.pad - P
    shb = pyr_b.pad - P
    va, vax, vay = (p[sh:, sh:] for p in (pyr_a.img[l], pyr_a.dx[l], pyr_a.dy[l]))
    vb = pyr_b.img[l][shb:, shb:]
    eps2, min_det = f32(f32(eps) * f32(eps)), f32(min_det)
    far2 = f32(P) if defect == "far psz" else f32(P * P)
    d = np.full((ny, nx, 2), np.nan, f32)
    status = np.zeros((ny, nx), np.uint8)

    for j, Y in enumerate(ys):
        for i, X in enumerate(xs):
            xl, yl = f32(X), f32(Y)
            ix, iy = init[j, i]
            sx, sy = f32(xl + ix), f32(yl + iy)
            if not (np.isfinite(ix) and np.isfinite(iy) and sx >= 0 and sy >= 0 and sx <= wl and sy <= hl):
                continue
            px, py, _, why = level_search(va, vax, vay, vb, wl, hl, xl, yl, ix, iy, P, maxiter, eps2, min_det, shape=shape)
            st = {STOP_NONE: TRACKED, STOP_COND: HELD_COND, STOP_VIEW: HELD_VIEW}[why]
            if st == TRACKED:
                ex, ey = f32(px - ix), f32(py - iy)
                if not (f32(f32(ex * ex) + f32(ey * ey)) <= far2):
                    st = HELD_FAR
            held = st >= HELD_COND
            if held and defect == "held lost":
                continue
            status[j, i] = st
            d[j, i] = (ix, iy) if held and defect != "held keeps p" else (px, py)
    return d, status == LOST, status


def fill(d, lost):
    """k_fg_rowfill, k_fg_colfill: a lost node takes the nearest kept node to its left in its row, else the nearest to its
    right; a row without one takes, node by node, the nearest row above that has one, else the nearest below, else 0."""
    ny, nx = lost.shape
    out = np.zeros((ny, nx, 2), f32)
    rowhas = ~lost.all(axis=1)
    for j in range(ny):
        kept = np.nonzero(~lost[j])[0]
        for i in range(nx if len(kept) else 0):
            left = kept[kept <= i]
            out[j, i] = d[j, left[-1] if len(left) else kept[0]]
    have = np.nonzero(rowhas)[0]
    for j in np.nonzero(~rowhas)[0]:
        above = have[have < j]
        if len(have):
            out[j] = out[above[-1] if len(above) else have[0]]
    return out


def level(pyr_a, pyr_b, l, coarse, step, psz, maxiter=10, eps=0.01, densify=None, refine=None, defect=None, init=None):
    """One level as ictr_c2fflow_run enqueues it: (field (h, w, 2), d after the fill, status). init: the starts, when they
    are not to be taken from `coarse` (the comparison with the definition level by level)."""
    w, h = level_size(pyr_a, l)
    if init is None:
        init = init_of(coarse, w, h, step, defect)
    d, lost, status = search(pyr_a, pyr_b, l, init, step, psz, maxiter, eps, defect=defect)
    filled = fill(d, lost)
    A, B = plane(pyr_a, l), plane(pyr_b, l)
    dz = dict(dict(minerr=2.0, power=1), **(densify or {}))
    field = DZ.densify(A, B, filled, lost, step, psz, dz["minerr"], dz["power"])
    if refine is not None:
        field = FR.refine(A, B, field, **refine)
    return field, filled, status


def run(pyr_a, pyr_b, step=4, psz=8, lv_f=2, maxiter=10, eps=0.01, densify=None, refine=None, defect=None, stages=None):
    """ictr_c2fflow_run: level 0's field (H, W, 2) f32. stages: a list that receives (level, field, d, status) per level
    from lv_f down."""
    field = None
    for l in range(lv_f, -1, -1):
        field, d, status = level(pyr_a, pyr_b, l, field, step, psz, maxiter, eps, densify, refine, defect)
        if stages is not None:
            stages.append((l, field, d, status))
    return field
