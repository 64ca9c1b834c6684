"""The variational refinement as csrc/ictr_flowrefine.hip computes it, restated in NumPy float32: the same expressions in
the kernels' operation order (every product and sum rounded to f32, nothing contracted), the coefficient stage tile by
tile with the kernel's 16 x 16 tiles and 2-pixel halo. It is written from the kernel, not from the host function: the
CPU module measures its distance to patchflow.refine_flow_host (the definition, f64), and the GPU tests hold the device
to 4 x that distance and, stage plane by stage plane, to this file's bits.

`defect` injects one mistake a kernel of this shape can make; test_flowrefine_cpu.py shows that each is seen:
  "colour"   the half-sweeps run colour 1 first
  "old_du"   the dv update uses the du of before the half-sweep
  "halo1"    the coefficient tile is loaded with a 1-pixel halo (what lies beyond repeats the halo's edge)
  "inside"   the inside mask is left out of the data weights
  "edge"     an edge weight is its own pixel's s, not the mean of the two
  "clamp"    the warp position is not clamped (the taps are, so that the restatement can still index)
and two that the tolerances of the stage checks need not see and a comparison of bits does:
  "fused"    a11, a12, a22 with their outer sum contracted: w0 * (..) + wg * (..) as one product-sum rounded once (formed
             in f64, where both products of f32 factors are exact), which is what a build that lost -ffp-contract=off does
  "border2"  the second derivatives are also zero in column / row 1 and w - 2 / h - 2
"""
from __future__ import annotations

import numpy as np

F = np.float32
TILE, HALO = 16, 2
EPS2 = F(1e-3) * F(1e-3)
ZETA2 = F(0.1) * F(0.1)
DEFECTS = ("colour", "old_du", "halo1", "inside", "edge", "clamp", "fused", "border2")
STAGES = ("bw", "a11", "a12", "a22", "b1", "b2", "wr", "wd", "du", "dv", "u", "v")


def warp(B, u, v, defect=None):
    """k_fr_warp without the fold: Bw (f32)."""
    h, w = B.shape
    yy, xx = np.mgrid[0:h, 0:w]
    px = xx.astype(F) + u
    py = yy.astype(F) + v
    if defect != "clamp":
        px = np.fmin(np.fmax(px, F(0)), F(w - 1))
        py = np.fmin(np.fmax(py, F(0)), F(h - 1))
    with np.errstate(invalid="ignore"):
        x0 = np.clip(np.floor(np.nan_to_num(px)).astype(np.int64), 0, w - 2)
        y0 = np.clip(np.floor(np.nan_to_num(py)).astype(np.int64), 0, h - 2)
    fx, fy = px - x0.astype(F), py - y0.astype(F)
    one = F(1)
    w00, w01, w10, w11 = (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy
    return ((w00 * B[y0, x0] + w01 * B[y0, x0 + 1]) + w10 * B[y0 + 1, x0]) + w11 * B[y0 + 1, x0 + 1]


def inside_mask(u, v):
    h, w = u.shape
    yy, xx = np.mgrid[0:h, 0:w]
    px, py = xx.astype(F) + u, yy.astype(F) + v
    with np.errstate(invalid="ignore"):
        return (px >= 0) & (px <= F(w - 1)) & (py >= 0) & (py <= F(h - 1))


def _tile(p, gx0, gy0, halo):
    """FrTile's LDS array: (TILE + 2 HALO)^2 values read at the nearest pixel of the frame; with halo < HALO what lies
    beyond the loaded halo repeats its edge."""
    h, w = p.shape
    side = TILE + 2 * HALO
    cy = np.arange(side) + gy0
    cx = np.arange(side) + gx0
    lo = HALO - halo
    cy = np.clip(cy, gy0 + lo, gy0 + side - 1 - lo)
    cx = np.clip(cx, gx0 + lo, gx0 + side - 1 - lo)
    return p[np.clip(cy, 0, h - 1)][:, np.clip(cx, 0, w - 1)]


class _T:
    """The derivative rules of FrTile on a tile array: 0 in the frame's first and last column / row."""

    def __init__(self, gx0, gy0, w, h):
        side = TILE + 2 * HALO
        X, Y = gx0 + np.arange(side), gy0 + np.arange(side)
        self.bx = ((X <= 0) | (X >= w - 1))[None, :]
        self.by = ((Y <= 0) | (Y >= h - 1))[:, None]
        self.bx2 = ((X <= 1) | (X >= w - 2))[None, :]  # the "border2" defect
        self.by2 = ((Y <= 1) | (Y >= h - 2))[:, None]

    def dx(self, p):
        out = np.zeros_like(p)
        out[:, 1:-1] = F(0.5) * (p[:, 2:] - p[:, :-2])
        return np.where(self.bx, F(0), out)

    def dy(self, p):
        out = np.zeros_like(p)
        out[1:-1, :] = F(0.5) * (p[2:, :] - p[:-2, :])
        return np.where(self.by, F(0), out)


def _fused(a, b, c, d):
    """a * b + c * d rounded once."""
    f64 = np.float64
    return (a.astype(f64) * b.astype(f64) + c.astype(f64) * d.astype(f64)).astype(F)


def coef(A, bw, u, v, alpha, gamma, delta, defect=None):
    """k_fr_coef: (a11, a12, a22, b1, b2, wr, wd), f32, tile by tile."""
    h, w = A.shape
    alpha, gamma, delta = F(alpha), F(gamma), F(delta)
    halo = 1 if defect == "halo1" else HALO
    outs = [np.zeros((h, w), F) for _ in range(7)]
    one, half = F(1), F(0.5)
    for ty in range(0, h, TILE):
        for tx in range(0, w, TILE):
            gx0, gy0 = tx - HALO, ty - HALO
            T = _T(gx0, gy0, w, h)
            tb, ta, tu, tv = (_tile(p, gx0, gy0, halo) for p in (bw, A, u, v))
            Ix, Iy, Iz = T.dx(tb), T.dy(tb), tb - ta
            Ixx, Ixy, Iyy = T.dx(Ix), T.dy(Ix), T.dy(Iy)
            if defect == "border2":
                Ixx, Ixy, Iyy = np.where(T.bx2, F(0), Ixx), np.where(T.by2, F(0), Ixy), np.where(T.by2, F(0), Iyy)
            Ixz, Iyz = Ix - T.dx(ta), Iy - T.dy(ta)
            n0 = one / ((Ix * Ix + Iy * Iy) + ZETA2)
            n1 = one / ((Ixx * Ixx + Ixy * Ixy) + ZETA2)
            n2 = one / ((Ixy * Ixy + Iyy * Iyy) + ZETA2)
            X, Y = gx0 + np.arange(TILE + 2 * HALO), gy0 + np.arange(TILE + 2 * HALO)
            px, py = X.astype(F)[None, :] + tu, Y.astype(F)[:, None] + tv
            with np.errstate(invalid="ignore"):
                ins = (px >= 0) & (px <= F(w - 1)) & (py >= 0) & (py <= F(h - 1))
            if defect == "inside":
                ins = np.ones_like(ins)
            w0 = np.where(ins, ((delta * n0) * half) / np.sqrt((n0 * Iz) * Iz + EPS2), F(0))
            wg = np.where(ins, (gamma * half) / np.sqrt(((n1 * Ixz) * Ixz + (n2 * Iyz) * Iyz) + EPS2), F(0))
            a11 = w0 * (Ix * Ix) + wg * (n1 * (Ixx * Ixx) + n2 * (Ixy * Ixy))
            a12 = w0 * (Ix * Iy) + wg * (n1 * (Ixx * Ixy) + n2 * (Ixy * Iyy))
            a22 = w0 * (Iy * Iy) + wg * (n1 * (Ixy * Ixy) + n2 * (Iyy * Iyy))
            if defect == "fused":
                a11, a12, a22 = (_fused(w0, p, wg, q) for p, q in ((Ix * Ix, n1 * (Ixx * Ixx) + n2 * (Ixy * Ixy)),
                                                                   (Ix * Iy, n1 * (Ixx * Ixy) + n2 * (Ixy * Iyy)),
                                                                   (Iy * Iy, n1 * (Ixy * Ixy) + n2 * (Iyy * Iyy))))
            b1 = -(w0 * (Ix * Iz) + wg * (n1 * (Ixx * Ixz) + n2 * (Ixy * Iyz)))
            b2 = -(w0 * (Iy * Iz) + wg * (n1 * (Ixy * Ixz) + n2 * (Iyy * Iyz)))
            ux, uy, vx, vy = T.dx(tu), T.dy(tu), T.dx(tv), T.dy(tv)
            t = ux * ux + uy * uy
            t = t + vx * vx
            t = t + vy * vy
            t = t + EPS2
            s = (alpha * half) / np.sqrt(t)
            wr, wd = np.zeros_like(s), np.zeros_like(s)
            if defect == "edge":
                wr[:, :-1], wd[:-1, :] = s[:, :-1], s[:-1, :]
            else:
                wr[:, :-1] = half * (s[:, :-1] + s[:, 1:])
                wd[:-1, :] = half * (s[:-1, :] + s[1:, :])
            wr = np.where((X < w - 1)[None, :], wr, F(0))
            wd = np.where((Y < h - 1)[:, None], wd, F(0))
            y1, x1 = min(ty + TILE, h), min(tx + TILE, w)
            c = (slice(HALO, HALO + y1 - ty), slice(HALO, HALO + x1 - tx))
            for k, p in enumerate((a11, a12, a22, b1, b2, wr, wd)):
                outs[k][ty:y1, tx:x1] = p[c]
    return tuple(outs)


def _shift(a):
    p = np.pad(a, 1)
    return p[1:-1, :-2], p[1:-1, 2:], p[:-2, 1:-1], p[2:, 1:-1]


def half_sweep(colour, omega, x_only, u, v, du, dv, a11, a12, a22, b1, b2, wr, wd, defect=None):
    """k_fr_sor<colour>, in place on du / dv (f32 arrays)."""
    h, w = u.shape
    om, one = F(omega), F(1)
    yy, xx = np.mgrid[0:h, 0:w]
    m = ((xx + yy) & 1) == colour
    wl, wu = _shift(wr)[0], _shift(wd)[2]
    # beyond the frame the kernel adds the constant 0; here the weight and the padded value are both 0
    wrr = np.where(xx < w - 1, wr, F(0))
    wdd = np.where(yy < h - 1, wd, F(0))
    sw = ((wl + wrr) + wu) + wdd
    ul, ur, uu, ud = _shift(u + du)
    su = ((wl * ul + wrr * ur) + wu * uu) + wdd * ud
    dun = (one - om) * du + om * ((((b1 - a12 * dv) + su) - sw * u) / (a11 + sw))
    du_old = du.copy()
    du[m] = dun[m]
    if x_only:
        return
    vl, vr, vu, vd = _shift(v + dv)
    sv = ((wl * vl + wrr * vr) + wu * vu) + wdd * vd
    dux = du_old if defect == "old_du" else du
    dvn = (one - om) * dv + om * ((((b2 - a12 * dux) + sv) - sw * v) / (a22 + sw))
    dv[m] = dvn[m]


def refine(img_a, img_b, flow, alpha=16.0, gamma=13.0, delta=4.5, n_outer=8, n_sor=5, omega=1.6, x_only=False,
           defect=None, trace=None):
    """ictr_flowrefine_run: (H, W, 2) f32. trace: a list that receives the stage planes of each outer iteration."""
    A, B = np.ascontiguousarray(img_a, F), np.ascontiguousarray(img_b, F)
    f0 = np.ascontiguousarray(flow, F)
    if n_outer == 0:
        return f0.copy()
    u, v = f0[..., 0].copy(), f0[..., 1].copy()
    du = dv = None
    for o in range(n_outer):
        if o > 0:  # step 6, folded into the warp
            u = u + du
            if not x_only:
                v = v + dv
        bw = warp(B, u, v, defect)
        c = coef(A, bw, u, v, alpha, gamma, delta, defect)
        du, dv = np.zeros_like(u), np.zeros_like(v)
        for _ in range(n_sor):
            for colour in ((1, 0) if defect == "colour" else (0, 1)):
                half_sweep(colour, omega, x_only, u, v, du, dv, *c, defect=defect)
        if trace is not None:
            trace.append(dict(zip(STAGES, (bw,) + c + (du.copy(), dv.copy(), u.copy(), v.copy()))))
    out = np.empty_like(f0)
    out[..., 0] = u + du
    out[..., 1] = v if x_only else v + dv
    return out
