"""The densification of a flow grid as csrc/ictr_densify.hip computes it, restated in NumPy float32: the same expressions
in the kernel's operation order (every product, sum and quotient rounded to f32, nothing contracted), a lane's loop over
its covering nodes in ascending node row, then column, taken for all pixels at once; the mean about the first vote,
d0 + sum(wgt (d - d0)) / sum(wgt), as the kernel takes it. It is written from the kernel, not
from the host function: the CPU module measures its distance to patchflow.densify_flow_host (the definition, f64), and the
GPU tests demand its bits of the device.

`defect` injects one mistake a kernel of this shape can make; test_densify_cpu.py shows that each is seen:
  "lost"      lost nodes vote (with their filled value)
  "footprint" the footprint is the symmetric X - psz // 2 .. X + psz // 2
  "order"     the votes are summed in descending node row and column
  "inside"    no inside test: a vote that leaves the frame is taken at the clamped position
  "fallback"  a pixel without a vote takes 0, not the grid's up-sampled value
  "minerr"    minerr is not applied (a residual of 0 is kept off the division by the smallest normal number)
"""
from __future__ import annotations

import numpy as np

F = np.float32
DEFECTS = ("lost", "footprint", "order", "inside", "fallback", "minerr")


def first_node(a, step):
    """dz_first: the least i >= 0 with a <= i step."""
    return np.where(a <= 0, 0, (a + step - 1) // step)


def last_node(b, step, n):
    """dz_last: the greatest i <= n - 1 with i step <= b, -1 without one."""
    return np.where(b < 0, -1, np.minimum(b // step, n - 1))


def bilinear(B, px, py):
    """fr_bilinear (ictr_warp_dev.h): clamp, taps min(floor, w - 2), the four weights and their order."""
    h, w = B.shape
    px = np.fmin(np.fmax(px, F(0)), F(w - 1))
    py = np.fmin(np.fmax(py, F(0)), F(h - 1))
    x0 = np.minimum(np.floor(px).astype(np.int64), w - 2)
    y0 = np.minimum(np.floor(py).astype(np.int64), h - 2)
    fx, fy = px - x0.astype(F), py - y0.astype(F)
    one = F(1)
    w00, w01, w10, w11 = (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy
    return ((w00 * B[y0, x0] + w01 * B[y0, x0 + 1]) + w10 * B[y0 + 1, x0]) + w11 * B[y0 + 1, x0 + 1]


def fg_value(d, w, h, step):
    """fg_value (ictr_flowgrid_dev.h) at every pixel from the filled node table d (ny, nx, 2): f64 blend, rounded once."""
    ny, nx = d.shape[:2]
    half = step // 2
    fx = np.fmin(np.fmax((np.arange(w) - half).astype(np.float64) / float(step), 0.0), float(nx - 1))
    fy = np.fmin(np.fmax((np.arange(h) - half).astype(np.float64) / float(step), 0.0), float(ny - 1))
    x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, nx - 1), np.minimum(y0 + 1, ny - 1)
    ax, ay = (fx - x0)[None, :, None], (fy - y0)[:, None, None]
    d = d.astype(np.float64)
    top = d[y0][:, x0] * (1 - ax) + d[y0][:, x1] * ax
    bot = d[y1][:, x0] * (1 - ax) + d[y1][:, x1] * ax
    return (top * (1 - ay) + bot * ay).astype(F)


def densify(img_a, img_b, d_filled, lost, step, psz, minerr=2.0, power=1, defect=None, stages=None):
    """k_densify: (H, W, 2) f32. d_filled: the grid's node table AFTER its fill (FlowGrid.nodes), lost: its mask.
    stages: a dict that receives "count" and "wsum" (f32 planes)."""
    A, B = np.ascontiguousarray(img_a, F), np.ascontiguousarray(img_b, F)
    d = np.ascontiguousarray(d_filled, F)
    lost = np.asarray(lost).astype(bool)
    h, w = A.shape
    ny, nx = lost.shape
    half = step // 2
    lo, hi = psz - psz // 2, psz // 2 - 1
    if defect == "footprint":
        lo, hi = psz // 2, psz // 2
    xs, ys = np.arange(w), np.arange(h)
    i0, i1 = first_node(xs - hi - half, step), last_node(xs + lo - half, step, nx)
    j0, j1 = first_node(ys - hi - half, step), last_node(ys + lo - half, step, ny)
    rec = d.copy()  # the LDS record: a lost node has dx = NaN
    if defect != "lost":
        rec[lost, 0] = np.nan
    yy, xx = np.mgrid[0:h, 0:w]
    xf, yf = xx.astype(F), yy.astype(F)
    su, sv, sw = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
    d0x, d0y = np.zeros((h, w), F), np.zeros((h, w), F)  # the first vote's displacement
    cnt = np.zeros((h, w), np.int32)
    me = F(minerr) if defect != "minerr" else np.finfo(F).tiny
    na, nb = max(int((j1 - j0).max()) + 1, 0), max(int((i1 - i0).max()) + 1, 0)
    with np.errstate(invalid="ignore"):
        for a in range(na):
            jr = j1 - a if defect == "order" else j0 + a
            vj = (jr >= j0) & (jr <= j1)
            j = np.clip(jr, 0, ny - 1)
            for b in range(nb):
                ir = i1 - b if defect == "order" else i0 + b
                vi = (ir >= i0) & (ir <= i1)
                i = np.clip(ir, 0, nx - 1)
                dx, dy = rec[j][:, i, 0], rec[j][:, i, 1]
                px, py = xf + dx, yf + dy
                inside = (px >= F(0)) & (px <= F(w - 1)) & (py >= F(0)) & (py <= F(h - 1))
                if defect == "inside":
                    inside = ~np.isnan(px) & ~np.isnan(py)
                ok = vj[:, None] & vi[None, :] & inside
                r = bilinear(B, px, py) - A
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
    out = fg_value(d, w, h, step)
    if defect == "fallback":
        out[...] = 0
    with np.errstate(invalid="ignore", divide="ignore"):
        out[..., 0] = np.where(cnt > 0, d0x + su / sw, out[..., 0])
        out[..., 1] = np.where(cnt > 0, d0y + sv / sw, out[..., 1])
    assert out.dtype == F and su.dtype == F and sw.dtype == F
    if stages is not None:
        stages.update(count=cnt.astype(F), wsum=sw)
    return out
