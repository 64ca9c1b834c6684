"""The coarse-to-fine dense flow on colour frames as the device computes it, restated in NumPy float32: the NCH = 3 forms of
pf_level_search_ch and pf_window_sum_ch (csrc/ictr_patchflow_dev.h), of k_c2f_level (csrc/ictr_c2fflow.hip) and
of k_densify (csrc/ictr_densify.hip). Written from the kernels. A frame is three pyramids; the search samples T, Gx, Gy
per channel with ONE set of taps; a lane adds channel 0, then 1, then 2 into the same accumulators (the pixels of a channel
in the grey slot order), then the wave tree and the wave order follow once (sum_ch); H and b are such sums, the decision
and the step are taken once. With patnorm every channel loses its own mean: the sums of T_c, of Gx_c (and Gy_c) and of I_c
are single-channel sums, b = s + sum_c (sum I_c / n) sum G_c with the channels added in order, and the tail takes
beta_c = sum(B_c at the final position) / n - mean(T_c). A vote weighs e = ((|r0| + |r1|) + |r2|) / 3.
The refinement's coefficient stage (k_fr_coef_rgb of csrc/ictr_flowrefine.hip) keeps n0, n1, n2 per channel, takes the two
robust weights on the channel means of their arguments and the coefficients as channel means, every channel sum from 0 in
the order 0, 1, 2 and every mean as a quotient by 3.
The unchanged pieces (taps, fetch, a channel's sum shape, the start, the fill, the fallback value, the up-sampling, the
warp, the tiles and their derivative rules, the half-sweeps) are those of patchflow_f32.py, c2fflow_f32.py,
densify_f32.py, c2fup_f32.py and flowrefine_f32.py.

The CPU module measures its distance to patchflow.c2f_flow_host on triples (the definition, f64); the GPU tests demand its
bits of the device.

`defect` injects one mistake a kernel of this shape can make; test_c2frgb_cpu.py shows that each is seen:
  "one channel thrice"   channel 0 is read three times, in both frames
  "H from channel 0"     H is summed over channel 0 alone (b over all three)
  "B order"              frame B's channels are read in the order 2, 1, 0
  "beta shifted"         the vote takes beta of channel c off channel c + 1's residual
  "vote sum"             the vote weighs the sum of the three absolute residuals, not their mean
  "robust without third" the refinement's two robust arguments are the channel sums, not the channel means
"""
from __future__ import annotations

import numpy as np

import c2fflow_f32 as C2
import c2fup_f32 as UP
import densify_f32 as DZ
import flowrefine_f32 as FR
from patchflow_f32 import ONE, STOP_COND, STOP_NONE, STOP_VIEW, ZERO, _fetch, _sum, _taps, f32

DEFECTS = ("one channel thrice", "H from channel 0", "B order", "beta shifted", "vote sum", "robust without third")
LOST, TRACKED, HELD_COND, HELD_VIEW, HELD_FAR = range(5)
MIN_DET, MIN_HX = 1e-4, 1e-2
F = np.float32


def sum_ch(terms_c, shape):
    """One patch sum over the channels: a lane's accumulator takes its slots of channel 0, then of 1, then of 2; the 64
    lanes meet in the pairwise tree, the waves in their order (patchflow_f32._sum's shape, the channels in front)."""
    npl, wpp = shape
    acc = np.zeros((wpp, 64), f32)
    for terms in terms_c:
        slots = np.zeros(64 * npl * wpp, f32)
        slots[:len(terms)] = terms
        slots = slots.reshape(npl, wpp, 64)
        for i in range(npl):
            acc = acc + slots[i]
    for _ in range(6):
        acc = acc[:, 0::2] + acc[:, 1::2]
    assert acc.dtype == f32 and acc.shape == (wpp, 1)
    tot = acc[0, 0]
    for q in range(1, wpp):
        tot = f32(tot + acc[q, 0])
    return tot


def level_search_rgb(A, vb, wl, hl, xl, yl, px, py, P, maxiter, eps2, min_cond, x_only, mean, shape, defect=None):
    """pf_level_search_ch<NPL, WPP, x_only, mean, 3> for one patch. A: per channel (va, vax, vay), vb: per channel the
    plane of frame B, all views padded by exactly P. Returns (px, py, iterations, STOP_*, [mean(T_c)])."""
    n = f32(P * P)
    ta = _taps(xl, yl, P, None)
    T = [_fetch(a[0], ta, P) for a in A]
    Gx = [_fetch(a[1], ta, P) for a in A]
    Gy = [_fetch(a[2], ta, P) for a in A]
    hc = (0,) if defect == "H from channel 0" else (0, 1, 2)
    hxx, hyy = sum_ch([Gx[c] * Gx[c] for c in hc], shape), sum_ch([Gy[c] * Gy[c] for c in hc], shape)
    mean_t = [ZERO] * 3
    if mean:
        mean_t = [f32(_sum(T[c], shape, None) / n) for c in range(3)]
        T = [T[c] - mean_t[c] for c in range(3)]
    tr = f32(hxx + hyy)
    if x_only:
        refused = not (tr > 0) or not (hxx > f32(min_cond * tr))
        div = hxx
    else:
        hxy = sum_ch([Gx[c] * Gy[c] for c in hc], shape)
        div = f32(f32(hxx * hyy) - f32(hxy * hxy))
        refused = not (div > f32(f32(min_cond * tr) * tr)) or not (tr > 0)
    if refused:
        return px, py, 0, STOP_COND, mean_t
    if mean:
        sgx = [_sum(Gx[c], shape, None) for c in range(3)]
        sgy = [_sum(Gy[c], shape, None) for c in range(3)]
    with np.errstate(over="ignore"):
        inv = f32(ONE / div)
    for nit in range(maxiter):
        cx, cy = f32(xl + px), (yl if x_only else f32(yl + py))
        if not (cx >= 0 and cy >= 0 and cx <= wl and cy <= hl):
            return px, py, nit, STOP_VIEW, mean_t
        tb = _taps(cx, cy, P, None)
        I = [_fetch(v, tb, P) for v in vb]
        r = [T[c] - I[c] for c in range(3)]
        assert r[0].dtype == f32
        bx = sum_ch([Gx[c] * r[c] for c in range(3)], shape)
        by = ZERO if x_only else sum_ch([Gy[c] * r[c] for c in range(3)], shape)
        if mean:
            for c in range(3):
                mi = f32(_sum(I[c], shape, None) / n)
                bx = f32(bx + f32(mi * sgx[c]))
                if not x_only:
                    by = f32(by + f32(mi * sgy[c]))
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


def _views(pyrs_a, pyrs_b, l, P, defect):
    ca = (0, 0, 0) if defect == "one channel thrice" else (0, 1, 2)
    cb = (0, 0, 0) if defect == "one channel thrice" else (2, 1, 0) if defect == "B order" else (0, 1, 2)
    A = []
    for c in ca:
        p, sh = pyrs_a[c], pyrs_a[c].pad - P
        A.append(tuple(q[sh:, sh:] for q in (p.img[l], p.dx[l], p.dy[l])))
    vb = [pyrs_b[c].img[l][pyrs_b[c].pad - P:, pyrs_b[c].pad - P:] for c in cb]
    return A, vb


def search(pyrs_a, pyrs_b, l, init, step, psz, maxiter=10, eps=0.01, patnorm=False, x_only=False, defect=None):
    """k_c2f_level<NPL, WPP, patnorm, x_only, 3> for one node after the other: (d before the fill (ny, nx, 2) f32, NaN at a
    lost node; lost (ny, nx) bool; status (ny, nx) uint8; bias (ny, nx, 3) f32, None without patnorm)."""
    P = psz
    shape = C2.form_shape(P)
    w, h = C2.level_size(pyrs_a[0], l)
    wl, hl = f32(w), f32(h)
    xs, ys = np.arange(step // 2, w, step), np.arange(step // 2, h, step)
    ny, nx = len(ys), len(xs)
    A, vb = _views(pyrs_a, pyrs_b, l, P, defect)
    eps2, min_cond = f32(f32(eps) * f32(eps)), f32(MIN_HX if x_only else MIN_DET)
    far2 = f32(P * P)
    d = np.full((ny, nx, 2), np.nan, f32)
    status = np.zeros((ny, nx), np.uint8)
    bias = np.zeros((ny, nx, 3), f32) if patnorm else None

    for j, Y in enumerate(ys):
        for i, X in enumerate(xs):
            xl, yl = f32(X), f32(Y)
            ix, iy = init[j, i]
            sx, sy = f32(xl + ix), f32(yl + iy)
            if not (np.isfinite(ix) and np.isfinite(iy) and sx >= 0 and sy >= 0 and sx <= wl and sy <= hl):
                continue
            px, py, _, why, mean_t = level_search_rgb(A, vb, wl, hl, xl, yl, ix, iy, P, maxiter, eps2, min_cond, x_only,
                                                      patnorm, shape, defect)
            st = {STOP_NONE: TRACKED, STOP_COND: HELD_COND, STOP_VIEW: HELD_VIEW}[why]
            if st == TRACKED:
                ex, ey = f32(px - ix), f32(py - iy)
                far = f32(ex * ex) if x_only else f32(f32(ex * ex) + f32(ey * ey))
                if not (far <= far2):
                    st = HELD_FAR
            held = st >= HELD_COND
            status[j, i] = st
            d[j, i] = (ix, iy) if held else (px, py)
            if patnorm:  # the tail: one more window pass of the three channels of B at the final position
                fx, fy = f32(xl + d[j, i, 0]), f32(yl + d[j, i, 1])
                if fx >= 0 and fy >= 0 and fx <= wl and fy <= hl:
                    tb = _taps(fx, fy, P, None)
                    for c in range(3):
                        sb = _sum(_fetch(vb[c], tb, P), shape, None)
                        bias[j, i, c] = f32(f32(sb / f32(P * P)) - mean_t[c])
    return d, status == LOST, status, bias


def densify(img_a, img_b, d_filled, lost, bias, step, psz, minerr=2.0, power=1, defect=None):
    """k_densify<bias is not None, 3>: img_a, img_b (3, H, W); bias (ny, nx, 3) or None. (H, W, 2) f32."""
    A, B = np.ascontiguousarray(img_a, F), np.ascontiguousarray(img_b, F)
    d = np.ascontiguousarray(d_filled, F)
    lost = np.asarray(lost).astype(bool)
    h, w = A.shape[1:]
    ny, nx = lost.shape
    half = step // 2
    lo, hi = psz - psz // 2, psz // 2 - 1
    xs, ys = np.arange(w), np.arange(h)
    i0, i1 = DZ.first_node(xs - hi - half, step), DZ.last_node(xs + lo - half, step, nx)
    j0, j1 = DZ.first_node(ys - hi - half, step), DZ.last_node(ys + lo - half, step, ny)
    rec = d.copy()
    rec[lost, 0] = np.nan
    beta = None if bias is None else np.ascontiguousarray(bias, F)
    if beta is not None and defect == "beta shifted":
        beta = np.roll(beta, 1, axis=2)
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
                r = []
                for c in range(3):
                    rc = DZ.bilinear(B[c], px, py) - A[c]
                    if beta is not None:
                        rc = rc - beta[j][:, i, c]
                    r.append(np.abs(rc))
                e = (r[0] + r[1]) + r[2]
                if defect != "vote sum":
                    e = e / F(3)
                m = np.fmax(e, me)
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


def coef(A, bw, u, v, alpha, gamma, delta, defect=None):
    """k_fr_coef_rgb: (a11, a12, a22, b1, b2, wr, wd), f32, tile by tile. A, bw: (3, h, w). Every sum over the channels
    starts from 0 and adds channel 0, 1, 2; the means are quotients by 3."""
    h, w = A.shape[1:]
    alpha, gamma, delta = F(alpha), F(gamma), F(delta)
    outs = [np.zeros((h, w), F) for _ in range(7)]
    one, half, three = F(1), F(0.5), F(3)
    T_, H_ = FR.TILE, FR.HALO
    for ty in range(0, h, T_):
        for tx in range(0, w, T_):
            gx0, gy0 = tx - H_, ty - H_
            T = FR._T(gx0, gy0, w, h)
            tu, tv = FR._tile(u, gx0, gy0, H_), FR._tile(v, gx0, gy0, H_)
            X, Y = gx0 + np.arange(T_ + 2 * H_), gy0 + np.arange(T_ + 2 * H_)
            px, py = X.astype(F)[None, :] + tu, Y.astype(F)[:, None] + tv
            with np.errstate(invalid="ignore"):
                ins = (px >= 0) & (px <= F(w - 1)) & (py >= 0) & (py <= F(h - 1))
            ch = []
            s0, sg = np.zeros_like(tu), np.zeros_like(tu)
            for c in range(3):
                tb, ta = FR._tile(bw[c], gx0, gy0, H_), FR._tile(A[c], gx0, gy0, H_)
                Ix, Iy, Iz = T.dx(tb), T.dy(tb), tb - ta
                Ixx, Ixy, Iyy = T.dx(Ix), T.dy(Ix), T.dy(Iy)
                Ixz, Iyz = Ix - T.dx(ta), Iy - T.dy(ta)
                n0 = one / ((Ix * Ix + Iy * Iy) + FR.ZETA2)
                n1 = one / ((Ixx * Ixx + Ixy * Ixy) + FR.ZETA2)
                n2 = one / ((Ixy * Ixy + Iyy * Iyy) + FR.ZETA2)
                s0 = s0 + (n0 * Iz) * Iz
                sg = sg + ((n1 * Ixz) * Ixz + (n2 * Iyz) * Iyz)
                ch.append((Ix, Iy, Iz, Ixx, Ixy, Iyy, Ixz, Iyz, n0, n1, n2))
            if defect != "robust without third":
                s0, sg = s0 / three, sg / three
            q0 = np.where(ins, (delta * half) / np.sqrt(s0 + FR.EPS2), F(0))
            qg = np.where(ins, (gamma * half) / np.sqrt(sg + FR.EPS2), F(0))
            a11, a12, a22, b1, b2 = (np.zeros_like(tu) for _ in range(5))
            for Ix, Iy, Iz, Ixx, Ixy, Iyy, Ixz, Iyz, n0, n1, n2 in ch:
                w0 = q0 * n0
                a11 = a11 + (w0 * (Ix * Ix) + qg * (n1 * (Ixx * Ixx) + n2 * (Ixy * Ixy)))
                a12 = a12 + (w0 * (Ix * Iy) + qg * (n1 * (Ixx * Ixy) + n2 * (Ixy * Iyy)))
                a22 = a22 + (w0 * (Iy * Iy) + qg * (n1 * (Ixy * Ixy) + n2 * (Iyy * Iyy)))
                b1 = b1 + (w0 * (Ix * Iz) + qg * (n1 * (Ixx * Ixz) + n2 * (Ixy * Iyz)))
                b2 = b2 + (w0 * (Iy * Iz) + qg * (n1 * (Ixy * Ixz) + n2 * (Iyy * Iyz)))
            a11, a12, a22, b1, b2 = a11 / three, a12 / three, a22 / three, -(b1 / three), -(b2 / three)
            assert a11.dtype == F and q0.dtype == F
            ux, uy, vx, vy = T.dx(tu), T.dy(tu), T.dx(tv), T.dy(tv)
            t = ux * ux + uy * uy
            t = t + vx * vx
            t = t + vy * vy
            t = t + FR.EPS2
            s = (alpha * half) / np.sqrt(t)
            wr, wd = np.zeros_like(s), np.zeros_like(s)
            wr[:, :-1] = half * (s[:, :-1] + s[:, 1:])
            wd[:-1, :] = half * (s[:-1, :] + s[1:, :])
            wr = np.where((X < w - 1)[None, :], wr, F(0))
            wd = np.where((Y < h - 1)[:, None], wd, F(0))
            y1, x1 = min(ty + T_, h), min(tx + T_, w)
            cut = (slice(H_, H_ + y1 - ty), slice(H_, H_ + x1 - tx))
            for k, p in enumerate((a11, a12, a22, b1, b2, wr, wd)):
                outs[k][ty:y1, tx:x1] = p[cut]
    return tuple(outs)


def refine(img_a, img_b, flow, alpha=16.0, gamma=13.0, delta=4.5, n_outer=8, n_sor=5, omega=1.6, x_only=False,
           defect=None):
    """ictr_flowrefine_run_level_ on three channels: (H, W, 2) f32; img_a, img_b (3, H, W). k_fr_warp<3> is
    flowrefine_f32.warp per channel, the half-sweeps are the grey ones."""
    A, B = np.ascontiguousarray(img_a, F), np.ascontiguousarray(img_b, F)
    f0 = np.ascontiguousarray(flow, F)
    if n_outer == 0:
        return f0.copy()
    u, v = f0[..., 0].copy(), f0[..., 1].copy()
    du = dv = None
    for o in range(n_outer):
        if o > 0:
            u = u + du
            if not x_only:
                v = v + dv
        bw = np.stack([FR.warp(B[c], u, v) for c in range(3)])
        cf = coef(A, bw, u, v, alpha, gamma, delta, defect)
        du, dv = np.zeros_like(u), np.zeros_like(v)
        for _ in range(n_sor):
            for colour in (0, 1):
                FR.half_sweep(colour, omega, x_only, u, v, du, dv, *cf)
    out = np.empty_like(f0)
    out[..., 0] = u + du
    out[..., 1] = v if x_only else v + dv
    return out


def planes(pyrs, l):
    return np.stack([C2.plane(p, l) for p in pyrs])


def level(pyrs_a, pyrs_b, l, coarse, step, psz, maxiter=10, eps=0.01, densify_params=None, patnorm=False, x_only=False,
          defect=None, init=None, refine_params=None):
    """One level as ictr_c2fflow_run_rgb enqueues it: (field (h, w, 2), d after the fill, status, bias or None)."""
    w, h = C2.level_size(pyrs_a[0], l)
    if init is None:
        init = C2.init_of(coarse, w, h, step).copy()
        if x_only:
            init[..., 1] = ZERO
    d, lost, status, bias = search(pyrs_a, pyrs_b, l, init, step, psz, maxiter, eps, patnorm, x_only, defect)
    filled = C2.fill(d, lost)
    ca = (0, 0, 0) if defect == "one channel thrice" else (0, 1, 2)
    cb = (2, 1, 0) if defect == "B order" else ca
    A, B = planes([pyrs_a[c] for c in ca], l), planes([pyrs_b[c] for c in cb], l)
    dz = dict(dict(minerr=2.0, power=1), **(densify_params or {}))
    field = densify(A, B, filled, lost, bias, step, psz, dz["minerr"], dz["power"], defect)
    if refine_params is not None:
        field = refine(A, B, field, x_only=x_only, defect=defect, **refine_params)
    return field, filled, status, bias


def run(pyrs_a, pyrs_b, step=4, psz=8, lv_f=2, lv_l=0, maxiter=10, eps=0.01, densify_params=None, patnorm=False,
        x_only=False, defect=None, stages=None, refine_params=None):
    """ictr_c2fflow_run_rgb: the (H, W, 2) f32 result. stages: a list that receives (level, field, d, status, bias) per
    level from lv_f down to lv_l."""
    field = None
    for l in range(lv_f, lv_l - 1, -1):
        field, d, status, bias = level(pyrs_a, pyrs_b, l, field, step, psz, maxiter, eps, densify_params, patnorm, x_only,
                                       defect, refine_params=refine_params)
        if stages is not None:
            stages.append((l, field, d, status, bias))
    if lv_l == 0:
        return field
    w, h = C2.level_size(pyrs_a[0], 0)
    return UP.upsample(field, w, h, lv_l, x_only)
