"""NumPy restatement of the per-patch translation IC-LK of invcompcamtrack_amd/csrc/ictr_patchflow.hip.

TEST INFRASTRUCTURE ONLY. The algorithm is build-defined (the reference obtains flow from an external binary that is
not in its repository), so this oracle pins the HIP kernel against an independent implementation, not against the
reference: "parity unpinned by the reference". Sampling = util_getPatch's convention (np_oracle.patches) except for the
first tap, which is floor(x) + 1 here and ceil(x + 1e-5f) there: the two differ at integer x >= 256 and one ulp below an
integer <= 64, where f32 rounds that sum across an integer and the reference's taps are not the pair its weights mean.

The sampling (_sample) takes (p + psz // 2) for the patch's first pixel, which holds in a plane padded by exactly psz. A
pyramid padded by more (pad >= psz is the contract) is sampled through the view plane[pad - psz:, pad - psz:], whose
pixel (0, 0) sits where a plane padded by psz has it.

Error bound of an f32 evaluation of one step (one_step, and summed over a run by track_points(detail=True)), first
order, u = 2^-24, for a kernel form that adds L pixels per lane with WPP waves per patch:

    per pixel   every bilinear value v = sum w_k v_k carries e(v) = 3 u sum w_k |v_k| (the taps are the shared pyramid's,
                the weights the same f32 expressions); r = T - I carries e(r) = e(T) + e(I) + u |r|
    per sum     S = (L + c) u sum |term|, c = 1 (the product) + 6 (DPP levels: two quad steps, half row, row, and the two
                levels of the four-row sum) + (WPP - 1) (the partner wave's partial): 7 or 8
    H           d hxx = sum 2 |Gx| e(Gx) + S(Gx Gx), d hyy alike, d hxy = sum (|Gx| e(Gy) + |Gy| e(Gx)) + S(Gx Gy)
    b           d bx = sum (e(Gx) |r| + |Gx| e(r)) + S(Gx r), d by alike
    solve       det = hxx hyy - hxy^2:  d det = hyy d hxx + hxx d hyy + 2 |hxy| d hxy + u (hxx hyy + hxy^2 + |det|)
                nx = hyy bx - hxy by:   d nx = hyy d bx + |bx| d hyy + |hxy| d by + |by| d hxy
                                               + u (|hyy bx| + |hxy by| + |nx|)
                dx = nx * (1 / det):    d dx = d nx / |det| + |nx| d det / det^2 + 2 u |dx|          (dy alike)
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
U = 2.0 ** -24


def form_of(psz, wpp_env=0):
    """(NPL, WPP) of launch_patchflow for a patch size; wpp_env = the value of ICTR_PF_WPP (0: unset)."""
    npl = (psz * psz + 63) // 64
    if (wpp_env == 2) if wpp_env else npl > 4:
        return 8, 2
    return (1 if npl <= 1 else 4 if npl <= 4 else 16), 1


def lane_pixels(psz, wpp):
    """L: the most pixels of a psz x psz patch that one lane adds with wpp waves per patch (lane 0 of wave 0)."""
    return len(range(0, psz * psz, 64 * wpp))


def _view(plane, pad, psz):
    s = pad - psz
    return plane[s:, s:] if s else plane


def _sample(plane, x, y, psz, pad):
    """(value, majorant sum w|v|) of the patch at (x, y), both (psz, psz) f64. Taps (floor, floor + 1) in x and in y,
    weights from x - floor(x), y - floor(y): at an integer centre the value is the plane's own pixels. Wherever
    f32(x + 1e-5) is not rounded across an integer the value is np_oracle.patches' for one centre, bit for bit (same
    f32 expressions in the same order, the four taps as slices; tests/test_patchflow_cpu.py compares the two, and
    states where they differ)."""
    v = _view(plane, pad, psz)
    x, y = f32(x), f32(y)
    p0, p1 = int(np.floor(x)) + 1, int(np.floor(y)) + 1
    r0, r1 = x - np.floor(x), y - np.floor(y)
    w0, w1, w2, w3 = r0 * r1, (f32(1) - r0) * r1, r0 * (f32(1) - r1), (f32(1) - r0) * (f32(1) - r1)
    row, col = p1 + psz // 2, p0 + psz // 2
    a, b = v[row:row + psz, col:col + psz], v[row:row + psz, col - 1:col - 1 + psz]
    c, d = v[row - 1:row - 1 + psz, col:col + psz], v[row - 1:row - 1 + psz, col - 1:col - 1 + psz]
    val = ((w0 * a + w1 * b) + w2 * c) + w3 * d
    maj = ((w0 * np.abs(a) + w1 * np.abs(b)) + w2 * np.abs(c)) + w3 * np.abs(d)
    assert val.dtype == f32 and val.shape == (psz, psz)
    return val.astype(np.float64), maj.astype(np.float64)


class _Template:
    """Template patch of one point at one level: T, Gx, Gy, H and the bound's H terms."""

    def __init__(self, pyr, l, xl, yl, psz, nsum):
        self.T, self.aT = _sample(pyr.img[l], xl, yl, psz, pyr.pad)
        self.Gx, self.aGx = _sample(pyr.dx[l], xl, yl, psz, pyr.pad)
        self.Gy, self.aGy = _sample(pyr.dy[l], xl, yl, psz, pyr.pad)
        Gx, Gy = self.Gx, self.Gy
        self.hxx, self.hxy, self.hyy = (Gx * Gx).sum(), (Gx * Gy).sum(), (Gy * Gy).sum()
        self.det, self.tr = self.hxx * self.hyy - self.hxy * self.hxy, self.hxx + self.hyy
        S = nsum * U
        self.eGx, self.eGy, self.eT = 3 * U * self.aGx, 3 * U * self.aGy, 3 * U * self.aT
        aGx, aGy = np.abs(Gx), np.abs(Gy)
        self.dhxx = (2 * aGx * self.eGx).sum() + S * (Gx * Gx).sum()
        self.dhyy = (2 * aGy * self.eGy).sum() + S * (Gy * Gy).sum()
        self.dhxy = (aGx * self.eGy + aGy * self.eGx).sum() + S * (aGx * aGy).sum()
        self.ddet = (self.hyy * self.dhxx + self.hxx * self.dhyy + 2 * abs(self.hxy) * self.dhxy
                     + U * (self.hxx * self.hyy + self.hxy * self.hxy + abs(self.det)))
        self.S = S

    def step(self, plane_b, pad, cx, cy, psz):
        """(dx, dy), (bound dx, bound dy) of the Gauss-Newton step against frame B sampled at (cx, cy)."""
        I, aI = _sample(plane_b, cx, cy, psz, pad)
        Gx, Gy, aGx, aGy = self.Gx, self.Gy, np.abs(self.Gx), np.abs(self.Gy)
        r = self.T - I
        ar = np.abs(r)
        er = self.eT + 3 * U * aI + U * ar
        bx, by = (Gx * r).sum(), (Gy * r).sum()
        dbx = (self.eGx * ar + aGx * er).sum() + self.S * (aGx * ar).sum()
        dby = (self.eGy * ar + aGy * er).sum() + self.S * (aGy * ar).sum()
        hxx, hxy, hyy, det = self.hxx, self.hxy, self.hyy, self.det
        nx, ny = hyy * bx - hxy * by, hxx * by - hxy * bx
        dnx = (hyy * dbx + abs(bx) * self.dhyy + abs(hxy) * dby + abs(by) * self.dhxy
               + U * (abs(hyy * bx) + abs(hxy * by) + abs(nx)))
        dny = (hxx * dby + abs(by) * self.dhxx + abs(hxy) * dbx + abs(bx) * self.dhxy
               + U * (abs(hxx * by) + abs(hxy * bx) + abs(ny)))
        dx, dy = nx / det, ny / det
        ex = dnx / abs(det) + abs(nx) * self.ddet / (det * det) + 2 * U * abs(dx)
        ey = dny / abs(det) + abs(ny) * self.ddet / (det * det) + 2 * U * abs(dy)
        return (dx, dy), (ex, ey)


def _level_size(pyr, l):
    return pyr.img[l].shape[1] - 2 * pyr.pad, pyr.img[l].shape[0] - 2 * pyr.pad


def track_points(pyr_a, pyr_b, pts, psz, lv_f, lv_l=0, maxiter=10, eps=0.01, min_det=1e-4, detail=False, nsum=24):
    """pyr_*: oracle.Pyramid (host planes, padded by pad >= psz). pts (K,2). Returns (new (K,2) f32 with NaN, status,
    iters), and with detail=True a fourth value: a dict of per-point (K,) f64 arrays
      view   smallest distance of a tested position from the border it is tested against (0, w_l, h_l), over the tests
             whose operands can differ between two evaluations: cx, cy from the second test of a run on. (xl = x0 * 0.5^l
             is exact in f32, and the first cx, cy of a run are xl + 0, yl + 0: those tests cannot differ.) inf if none.
      view0  the same over every test, the exact ones included (a point on the frame's corner has 0 here)
      det    smallest |det / tr^2 - min_det| over the levels reached (inf where tr == 0: every product is an exact zero)
      eps    smallest |dx^2 + dy^2 - eps^2| over the steps taken;  eps_px: smallest | |d| - eps |
      bound  sum over the steps taken of the one-step bound (larger component) * 2^level, for sums of nsum = L + c terms
    """
    pts = np.asarray(pts, f32)
    K = len(pts)
    out = np.full((K, 2), np.nan, f32)
    status = np.zeros(K, bool)
    iters = np.zeros(K, np.int32)
    d = {k: np.full(K, np.inf) for k in ("view", "view0", "det", "eps", "eps_px")}
    d["bound"] = np.zeros(K)

    def border(k, x, y, wl, hl, exact):
        with np.errstate(invalid="ignore"):
            m = float(np.min(np.abs([x, y, x - wl, y - hl]).astype(np.float64)))
        d["view0"][k] = min(d["view0"][k], m)
        if not exact:
            d["view"][k] = min(d["view"][k], m)

    for k in range(K):
        x0, y0 = pts[k]
        if not (np.isfinite(x0) and np.isfinite(y0)):
            continue
        p = np.zeros(2, f32)
        ok, nit, first = True, 0, True
        for l in range(lv_f, lv_l - 1, -1):
            if l != lv_f:
                p = p * f32(2)
            sc = f32(0.5 ** l)
            wl, hl = _level_size(pyr_a, l)
            xl, yl = f32(x0 * sc), f32(y0 * sc)
            border(k, xl, yl, wl, hl, True)
            if not (0 <= xl <= wl and 0 <= yl <= hl):
                ok = False
                break
            t = _Template(pyr_a, l, xl, yl, psz, nsum)
            if t.tr > 0:
                d["det"][k] = min(d["det"][k], abs(t.det / (t.tr * t.tr) - min_det))
            if not (t.det > min_det * t.tr * t.tr) or not (t.tr > 0):
                ok = False
                break
            for _ in range(maxiter):
                cx, cy = f32(xl + p[0]), f32(yl + p[1])
                border(k, cx, cy, wl, hl, first)
                first = False
                if not (0 <= cx <= wl and 0 <= cy <= hl):
                    ok = False
                    break
                (dx, dy), (ex, ey) = t.step(pyr_b.img[l], pyr_b.pad, cx, cy, psz)
                p = (p + np.array([dx, dy])).astype(f32)
                nit += 1
                n2 = dx * dx + dy * dy
                d["eps"][k] = min(d["eps"][k], abs(n2 - eps * eps))
                d["eps_px"][k] = min(d["eps_px"][k], abs(np.sqrt(n2) - eps))
                d["bound"][k] += max(ex, ey) * 2.0 ** l
                if n2 < eps * eps:
                    break
            if not ok:
                break
        if ok:
            s = f32(2.0 ** lv_l)
            out[k] = (x0 + p[0] * s, y0 + p[1] * s)
        status[k], iters[k] = ok, nit
    return (out, status, iters, d) if detail else (out, status, iters)


def one_step(pyr_a, pyr_b, pts, psz, level, L, wpp=1, min_det=1e-4):
    """The Gauss-Newton step H^-1 b of every point at one level from p = 0, in f64 on the f32 patch values, and the
    per-component bound of an f32 evaluation that adds L pixels per lane with wpp waves per patch (module docstring).
    Returns (step (K,2) f64, bound (K,2) f64, det / tr^2 (K,) f64); NaN rows for points that are not finite, out of view
    at the level or refused by the conditioning test."""
    pts = np.asarray(pts, f32)
    K = len(pts)
    step, bound, cond = np.full((K, 2), np.nan), np.full((K, 2), np.nan), np.full(K, np.nan)
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
            cond[k] = t.det / (t.tr * t.tr)
        if not (t.det > min_det * t.tr * t.tr) or not (t.tr > 0):
            continue
        step[k], bound[k] = t.step(pyr_b.img[level], pyr_b.pad, xl, yl, psz)
    return step, bound, cond
