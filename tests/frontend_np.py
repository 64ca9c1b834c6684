"""The point-track front end restated in NumPy (test infrastructure, like triang_np.py): the checker of ictr_frontend.hip.

Each function states in words-as-code the definition that the device kernels implement (DESIGN.md §4 "Point-track front
end"), written independently of the host functions it is pinned to by tests/test_frontend_cpu.py:

  good_features(img, ...)      the cell rule: direct separable window sums, one winner per mindist x mindist cell, winners
                               ordered by (lam descending, index ascending)      == patchflow.good_features on integer frames
  fill(d, lost)                lost nodes: nearest tracked node to the left, else right; empty rows: nearest filled row
                               above, else below; else 0                         == dense_flow's fill
  field_at(d, step, w, h, X, Y) dense_flow's up-sampled field at integer pixels, from the nodes
  gather(d, step, w, h, xy)    func_get_transf_position on that field, never formed
  OfTrack                      oftrack.addframe per live point, on two gather callables
"""
import numpy as np


def good_features(img, maxcorners=1000, quality=0.001, mindist=5, win=3):
    img = np.asarray(img, np.float64)
    H, W = img.shape
    gx, gy = np.zeros((H, W)), np.zeros((H, W))
    if W > 2:
        gx[:, 1:-1] = img[:, 2:] - img[:, :-2]
    if H > 2:
        gy[1:-1, :] = img[2:, :] - img[:-2, :]

    def box(a):  # zero-padded (2 win + 1)^2 sums: rows over dx ascending, then columns over dy ascending
        p = np.pad(a, ((0, 0), (win, win)))
        r = np.zeros((H, W))
        for k in range(2 * win + 1):
            r = r + p[:, k:k + W]
        p = np.pad(r, ((win, win), (0, 0)))
        c = np.zeros((H, W))
        for k in range(2 * win + 1):
            c = c + p[k:k + H, :]
        return c

    sxx, sxy, syy = box(gx * gx), box(gx * gy), box(gy * gy)
    df = sxx - syy
    lam = 0.5 * (sxx + syy) - np.sqrt(0.25 * (df * df) + sxy * sxy)
    ys, xs = np.mgrid[0:H, 0:W]
    lam[(xs < mindist) | (xs >= W - mindist) | (ys < mindist) | (ys >= H - mindist)] = 0.0
    thr = quality * lam.max()
    p = np.pad(lam, 1, constant_values=-1.0)
    cand = lam > thr
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                cand &= lam >= p[dy:dy + H, dx:dx + W]
    best = {}  # cell -> (lam, index): the largest lam, ties to the smallest index
    for y, x in zip(*np.nonzero(cand)):
        c = (y // mindist, x // mindist)
        v, i = lam[y, x], y * W + x
        if c not in best or v > best[c][0] or (v == best[c][0] and i < best[c][1]):
            best[c] = (v, i)
    win_ = sorted(best.values(), key=lambda t: (-t[0], t[1]))[:maxcorners]
    return np.array([(i % W, i // W) for _, i in win_], np.float32).reshape(-1, 2)


def fill(d, lost):
    """d (ny, nx, 2) float32, lost (ny, nx) bool -> the filled copy."""
    d = np.array(d, np.float32)
    lost = np.asarray(lost, bool)
    ny, nx = lost.shape
    out = np.zeros_like(d)
    has = ~lost.all(1)
    for j in np.nonzero(has)[0]:
        tracked = np.nonzero(~lost[j])[0]
        for i in range(nx):
            left = tracked[tracked <= i]
            src = left[-1] if len(left) else tracked[tracked > i][0]
            out[j, i] = d[j, src]
    rows = np.nonzero(has)[0]
    for j in np.nonzero(~has)[0]:
        above = rows[rows < j]
        below = rows[rows > j]
        if len(above):
            out[j] = out[above[-1]]
        elif len(below):
            out[j] = out[below[0]]
    return out


def field_at(d, step, w, h, X, Y):
    """dense_flow's field at the integer pixels (X, Y) (arrays): (n, 2) float32, from the filled nodes d."""
    ny, nx = d.shape[:2]
    X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
    fx = np.clip((X - step // 2) / step, 0, nx - 1)
    fy = np.clip((Y - step // 2) / step, 0, ny - 1)
    x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
    x1, y1 = np.minimum(x0 + 1, nx - 1), np.minimum(y0 + 1, ny - 1)
    ax, ay = (fx - x0)[:, None], (fy - y0)[:, None]
    top = d[y0, x0] * (1 - ax) + d[y0, x1] * ax
    bot = d[y1, x0] * (1 - ax) + d[y1, x1] * ax
    return (top * (1 - ay) + bot * ay).astype(np.float32)


def gather(d, step, w, h, xy):
    """func_get_transf_position(xy, F[:, :, 0], F[:, :, 1]), F the dense w x h field of the nodes d, four taps a point."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    out = np.full(xy.shape, np.nan)
    fl = np.floor(xy)
    ok = (fl[:, 0] >= 0) & (fl[:, 1] >= 0) & (fl[:, 0] + 1 < w) & (fl[:, 1] + 1 < h)  # NaN compares false
    idx = np.nonzero(ok)[0]
    x0, y0 = fl[idx, 0].astype(np.int64), fl[idx, 1].astype(np.int64)
    fx, fy = xy[idx, 0] - fl[idx, 0], xy[idx, 1] - fl[idx, 1]
    w0, w1, w2, w3 = fx * fy, (1 - fx) * fy, fx * (1 - fy), (1 - fx) * (1 - fy)
    f11, f01 = field_at(d, step, w, h, x0 + 1, y0 + 1), field_at(d, step, w, h, x0, y0 + 1)
    f10, f00 = field_at(d, step, w, h, x0 + 1, y0), field_at(d, step, w, h, x0, y0)
    for c in (0, 1):
        out[idx, c] = xy[idx, c] + (f11[:, c] * w0 + f01[:, c] * w1 + f10[:, c] * w2 + f00[:, c] * w3)
    return out


class OfTrack:
    """oftrack with addframe taking two gather callables (xy (K,2) f64 -> (K,2) f64) instead of two dense fields."""

    def __init__(self, bsize, th_ratio=0.2, th_abs=1.0):
        self.bsize, self.th_ratio, self.th_abs = bsize, th_ratio, th_abs
        self.tracks, self.tracks_valid, self.tracks_absmovement, self.frcounter = [], [], [], 0

    def addframe(self, forw, back, corners=None):
        self.frcounter += 1
        if corners is not None and len(corners):
            K = len(corners)
            blk = np.full((K, 2, self.bsize), np.nan, np.float32)
            blk[:, :, 0] = corners
            self.tracks.append(blk)
            self.tracks_valid.append(np.ones(K, bool))
            self.tracks_absmovement.append(np.zeros(K, np.float64))
        else:
            self.tracks.append(None)
            self.tracks_valid.append(None)
            self.tracks_absmovement.append(None)
        k = self.frcounter - 1
        for age in range(0, self.bsize - 1):
            b = k - age
            if b < 0 or self.tracks[b] is None:
                continue
            t, va, am = self.tracks[b], self.tracks_valid[b], self.tracks_absmovement[b]
            for i in np.nonzero(va)[0]:  # per live point, as the device does
                xl = t[i, :, age].astype(np.float64)
                xf = forw(xl[None])[0]
                xb = back(xf[None])[0]
                with np.errstate(invalid="ignore", divide="ignore"):
                    e, m = xl - xb, xl - xf
                    fb = np.sqrt(e[0] * e[0] + e[1] * e[1])
                    mv = np.sqrt(m[0] * m[0] + m[1] * m[1])
                    ok = (fb / mv < self.th_ratio) and (fb < self.th_abs)
                    if not ok:
                        xf = np.array([np.nan, np.nan])
                    t[i, :, age + 1] = xf
                    a = t[i, :, 0].astype(np.float64) - xf
                    am[i] = np.sqrt(a[0] * a[0] + a[1] * a[1])
                va[i] = bool((~np.isnan(xf)).any())
        for b in range(0, self.frcounter - self.bsize + 1):
            if self.tracks[b] is None:
                continue
            live = np.nonzero(self.tracks_valid[b])[0]
            self.tracks[b] = self.tracks[b][live]
            self.tracks_valid[b] = np.ones(len(live), bool)
            self.tracks_absmovement[b] = self.tracks_absmovement[b][live]


# ---------------------------------------------------------------- the cases shared by the CPU and the GPU tests
# (H, W, mindist, win, maxcorners, grey levels)
CORNER_CASES = [(37, 53, 5, 3, 1000, 256), (37, 53, 5, 3, 7, 256), (40, 64, 3, 1, 50, 4), (23, 29, 7, 2, 100, 8),
                (64, 64, 1, 3, 5000, 256)]
# (w, h, step)
GRID_CASES = [(53, 37, 4), (64, 40, 4), (50, 31, 5), (9, 7, 4), (41, 23, 3)]


def corner_image(H, W, levels, seed=0):
    """Integer-valued frame with `levels` grey levels in 0..255 (few levels: heavy ties in lam)."""
    rng = np.random.default_rng(seed + H * 1000 + W)
    return np.round(rng.integers(0, levels, (H, W)) * (255.0 / max(levels - 1, 1))).astype(np.float32)


def grid_nodes(w, h, step, lost_fraction, seed, rows_lost_at_top=0):
    """Injected node displacements, the lost mask, and the nodes as dense_flow holds them before its fill (lost = NaN)."""
    rng = np.random.default_rng(seed)
    nx, ny = len(range(step // 2, w, step)), len(range(step // 2, h, step))
    d = rng.uniform(-3, 3, (ny, nx, 2)).astype(np.float32)
    lost = rng.uniform(size=(ny, nx)) < lost_fraction
    lost[:rows_lost_at_top] = True
    return d, lost


def grid_points(w, h, seed, n=200):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-2, max(w, h) + 2, (n, 2))
    pts[:, 0] = rng.uniform(-2, w + 2, n)
    pts[:, 1] = rng.uniform(-2, h + 2, n)
    special = [(np.nan, 3.0), (2.0, np.nan), (0, 0), (w - 1, h - 1), (w - 2, h - 2), (w - 1.5, h - 1.5), (-0.5, 1), (1e30, 1),
               (w - 1.0, 2.0), (0.25, h - 2.0)]
    return np.concatenate([np.array(special, np.float64), pts])
