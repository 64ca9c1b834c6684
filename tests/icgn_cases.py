"""Cases, oracle records and error bounds for the raw H / b sums of the full-frame alignment engine
(csrc/ictr_icgn.hip), shared by test_gpu_icgn_sums.py and test_icgn_sums_cpu.py.

One *case* is one engine (frame, model, template region, kernel form, grid) evaluated at one initial warp; every case
is checked at pyramid levels 0, 1 and 2. The oracle is oracle/np_icgn.NpEngine (f64) on the planes of oracle.Pyramid,
which are bit-equal to the device's.

Bound (derived, not fitted): the device sums f32 terms whose per-pixel relative error is a few roundings -- coordinates,
warp, four-tap blend, steepest-descent row, product -- and adds them in f32 L at a time per lane, then over 6 shuffle
and 2 LDS steps, then in f64:

    tol_H[a,c] = (24 + L) * 2^-24 * sum_px         sd~_a * sd~_c
    tol_b[k]   = (24 + L) * 2^-24 * sum_in-frame   sd~_k * (max|cur plane| + |T(x)|)

sd~ is the steepest-descent row built from |gx|, |gy|, |nx|, |ny| with every subtraction turned into a sum (for the
homography q~ = |gx||nx| + |gy||ny|). The blend is bounded against the image amplitude because r = I - T cancels.
L is the largest number of pixels one lane adds, from the kernel's tiling (lane_load below).
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from oracle import np_icgn as NI

LV_F = 2
LEVELS = (0, 1, 2)
MODELS = ("translation", "se2", "affine", "homography")
MODEL_ID = {"translation": 0, "se2": 1, "affine": 2, "homography": 3}
GT_SHIFT = (1.3, -0.7)          # the pair is rendered with this translation; the sums are taken elsewhere
EPS24 = 2.0 ** -24
K_ROUND = 24                    # per-pixel roundings + 6 shuffle + 2 LDS additions
BLOCK, WAVES = 256, 4           # kBlock, kWaves of the kernels
LDS_W, LDS_H = 288, 12          # kIcLW, kIcLH

# frame name -> (w, h, padding, the path it is the smallest shape to reach)
FRAMES = {
    "75x51p4": (75, 51, 4, "pitch 83: scalar form chosen by the pitch; levels 38x26 and 19x13 round up"),
    "76x52p4": (76, 52, 4, "vector form at level 0 (pitch 84), scalar at levels 1 and 2 (pitches 46, 27)"),
    "70x46p2": (70, 46, 2, "scalar form chosen by the padding (< 4)"),
    "96x40p16": (96, 40, 16, "pitch 128: 32-float start, x0 = 2 masks the first 16 pixels of a row; level 1 has "
                             "the 4-float start (pitch 80)"),
    "300x20p4": (300, 20, 4, "two tile columns (256 + 40), last tile row of fewer than 4 rows, nq > 64"),
    "288x24p16": (288, 24, 16, "pitch 320: 32-float start and two tile columns at once"),
}
VECTOR_FRAMES = ("76x52p4", "96x40p16", "300x20p4", "288x24p16")   # level 0 runs a vector form by default
BAND_FRAMES = ("75x51p4", "76x52p4")
# ranks the default region's rows are split over: 47 rows over 3 give 16, 16, 15; the 48 rows of 76x52 give three
# multiples of four, so that frame is also split over 5 (10, 10, 10, 9, 9)
BAND_SPLITS = {"75x51p4": (3,), "76x52p4": (3, 5)}

# warps the sums are evaluated at (none is the truth, so residuals are far from zero)
# (the vertical shift is large enough that, at level 2 of the flat frames, the last template row stays below the
# threshold h_l - 1 under the rotations and shears: a row crossing it at a slope of 0.003 px per pixel cannot keep
# every pixel 1e-3 px away from it)
NEAR = {
    "translation": [0.83, -0.91],
    "se2": [0.0037, 0.83, -0.91],
    "affine": [0.0041, -0.0029, 0.0023, -0.0047, 0.83, -0.91],
    "homography": [0.0041, -0.0029, 2.1e-5, 0.0023, -0.0047, -3.3e-5, 0.83, -0.91],
}
# shift of the far warp: (6.5, -5.5); on 288x24 x' = 1.05 x - 0.7 puts column 274 on the threshold w - 1 = 287 exactly,
# so there the shift moves by 0.03 px
FAR_SHIFT = {None: (6.5, -5.5), "288x24p16": (6.53, -5.5)}
WARPS = {
    "near": "the model's own parametrisation, half a pixel from the truth",
    "far": "affine, scale 1.05 about the centre, shift (6.5, -5.5): about 20 % of the template leaves the frame",
    "rot001": "SE(2), theta = 0.01: a tile's footprint is at most 12 rows, the LDS form stages it",
    "rot02": "SE(2), theta = 0.2: 96 sin 0.2 = 19 rows, the LDS form falls back to direct gathers",
}

Case = namedtuple("Case", "frame model region warp form gridx why")


def case_id(c):
    return f"{c.frame}-{c.model}-{c.region}-{c.warp}-{c.form}-g{c.gridx or 'dflt'}"


def frame_size(frame):
    w, h, pad, _ = FRAMES[frame]
    return w, h, pad


def level_size(w, h, l):
    for _ in range(l):
        w, h = (w + 1) // 2, (h + 1) // 2
    return w, h


def region_px(frame, region):
    """Level-0 template region (x0, y0, w, h): the engine's default (a 2-pixel rim) or one with odd origin and size.
    The two flat frames keep 15 and 19 rows (last tile row of 3 rows): with h - 9 their level 2 would be 3 rows, and
    the far warp's share inside the frame could only be 2/3 or 1."""
    w, h, _ = frame_size(frame)
    return (2, 2, w - 4, h - 4) if region == "default" else (5, 3, w - 12, h - 9 if h >= 40 else h - 5)


def warp_px(frame, model, warp):
    """Initial warp in level-0 pixel coordinates."""
    from invcompcamtrack_amd import icgn
    w, h, _ = frame_size(frame)
    C = np.array([[1, 0, w / 2], [0, 1, h / 2], [0, 0, 1.0]])
    if warp == "near":
        A = icgn.warp_matrix(model, NEAR[model])
    elif warp == "far":
        sx, sy = FAR_SHIFT.get(frame, FAR_SHIFT[None])
        A = np.array([[1.05, 0, sx], [0, 1.05, sy], [0, 0, 1.0]])
    else:
        A = icgn.warp_matrix("se2", [{"rot001": 0.01, "rot02": 0.2}[warp], 0.8, -0.3])
    M = C @ A @ np.linalg.inv(C)
    return M / M[2, 2]


def iter_form(frame, level, form):
    """The form of k_icgn_iter a level runs (icgn_iter_main): 'scalar', 'vector' or 'lds'."""
    w, h, pad = frame_size(frame)
    sw = level_size(w, h, level)[0] + 2 * pad
    if form == "scalar" or pad < 4 or sw % 4:
        return "scalar"
    return "lds" if form == "lds" else "vector"


def grid_blocks(region0, level, gridx, vec, nproblems=1):
    """Workgroups per problem at one level (icgn_grid); gridx None = the engine's default."""
    gx = max(64, 8192 // nproblems) if gridx is None else max(int(gridx), 1)
    s = 1 << level
    w, h = max(region0[2] // s, 1), max(region0[3] // s + 1, 1)
    units = ((w + 255) // 256 + 1) * ((h + 3) // 4) if vec else (w * h + BLOCK - 1) // BLOCK
    per = (units + gx - 1) // gx
    return max(1, min(gx, (units + per - 1) // per))


def _lane_counts(kind, R, pad, sw, nblk):
    """Pixels added by each (workgroup, thread) of one launch over level region R = (x0, y0, w, h), from the tiling."""
    x0, y0, rw, rh = R
    cnt = np.zeros(nblk * BLOCK, np.int64)
    if rw <= 0 or rh <= 0:
        return cnt
    if kind == "scalar":                      # grid-stride over the region's pixels, x fastest
        t = np.arange(rw * rh)
        np.add.at(cnt, t % (nblk * BLOCK), 1)
        return cnt
    rows = np.arange(rh)
    ty, wave = rows // WAVES, rows % WAVES
    if kind == "vector":                      # quads aligned to the padded row, 64 quads x 4 rows per tile
        xs = x0 - ((x0 + pad) & (31 if sw % 32 == 0 else 3))
        nq = (x0 + rw - xs + 3) >> 2
        ntx = (nq + 63) >> 6
        q = np.arange(nq)
        xq = xs + 4 * q
        npx = np.clip(np.minimum(xq + 4, x0 + rw) - np.maximum(xq, x0), 0, 4)
        tx, lane = q // 64, q % 64
    else:                                     # lds: 256 pixels x 4 rows per tile from the region's first column
        ntx = (rw + 255) >> 8
        c = np.arange(rw)
        npx = np.ones(rw, np.int64)
        tx, lane = c // 256, c % 64
    blk = (ty[:, None] * ntx + tx[None, :]) % nblk
    tid = wave[:, None] * 64 + lane[None, :]
    np.add.at(cnt, (blk * BLOCK + tid).ravel(), np.broadcast_to(npx[None, :], blk.shape).ravel())
    return cnt


def lane_load(c, level, rows=None, nproblems=1):
    """(L of k_icgn_hess, L of the iteration kernel): the most pixels one lane adds in f32."""
    w, h, pad = frame_size(c.frame)
    reg0 = region_px(c.frame, c.region)
    R = NI.region_at(reg0, level, rows)
    sw = level_size(w, h, level)[0] + 2 * pad
    kind = iter_form(c.frame, level, c.form)
    nb_h = grid_blocks(reg0, level, c.gridx, False, nproblems)
    nb_i = grid_blocks(reg0, level, c.gridx, kind != "scalar", nproblems)
    return int(_lane_counts("scalar", R, pad, sw, nb_h).max()), int(_lane_counts(kind, R, pad, sw, nb_i).max())


def lane_load_brute(kind, R, pad, sw, nblk):
    """The same count by running every thread's loop of the kernel one step at a time (checks lane_load)."""
    x0, y0, rw, rh = R
    best = 0
    for bx in range(nblk):
        for tid in range(BLOCK):
            lane, wave, n = tid & 63, tid >> 6, 0
            if kind == "scalar":
                t = bx * BLOCK + tid
                while t < rw * rh:
                    n += 1
                    t += nblk * BLOCK
            elif kind == "vector":
                xs = x0 - ((x0 + pad) & (31 if (sw & 31) == 0 else 3))
                nq = (x0 + rw - xs + 3) >> 2
                ntx, nty = (nq + 63) >> 6, (rh + WAVES - 1) // WAVES
                for t in range(bx, ntx * nty, nblk):
                    ty = t // ntx
                    tx = t - ty * ntx
                    row, q = ty * WAVES + wave, tx * 64 + lane
                    if row >= rh or q >= nq:
                        continue
                    x = xs + 4 * q
                    n += sum(1 for j in range(4) if x0 <= x + j < x0 + rw)
            else:
                ntx, nty = (rw + 255) >> 8, (rh + WAVES - 1) // WAVES
                for t in range(bx, ntx * nty, nblk):
                    ty = t // ntx
                    tx = t - ty * ntx
                    if ty * WAVES + wave >= rh:
                        continue
                    n += sum(1 for j in range(4) if (tx << 8) + lane + 64 * j < rw)
            best = max(best, n)
    return best


def lds_rows(frame, model, warp, level, region):
    """Largest number of current-frame rows the LDS form would stage for a tile (its own formula, in f64)."""
    w, h, pad = frame_size(frame)
    wl, hl = level_size(w, h, level)
    cx, cy, f = NI.level_geometry(w, h, level)
    K = NI.K_matrix(w, h)
    M = np.linalg.inv(K) @ warp_px(frame, model, warp) @ K
    x0, y0, rw, rh = NI.region_at(region_px(frame, region), level)
    worst = 0
    for ty0 in range(y0, y0 + rh, WAVES):
        for tx0 in range(x0, x0 + rw, 256):
            xs = np.array([tx0, min(tx0 + 255, x0 + rw - 1)], np.float64)
            ys = np.array([ty0, min(ty0 + WAVES - 1, y0 + rh - 1)], np.float64)
            X, Y = np.meshgrid((xs - cx) / f, (ys - cy) / f)
            q = M[2, 0] * X + M[2, 1] * Y + M[2, 2]
            py = (M[1, 0] * X + M[1, 1] * Y + M[1, 2]) / q * f + cy
            c0 = max(int(np.floor(py.min())) - 1, -pad)
            c1 = min(int(np.floor(py.max())) + 2, hl - 1 + pad)
            worst = max(worst, c1 - c0 + 1)
    return worst


# ---------------------------------------------------------------- images, planes, oracle records
@functools.lru_cache(maxsize=None)
def pair(frame, seed=1234):
    from invcompcamtrack_amd import icgn
    w, h, _ = frame_size(frame)
    Mgt = np.eye(3)
    Mgt[0, 2], Mgt[1, 2] = GT_SHIFT
    return icgn.make_warped_pair(w, h, Mgt, seed=seed)


_planes = {}


def oracle_planes(O, frame, seed=1234):
    """(template planes per level, current planes per level) of oracle.Pyramid."""
    key = (frame, seed)
    if key not in _planes:
        _, _, pad = frame_size(frame)
        a, b = pair(frame, seed)
        pa, pb = O.Pyramid(a, LV_F, pad), O.Pyramid(b, LV_F, pad)
        _planes[key] = (pa, [(pa.img[l], pa.dx[l], pa.dy[l]) for l in range(LV_F + 1)],
                        [pb.img[l] for l in range(LV_F + 1)])
    return _planes[key][1], _planes[key][2]


Record = namedtuple("Record", "H b majH majb npx inframe margin")
_records = {}


def sd_majorant(model, gx, gy, x, y):
    gx, gy, x, y = np.abs(gx), np.abs(gy), np.abs(x), np.abs(y)
    if model == 0:
        return [gx, gy]
    if model == 1:
        return [gy * x + gx * y, gx, gy]
    if model == 2:
        return [gx * x, gy * x, gx * y, gy * y, gx, gy]
    q = gx * x + gy * y
    return [gx * x, gy * x, q * x, gx * y, gy * y, q * y, gx, gy]


def oracle_record(O, frame, model, level, region0, M0, rows=None, seed=1234):
    """H (upper triangle) and b of one launch in f64, the majorants of the bound, and the inputs' condition: the share
    of template pixels that land inside the current frame and the smallest distance of a warped position from the
    in-frame test's thresholds 0, w_l - 1 and h_l - 1."""
    key = (frame, model, level, tuple(region0), tuple(np.asarray(M0).ravel()), rows, seed)
    if key in _records:
        return _records[key]
    w, h, pad = frame_size(frame)
    m = MODEL_ID[model]
    pa, pb = oracle_planes(O, frame, seed)
    e = NI.NpEngine(pa, pb, pad, w, h, m, 1, 0.0, tuple(region0), M0, rows)
    e.begin()
    e.hess_accumulate(level)
    n, nh = e.n, e.n * (e.n + 1) // 2
    H = e.red[:nh].copy()
    e.hess_finish(level)
    e.iter_accumulate(level)
    b = e.red[36:36 + n].copy()
    x0, y0, rw, rh = NI.region_at(tuple(region0), level, rows)
    if rw * rh == 0:
        rec = Record(H, b, np.zeros(nh), np.zeros(n), 0, 1.0, np.inf)
    else:
        ys, xs = np.mgrid[y0:y0 + rh, x0:x0 + rw]
        gx = np.asarray(pa[level][1], np.float64)[ys + pad, xs + pad].ravel()
        gy = np.asarray(pa[level][2], np.float64)[ys + pad, xs + pad].ravel()
        nx, ny = e.nx.ravel(), e.ny.ravel()
        sdm = np.stack(sd_majorant(m, gx, gy, nx, ny), 0)
        majH = (sdm @ sdm.T)[np.triu_indices(n)]
        M = e.M
        q = M[2, 0] * nx + M[2, 1] * ny + M[2, 2]
        px = (M[0, 0] * nx + M[0, 1] * ny + M[0, 2]) / q * e.f + e.cx
        py = (M[1, 0] * nx + M[1, 1] * ny + M[1, 2]) / q * e.f + e.cy
        ok = (px >= 0) & (py >= 0) & (px <= e.wl - 1) & (py <= e.hl - 1)
        amp = np.abs(e.cur).max() + np.abs(e.T.ravel())
        majb = sdm[:, ok] @ amp[ok]
        margin = min(np.abs(px).min(), np.abs(py).min(), np.abs(px - (e.wl - 1)).min(), np.abs(py - (e.hl - 1)).min())
        rec = Record(H, b, majH, majb, rw * rh, float(ok.mean()), float(margin))
    _records[key] = rec
    return rec


def tolerances(rec, L_hess, L_iter):
    return (K_ROUND + L_hess) * EPS24 * rec.majH, (K_ROUND + L_iter) * EPS24 * rec.majb


def trimmed_regions(region0, level):
    """Four level-0 regions whose level-`level` region is the case's without its first column, last column, first row,
    last row (exactly one level pixel each)."""
    x0, y0, rw, rh = region0
    s = 1 << level
    lx0, ly0, lw, lh = NI.region_at(region0, level)
    x1, y1 = x0 + rw, y0 + rh
    out = {"first column": (s * (lx0 + 1), y0, x1 - s * (lx0 + 1), rh),
           "last column": (x0, y0, s * (lx0 + lw - 1) - x0, rh),
           "first row": (x0, s * (ly0 + 1), rw, y1 - s * (ly0 + 1)),
           "last row": (x0, y0, rw, s * (ly0 + lh - 1) - y0)}
    for name, r in out.items():
        want = {"first column": (lx0 + 1, ly0, lw - 1, lh), "last column": (lx0, ly0, lw - 1, lh),
                "first row": (lx0, ly0 + 1, lw, lh - 1), "last row": (lx0, ly0, lw, lh - 1)}[name]
        assert NI.region_at(r, level) == want, (name, r, level)
    return out


# ---------------------------------------------------------------- bands, batch, rank-deficient inputs
ONE_ROW = (24, 25)     # level-0 rows; 24 is a multiple of 4, so the band holds exactly one row at every level
EMPTY = (24, 24)
BATCH_WARPS = ("near", "far", "rot001")
BATCH_SEEDS = (1234, 77, 5)

# Vertical stripes: gy is exactly 0 at every level, so the translation H has rank 1 and the affine H rank 3. The frame
# is 64 wide so that f = 32: the conversion between normalised and pixel warps is then exact and zeros stay zeros.
STRIPES_W, STRIPES_H, STRIPES_PAD, STRIPES_SHIFT = 64, 48, 4, 1.5


def stripes_pair():
    xs = np.arange(STRIPES_W, dtype=np.float64)
    a = np.tile(100 + 50 * np.sin(0.35 * xs), (STRIPES_H, 1)).astype(np.float32)
    b = np.tile(100 + 50 * np.sin(0.35 * (xs - STRIPES_SHIFT)), (STRIPES_H, 1)).astype(np.float32)
    return a, b


def planes_of(O, a, b, pad, lv_f=LV_F):
    pa, pb = O.Pyramid(a, lv_f, pad), O.Pyramid(b, lv_f, pad)
    return [(pa.img[l], pa.dx[l], pa.dy[l]) for l in range(lv_f + 1)], [pb.img[l] for l in range(lv_f + 1)]


def lstsq(H, b):
    """Minimum-norm solve: on a block-zero H it equals "free variables = 0", the device's particular solution."""
    return np.linalg.lstsq(H, b, rcond=None)[0]


# ---------------------------------------------------------------- the case table
def _cases():
    out = []
    # every frame x model x region x (near, far) in the form and grid a user gets
    for fr in FRAMES:
        for m in MODELS:
            for reg in ("default", "odd"):
                for wp in ("near", "far"):
                    out.append(Case(fr, m, reg, wp, "default", None, FRAMES[fr][3]))
    # the other two forms where the pitch allows a choice
    for fr in VECTOR_FRAMES:
        for m in MODELS:
            for form in ("lds", "scalar"):
                for reg in ("default", "odd"):
                    out.append(Case(fr, m, reg, "far", form, None, f"ICTR_ICGN_{form.upper()}=1 on {fr}"))
            out.append(Case(fr, m, "default", "near", "lds", None, "LDS form, near-identity warp: every tile staged"))
            out.append(Case(fr, m, "odd", "rot001", "lds", None, WARPS["rot001"]))
    for m in MODELS:
        out.append(Case("96x40p16", m, "default", "rot02", "lds", None, WARPS["rot02"]))
        out.append(Case("96x40p16", m, "default", "rot02", "default", None, "the same warp through direct gathers"))
    # 1 and 3 workgroups: grid-stride loops, and tails over a number of partials that is no multiple of 4 or 32
    for fr in FRAMES:
        forms = ("default", "lds", "scalar") if fr in VECTOR_FRAMES else ("default",)
        for m in MODELS:
            for form in forms:
                for g in (1, 3):
                    out.append(Case(fr, m, "odd", "far", form, g, f"ICTR_ICGN_GRIDX={g}: grid-stride loop, {g} partial(s)"))
    return out


CASES = _cases()
