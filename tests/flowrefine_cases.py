"""Cases, recorded differences and usefulness scenes for the variational refinement (csrc/ictr_flowrefine.hip), shared by
test_flowrefine_cpu.py and test_gpu_flowrefine.py.

The definition is patchflow.refine_flow_host (f64). flowrefine_f32.py restates the kernels in f32; its worst absolute
difference to the definition over the table below is RECORDED here per stage (one outer iteration, so that both start from
the same planes) and per full-run setting. test_flowrefine_cpu.py measures the differences again and fails if one exceeds
its record; the GPU tests hold the device to MARGIN x the record, MARGIN = 4 being the project's allowance for the
device's other contraction order. Nothing here is fitted to the device.

Those tolerances are set by a few ill-conditioned pixels, so the GPU tests also hold the device to the restatement's BITS:
every stage plane and every full run of TABLE and of EDGE (below: the shapes where a tile's edge, a one-lane workgroup or
a colour's row length can be misread, with part of every field outside the frame), the weights of PARAMS, and fields
that leave the frame by far or hold a NaN. The restatement's own distance to the definition at those shapes and weights
is recorded in the same way (EDGE_STAGE_DIFF, EDGE_FULL_DIFF, PARAM_DIFF) and carries no margin.

Frames: patchflow_cases.pair's 100x77 and 67x53 (partial tiles in x and y, several tiles each way), its far frames 320x64
and 64x320, and 9x7, a crop that is a single partial tile. F0 is dense_flow on the host oracle's tracking ("dense") or a
seeded smooth field ("smooth").
"""
from __future__ import annotations

import functools

import numpy as np

import patchflow_cases as PC
from oracle import np_patchflow as NP

MARGIN = 4.0
U = 2.0 ** -24
FRAMES = ("100x77", "67x53", "farxy-320x64", "farxy-64x320", "9x7")
# (frame, F0 kind): the table the differences are recorded over
TABLE = (("100x77", "dense"), ("100x77", "smooth"), ("67x53", "dense"), ("67x53", "smooth"), ("farxy-320x64", "smooth"),
         ("farxy-64x320", "smooth"), ("9x7", "smooth"))
RUNS = ((1, 1, 1.0), (3, 5, 1.6), (8, 5, 1.6))     # (n_outer, n_sor, omega), each with and without x_only
BOUNDARY_PX, BOUNDARY_SHARE = 1e-3, 0.005          # pixels this close to the inside boundary may be left out


# the far pair of 64 x 320 is farxy-320x64 transposed: fary-64x320's own shift has no x component, and a refined u that
# tends to 0 puts the whole first column on the inside boundary (see BOUNDARY_SHARE)
SHIFT = {"farxy-320x64": (1.3, -0.9), "farxy-64x320": (-0.9, 1.3), "9x7": (0.3, -0.2)}


def frame_size(frame):
    if frame.startswith("edge-"):
        w, h = frame[5:].split("x")
        return int(w), int(h)
    return (9, 7) if frame == "9x7" else (64, 320) if frame == "farxy-64x320" else PC.frame_size(frame)


@functools.lru_cache(maxsize=None)
def pair(frame):
    if frame.startswith("edge-"):
        return _edge_pair(frame)
    if frame == "9x7":
        a, b = PC.pair("100x77")
        return np.ascontiguousarray(a[30:37, 40:49]), np.ascontiguousarray(b[30:37, 40:49])
    if frame == "farxy-64x320":
        a, b = PC.pair("farxy-320x64")
        return np.ascontiguousarray(a.T), np.ascontiguousarray(b.T)
    return PC.pair(frame)


def smooth_field(w, h, seed, mean=(0.0, 0.0), amp=0.6):
    """A seeded field of four long waves per component around `mean`, f32 (H, W, 2)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((h, w, 2))
    for c in range(2):
        f = np.full((h, w), float(mean[c]))
        for _ in range(4):
            lam, th, ph = rng.uniform(25, 90), rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
            f += amp / 2 * rng.uniform(0.3, 1.0) * np.sin(2 * np.pi * (np.cos(th) * x + np.sin(th) * y) / lam + ph)
        out[..., c] = f
    return np.ascontiguousarray(out, np.float32)


def oracle_dense_flow(img_a, img_b, psz=15, lv_f=2, step=4):
    """patchflow.dense_flow with the nodes tracked by the host oracle (oracle/np_patchflow.track_points)."""
    from invcompcamtrack_amd import patchflow as pf
    from oracle import oracle as O
    pa, pb = O.Pyramid(img_a, lv_f, psz), O.Pyramid(img_b, lv_f, psz)
    return pf.dense_flow(pa, pb, step, psz, lv_f,
                         _track=lambda a, b, pts, psz, lv_f, maxiter, eps: NP.track_points(a, b, pts, psz, lv_f, 0, maxiter,
                                                                                           eps))


# ---------------------------------------------------------------- the edge-shape table
# (w, h) -> seed. The shapes at which a tiled stencil with a 2-pixel halo and a colour-compacted plane goes wrong: the
# 4 x 4 minimum, exactly one and two tiles, a last tile one or two pixels wide or high, odd and even widths (the two colours'
# rows differ in length), and widths whose half-sweep has a second workgroup in x of one lane (129) or of none (128). A
# seed is the first of 0, 1, 2, .. at which EDGE_OUTSIDE of F0's positions are outside the frame (between the 6 % that the
# pushed row and column are of 32 x 32 and the 44 % that they are of 4 x 4) and no warped position of the definition comes
# within BOUNDARY_PX of the inside boundary in any outer iteration of any run used on the entry (edge_runs): nothing is
# left out on these frames. test_flowrefine_cpu.py checks both. Measured shares: 44, 40, 40, 23, 12, 20, 11, 11, 7, 9, 21,
# 21, 35, 29 % in the table's order; the shift's sign puts pixels of a third or fourth side outside on ten of the fourteen.
EDGE_SEEDS = {(4, 4): 3, (5, 4): 9, (4, 5): 2, (16, 16): 0, (17, 16): 0, (16, 17): 0, (18, 33): 0, (33, 18): 2,
              (31, 31): 0, (32, 32): 0, (129, 5): 0, (5, 129): 0, (128, 6): 0, (130, 7): 0}
EDGE_OUTSIDE = (0.06, 0.45)
EDGE = tuple((f"edge-{w}x{h}", "edge") for w, h in EDGE_SEEDS)
EDGE_RUNS = (RUNS[0], RUNS[1])
EDGE_PUSH = (3.0, 2.5)  # the first row goes up by the first, the last column right by the second (px)
# (alpha, gamma, delta, omega): one data term off, both off (the right-hand side is the smoothness term alone), all three
# far from their defaults with under-relaxation. Each runs (3, 5, omega) on PARAM_CASES, with and without x_only.
PARAMS = ((16.0, 0.0, 4.5, 1.6), (16.0, 13.0, 0.0, 1.0), (3.0, 0.0, 0.0, 1.9), (40.0, 2.0, 9.0, 0.5))
PARAM_CASES = (("67x53", "smooth"), ("edge-33x18", "edge"), ("edge-17x16", "edge"))


def weight_args(weights):
    return {} if weights is None else dict(zip(("alpha", "gamma", "delta"), weights))


def pad_extra(frame):
    """What a test's pyramids of `frame` are padded by beyond its patch size: 0, 1, 5 in rotation over EDGE, so that a
    plane's stride is neither its width nor a fixed offset from it; 0 for the other frames."""
    names = [f for f, _ in EDGE]
    return (0, 1, 5)[names.index(frame) % 3] if frame in names else 0


def _edge_shift(frame):
    """The pair's shift: 0.3 .. 0.9 px per component, either sign."""
    w, h = frame_size(frame)
    rng = np.random.default_rng(4000 + EDGE_SEEDS[w, h] + 17 * w + h)
    return tuple(rng.uniform(0.3, 0.9, 2) * rng.choice((-1.0, 1.0), 2))


def _edge_pair(frame):
    w, h = frame_size(frame)
    seed = EDGE_SEEDS[w, h] + 17 * w + h
    sx, sy = _edge_shift(frame)
    a = texture(w, h, 1000 + seed)
    b = texture(w, h, 1000 + seed, lambda X, Y: (X - sx, Y - sy))
    return _noisy(a, 2000 + seed), _noisy(b, 3000 + seed)


def _edge_f0(frame):
    """smooth_field around the pair's shift (amplitude 0.3 px), the first row pushed up and the last column pushed right
    by EDGE_PUSH: the clamp and the inside mask act there, and wherever the shift itself leaves the frame."""
    w, h = frame_size(frame)
    out = smooth_field(w, h, 5000 + EDGE_SEEDS[w, h] + 17 * w + h, _edge_shift(frame), amp=0.3).copy()
    out[0, :, 1] -= np.float32(EDGE_PUSH[0])
    out[:, -1, 0] += np.float32(EDGE_PUSH[1])
    return out


def edge_runs(frame, kind):
    """Every (n_outer, n_sor, omega, x_only, weights) that a test runs the definition with on an EDGE entry."""
    out = [run + (x_only, None) for run in (STAGE_RUN,) + EDGE_RUNS for x_only in (False, True)]
    if (frame, kind) in PARAM_CASES:
        out += [(3, 5, p[3], x_only, p[:3]) for p in PARAMS for x_only in (False, True)]
    return out


def outside_share(frame, kind):
    """The share of F0's positions outside the frame."""
    f = f0(frame, kind)
    h, w = f.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    px, py = xx + f[..., 0].astype(np.float64), yy + f[..., 1].astype(np.float64)
    return float(1.0 - ((px >= 0) & (px <= w - 1) & (py >= 0) & (py <= h - 1)).mean())


def far_field(frame, kind):
    """F0 with its first six rows sent 400 px and its last six 1e6 px out of the frame."""
    f = f0(frame, kind).copy()
    f[:6] += 400.0
    f[-6:] -= 1e6
    return f


@functools.lru_cache(maxsize=None)
def restated(frame, kind, n_outer, n_sor, omega, x_only, weights=None):
    """(refined field, trace) of the f32 restatement; shared, do not write to it."""
    import flowrefine_f32 as R
    a, b = pair(frame)
    tr = []
    out = R.refine(a, b, f0(frame, kind), n_outer=n_outer, n_sor=n_sor, omega=omega, x_only=x_only, trace=tr,
                   **weight_args(weights))
    return out, tr


@functools.lru_cache(maxsize=None)
def f0(frame, kind):
    """The input flow of a table entry, f32 (H, W, 2); shared, do not write to it."""
    w, h = frame_size(frame)
    if kind == "edge":
        out = _edge_f0(frame)
    elif kind == "dense":
        a, b = pair(frame)
        out = oracle_dense_flow(a, b)
    else:
        mean = SHIFT.get(frame, (-0.4, -2.4))
        out = smooth_field(w, h, 7 * len(frame) + w, mean)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------- recorded differences of the f32 restatement
# worst |restatement - definition| over TABLE after ONE outer iteration (n_sor = 5, omega = 1.6) per stage plane; "sweep"
# is one half-sweep of each colour from the definition's own coefficients (du, dv). Measured by test_flowrefine_cpu.py.
STAGE_DIFF = {"bw": 2.7e-4, "a11": 64.0, "a12": 17.1, "a22": 25.3, "b1": 0.081, "b2": 0.054, "wr": 6.5e-4, "wd": 4.9e-4,
              "du": 2.6e-4, "dv": 1.3e-4, "sweep": 1.2e-6}
# worst |restatement - definition| of the refined field over TABLE per (n_outer, n_sor, omega, x_only), pixels near the
# inside boundary left out
FULL_DIFF = {(1, 1, 1.0, False): 5.4e-5, (1, 1, 1.0, True): 5.4e-5, (3, 5, 1.6, False): 5.2e-4, (3, 5, 1.6, True): 2.7e-4,
             (8, 5, 1.6, False): 4.4e-4, (8, 5, 1.6, True): 6.1e-5}

# the same over EDGE (both with and without x_only), where nothing is left out; and per weights of PARAMS the worst of the
# refined field after (3, 5, omega) over PARAM_CASES. The device is held to the restatement's bits on all of them, so no
# margin multiplies these: they say how far the restatement, which is written from the kernels, is from the definition,
# which has no tiles, at the shapes where a misreading of a tile's edge would show.
EDGE_STAGE_DIFF = {"bw": 7.5e-5, "a11": 5.1, "a12": 0.72, "a22": 1.53, "b1": 8.3e-3, "b2": 1.7e-3, "wr": 4.4e-4,
                   "wd": 4.8e-4, "du": 7.8e-5, "dv": 1.7e-4, "sweep": 1.1e-6}
# (the single sweep's 4.9e-4 is one pixel of 5 x 129 whose brightness residual is nearly 0: its robust weight turns the
# rounding of Bw into 1 part in 600 of a11, and du is 0.49 px there; the next largest difference of that run is 3.5e-5)
EDGE_FULL_DIFF = {(1, 1, 1.0, False): 5.0e-4, (1, 1, 1.0, True): 5.0e-4, (3, 5, 1.6, False): 1.9e-4,
                  (3, 5, 1.6, True): 8.6e-5}
PARAM_DIFF = {PARAMS[0]: 1.2e-4, PARAMS[1]: 1.5e-5, PARAMS[2]: 1.2e-4, PARAMS[3]: 1.5e-5}
NAN_AT = (9, 12)  # (x, y) of the pixel whose u is a NaN in the tests of a field that is not finite


@functools.lru_cache(maxsize=None)
def host_run(frame, kind, n_outer, n_sor, omega, x_only, weights=None):
    """(refined field, trace, boundary mask) of the definition; the mask marks the pixels whose warped position came
    within BOUNDARY_PX of the inside boundary in any outer iteration. weights: (alpha, gamma, delta), None: the
    defaults."""
    from invcompcamtrack_amd import patchflow as pf
    a, b = pair(frame)
    tr = []
    out = pf.refine_flow_host(a, b, f0(frame, kind), n_outer=n_outer, n_sor=n_sor, omega=omega, x_only=x_only, _trace=tr,
                              **weight_args(weights))
    h, w = a.shape
    near = np.zeros((h, w), bool)
    for t in tr:
        for p, hi in ((t["px"], w - 1), (t["py"], h - 1)):
            near |= (np.abs(p) < BOUNDARY_PX) | (np.abs(p - hi) < BOUNDARY_PX)
    assert near.mean() <= BOUNDARY_SHARE, (frame, kind, "choose another input: pixels at the inside boundary", near.mean())
    return out, tr, near


def full_error(frame, kind, n_outer, n_sor, omega, x_only, got, weights=None):
    """Worst |got - definition| outside the boundary mask."""
    ref, _, near = host_run(frame, kind, n_outer, n_sor, omega, x_only, weights)
    return float(np.abs(got.astype(np.float64) - ref.astype(np.float64))[~near].max())


# ---------------------------------------------------------------- the checks, shared by the restatement and the device
COEF_PLANES = ("a11", "a12", "a22", "b1", "b2", "wr", "wd")
STAGE_RUN = (1, 5, 1.6)   # the stage planes are compared after ONE outer iteration: both sides start from F0's bits


def warp_error(frame, kind, bw):
    """(worst |bw - definition|, bound) of a warp of pair(frame)'s B by F0.

    The definition's bilinear rule (patchflow._fr_warp, f64) is evaluated at the positions x + u, y + v ROUNDED TO F32, as
    an f32 kernel forms them: the rounding of the position itself (half an ulp of a coordinate of up to 320, times the
    image gradient) is a property of the number format and far larger than the arithmetic that the bound is about. From
    there on: fx = px - x0 is exact, 1 - fx is rounded once (u = 2^-24), a weight is a product of two such factors
    (relative error <= 3u), each of the four products with B adds u (<= 4u), and the three sums of the convex combination
    add at most u each on partial sums that do not exceed max|B| in magnitude: <= (4 + 3) u max|B| < 8 u max|B|."""
    from invcompcamtrack_amd import patchflow as pf
    a, b = pair(frame)
    f = f0(frame, kind)
    h, w = b.shape
    yy, xx = np.mgrid[0:h, 0:w]
    px = (xx.astype(np.float32) + f[..., 0]).astype(np.float64)
    py = (yy.astype(np.float32) + f[..., 1]).astype(np.float64)
    ref, _ = pf._fr_warp(b.astype(np.float64), px, py)
    return float(np.abs(bw.astype(np.float64) - ref).max()), 8 * U * float(np.abs(b).max())


def stage_errors(frame, kind, x_only, planes):
    """{name: worst |plane - definition|} after one outer iteration (STAGE_RUN) for the planes given (a dict)."""
    _, tr, near = host_run(frame, kind, *STAGE_RUN, x_only)
    return {k: float(np.abs(p.astype(np.float64) - tr[0][k])[~near].max()) for k, p in planes.items()}


@functools.lru_cache(maxsize=None)
def sweep_inputs(frame, kind):
    """The planes a half-sweep is injected with, all f32: the definition's coefficients of the first outer iteration
    rounded to f32, u, v = F0, and seeded du, dv of N(0, 0.05 px)."""
    _, tr, _ = host_run(frame, kind, *STAGE_RUN, False)
    f = f0(frame, kind)
    rng = np.random.default_rng(3)
    out = {k: np.ascontiguousarray(tr[0][k], np.float32) for k in COEF_PLANES}
    out.update(u=f[..., 0].copy(), v=f[..., 1].copy(), du=rng.normal(0, 0.05, f.shape[:2]).astype(np.float32),
               dv=rng.normal(0, 0.05, f.shape[:2]).astype(np.float32))
    return out


def sweep_error(frame, kind, colour, x_only, du, dv):
    """Worst |du, dv - definition| after one half-sweep of `colour` from sweep_inputs."""
    from invcompcamtrack_amd import patchflow as pf
    p = {k: v.astype(np.float64) for k, v in sweep_inputs(frame, kind).items()}
    pf._fr_half_sweep(colour, 1.6, x_only, p["u"], p["v"], p["du"], p["dv"], *[p[k] for k in COEF_PLANES])
    return float(max(np.abs(du - p["du"]).max(), np.abs(dv - p["dv"]).max()))


# ---------------------------------------------------------------- usefulness scenes
def texture(w, h, seed, warp=None):
    """A seeded analytic texture of ten waves (7 .. 40 px) sampled at warp(x, y) (identity by default), f64."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    if warp is not None:
        x, y = warp(x, y)
    out = np.full(x.shape, 128.0)
    for _ in range(10):
        lam, th, ph, amp = rng.uniform(7, 40), rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi), rng.uniform(8, 22)
        out += amp * np.sin(2 * np.pi * (np.cos(th) * x + np.sin(th) * y) / lam + ph)
    return out


def _noisy(img, seed, sigma=2.0):
    return np.ascontiguousarray(img + np.random.default_rng(seed).normal(0, sigma, img.shape), np.float32)


SCENE_W, SCENE_H = 160, 96
RECT = (50, 28, 110, 68)           # x0, y0, x1, y1 of the 60 x 40 layer in frame A
D_BG, D_RECT = (1.3, 0.4), (-1.7, 0.8)


@functools.lru_cache(maxsize=None)
def scene(kind, seed, psz=15):
    """(img_a, img_b, F0, truth, mask): frames with sigma = 2 grey levels of noise, the input flow, the true flow and the
    pixels the mean endpoint error is taken over.
      "layers"  a 60 x 40 rectangle moving by D_RECT over a background moving by D_BG; F0 from the host oracle's
                tracking; mask: pixels 1 .. 8 px from the motion boundary
      "rotzoom" rotation by 1.5 degrees and zoom 1.02 about the centre; F0 likewise; mask: 16 px inside the frame
      "nodes"   the same motion; F0 is the truth at the grid nodes + N(0, 0.15 px), up-sampled (no tracker); mask: 8 px
                inside the frame"""
    w, h = SCENE_W, SCENE_H
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    # rotation by 1.5 degrees and zoom 1.02 about the centre, and its inverse
    cx, cy, th, z = (w - 1) / 2, (h - 1) / 2, np.deg2rad(1.5), 1.02
    c, s = np.cos(th), np.sin(th)
    fwd = lambda X, Y: (cx + z * (c * (X - cx) - s * (Y - cy)), cy + z * (s * (X - cx) + c * (Y - cy)))
    inv = lambda X, Y: (cx + (c * (X - cx) + s * (Y - cy)) / z, cy + (-s * (X - cx) + c * (Y - cy)) / z)
    if kind == "layers":
        x0, y0, x1, y1 = RECT
        in_a = (x >= x0) & (x < x1) & (y >= y0) & (y < y1)
        a = np.where(in_a, texture(w, h, 100 + seed), texture(w, h, 200 + seed))
        xr, yr = x - D_RECT[0], y - D_RECT[1]
        in_b = (xr >= x0) & (xr < x1) & (yr >= y0) & (yr < y1)
        b = np.where(in_b, texture(w, h, 100 + seed, lambda X, Y: (X - D_RECT[0], Y - D_RECT[1])),
                     texture(w, h, 200 + seed, lambda X, Y: (X - D_BG[0], Y - D_BG[1])))
        truth = np.where(in_a[..., None], np.array(D_RECT), np.array(D_BG))
        dist = np.full((h, w), np.inf)  # Chebyshev distance to the nearest pixel of the other layer
        ys, xs = np.nonzero(in_a)
        yo, xo = np.nonzero(~in_a)
        dist[in_a] = _cheb_to_outside(xs, ys, RECT)
        dist[~in_a] = _cheb_to_rect(xo, yo, RECT)
        mask = (dist >= 1) & (dist <= 8)
    elif kind == "rotzoom":
        a, b = texture(w, h, 300 + seed), texture(w, h, 300 + seed, inv)
        fx, fy = fwd(x, y)
        truth = np.stack([fx - x, fy - y], -1)
        mask = (x >= 16) & (x < w - 16) & (y >= 16) & (y < h - 16)
    elif kind == "nodes":  # the same motion as "rotzoom", other textures
        a, b = texture(w, h, 500 + seed), texture(w, h, 500 + seed, inv)
        fx, fy = fwd(x, y)
        truth = np.stack([fx - x, fy - y], -1)
        mask = (x >= 8) & (x < w - 8) & (y >= 8) & (y < h - 8)
    else:
        raise KeyError(kind)
    a, b = _noisy(a, 2 * seed + 1), _noisy(b, 2 * seed + 2)
    if kind == "nodes":
        from invcompcamtrack_amd import patchflow as pf
        step = 4
        rng = np.random.default_rng(600 + seed)
        xs, ys = np.arange(step // 2, w, step), np.arange(step // 2, h, step)
        nodes = truth[ys][:, xs] + rng.normal(0, 0.15, (len(ys), len(xs), 2))
        f = pf.dense_flow(_Size(w, h), None, step, _track=lambda pa, pb, pts, **k: (
            (pts + nodes.reshape(-1, 2)).astype(np.float32), np.ones(len(pts), bool), None))
    else:
        f = oracle_dense_flow(a, b, psz=psz)
    for arr in (a, b, f, truth, mask):
        arr.setflags(write=False)
    return a, b, f, truth, mask


class _Size:
    def __init__(self, w, h):
        self.w, self.h = w, h


def _cheb_to_rect(xs, ys, rect):
    x0, y0, x1, y1 = rect
    dx = np.maximum(np.maximum(x0 - xs, xs - (x1 - 1)), 0)
    dy = np.maximum(np.maximum(y0 - ys, ys - (y1 - 1)), 0)
    return np.maximum(dx, dy).astype(np.float64)


def _cheb_to_outside(xs, ys, rect):
    x0, y0, x1, y1 = rect
    return np.minimum(np.minimum(xs - x0, x1 - 1 - xs), np.minimum(ys - y0, y1 - 1 - ys)).astype(np.float64) + 1


def epe(flow, truth, mask):
    """Mean endpoint error over the mask, px."""
    d = flow.astype(np.float64) - truth
    return float(np.hypot(d[..., 0], d[..., 1])[mask].mean())


SEEDS = (0, 1, 2)
# kind -> (n_outer, ratio): ratio is the definition's worst after / before over SEEDS (mean endpoint errors over the
# scene's mask), measured by test_flowrefine_cpu.py on the host function alone: layers 0.945 -> 0.464, 0.923 -> 0.419,
# 0.977 -> 0.652 px; rotzoom 0.104 -> 0.075, 0.077 -> 0.055, 0.084 -> 0.064; nodes 0.128 -> 0.052, 0.125 -> 0.047,
# 0.123 -> 0.051. The bar is after <= useful_bar(kind) * before: the measured ratio plus a quarter of the measured gain.
# Taking the worst seed as the measured ratio makes the definition hold the bar on all three seeds without picking seeds.
USEFUL = {"layers": (8, 0.668), "rotzoom": (3, 0.765), "nodes": (3, 0.411)}


def useful_bar(kind):
    ratio = USEFUL[kind][1]
    return ratio + (1.0 - ratio) / 4
