"""Cases, recorded differences and usefulness scenes for the coarse-to-fine dense flow (csrc/ictr_c2fflow.hip), shared by
test_c2fflow_cpu.py and test_gpu_c2fflow.py.

The definition is patchflow.c2f_flow_host (f64). c2fflow_f32.py restates the kernel and its launcher in f32; the GPU tests
demand its bits of the device, per level and of the final field. The CPU module compares the restatement with the
definition level by level from the SAME starts (the definition's coarser field), so that one differing decision does not
cascade, on the nodes where every decision of the definition has its margin; the worst differences are RECORDED here and
measured again by test_c2fflow_cpu.py, which fails above a record or below half of it. Nothing here is fitted to the device.
"""
from __future__ import annotations

import functools

import numpy as np

import flowrefine_cases as FC
from oracle import np_patchflow as NP

PAD_EXTRA = (0, 1, 5)          # pyramids padded by psz + one of these, in rotation over the table
REFINE = dict(n_outer=1, n_sor=2)
# (frame, psz, lv_f, maxiter, eps, refine, step): 100x77 and 67x53 halve oddly (67 -> 34 -> 17, 53 -> 26 -> 13); psz 8 /
# 15 / 23, 32 reach the forms 11 / 41 / 82; every psz has an entry with eps = 0, where no stop decision exists and every
# node runs maxiter. The clamp of the start's row: a level of 4 m + 1 rows halves to 2 m, and a node in its last row 4 m
# asks for row 2 m. At step 4 the nodes sit at 2 + 4 k and never stand there; the last entry, at step 3, has node row 52 of
# the 53 rows of level 0 ask for row 26 of 26.
TABLE = (
    ("100x77", 8, 2, 10, 0.01, None, 4),
    ("100x77", 8, 2, 10, 0.0, None, 4),
    ("100x77", 15, 2, 10, 0.01, None, 4),
    ("100x77", 8, 2, 10, 0.01, "refine", 4),
    ("67x53", 8, 2, 10, 0.01, None, 4),
    ("67x53", 8, 1, 10, 0.01, None, 4),
    ("67x53", 15, 2, 10, 0.0, None, 4),
    ("67x53", 15, 2, 2, 0.01, None, 4),
    ("67x53", 23, 2, 10, 0.01, None, 4),
    ("67x53", 23, 2, 10, 0.0, None, 4),
    ("67x53", 32, 2, 10, 0.0, None, 4),
    ("farxy-320x64", 8, 2, 10, 0.01, None, 4),
    ("farxy-320x64", 15, 2, 10, 0.01, None, 4),
    ("farxy-64x320", 8, 2, 10, 0.0, None, 4),
    ("farxy-64x320", 15, 2, 10, 0.01, None, 4),
    ("status-96x64", 8, 2, 10, 0.01, None, 4),
    ("67x53", 8, 2, 10, 0.01, None, 3),
)
assert {c[1] for c in TABLE if c[4] == 0.0} == {8, 15, 23, 32}


# The status pair in the other two forms, outside TABLE (whose entries also feed the definition-distance records): psz 15
# is form <4,1>, psz 17 form <8,2> (289 pixels: more than 4 per lane of one wave), where a stopped node keeps running its
# workgroup's iteration slots and its reason has to survive them. On the restatement every status value occurs over the
# three levels of each (counts of 0..4 at pad psz + 1: 18, 413, 35, 33, 5 and 18, 420, 35, 30, 1; psz 23 has no HELD_FAR
# node). test_c2fflow_cpu.py asserts that; test_gpu_c2fflow.py demands the restatement's bits of the device.
STATUS_FORMS = (("status-96x64", 15, 2, 10, 0.01, None, 4), ("status-96x64", 17, 2, 10, 0.01, None, 4))


def pad_of(case):
    return case[1] + (1 if case in STATUS_FORMS else PAD_EXTRA[TABLE.index(case) % 3])


def refine_of(case):
    return REFINE if case[5] else None


@functools.lru_cache(maxsize=None)
def status_pair(seed=0, w=96, h=64):
    """A seeded pair on which every status value occurs at some level (psz 8, lv_f 2): the content moves by (-6.5, 0.5)
    and leaves over the left edge (nodes whose start is out of view: 0; nodes that walk out: 3); a flat band, the same
    in both frames (2); a ramp block whose brightness jumps by 45 grey levels, so that the step never settles (4)."""
    rng = np.random.default_rng(seed)
    a = FC.texture(w, h, 700 + seed)
    b = FC.texture(w, h, 700 + seed, lambda X, Y: (X + 6.5, Y - 0.5))
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    blk = (slice(4, 36), slice(48, 92))
    ramp = 100 + 2.5 * x + 1.5 * y + 3.0 * np.sin(x * 0.9) * np.cos(y * 0.7)
    a[blk], b[blk] = ramp[blk], ramp[blk] + 45.0
    a, b = a + rng.normal(0, 0.5, a.shape), b + rng.normal(0, 0.5, b.shape)
    a[40:64, 56:96] = b[40:64, 56:96] = 90.0
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)


def frame_size(frame):
    return (96, 64) if frame == "status-96x64" else FC.frame_size(frame)


def pair(frame):
    return status_pair() if frame == "status-96x64" else FC.pair(frame)


_pyr = {}


def host_pyramids(frame, pad, lv_f=2):
    """(oracle.Pyramid A, B) of a frame pair; shared, do not write to them. Needs the built oracle."""
    from oracle import oracle as O
    if (frame, pad, lv_f) not in _pyr:
        a, b = pair(frame)
        _pyr[frame, pad, lv_f] = (O.Pyramid(a, lv_f, pad), O.Pyramid(b, lv_f, pad))
    return _pyr[frame, pad, lv_f]


@functools.lru_cache(maxsize=None)
def host_run(case):
    """(field, stages) of the definition on a table entry."""
    from invcompcamtrack_amd import patchflow as pf
    frame, psz, lv_f, maxiter, eps, _, step = case
    st = []
    out = pf.c2f_flow_host(*host_pyramids(frame, pad_of(case)), step, psz, lv_f, maxiter, eps, refine=refine_of(case),
                           _stages=st)
    return out, st


@functools.lru_cache(maxsize=None)
def restated(case, defect=None):
    """(field, [(level, field, d, status)]) of the f32 restatement on a table entry."""
    import c2fflow_f32 as R
    frame, psz, lv_f, maxiter, eps, _, step = case
    st = []
    out = R.run(*host_pyramids(frame, pad_of(case)), step, psz, lv_f, maxiter, eps, refine=refine_of(case), defect=defect,
                stages=st)
    return out, st


# ---------------------------------------------------------------- restatement against definition
# A node is compared where every decision of the definition has its margin.
MARGIN_EPS, MARGIN_PX, MARGIN_DET = 1e-4, 1e-3, 1e-5
LEFT_OUT_CAP, LEFT_OUT_MIN_NODES = 0.10, 20


def compared(stage, eps):
    """(ny, nx) bool: the nodes of a definition's level whose decisions all have their margins."""
    m = stage["margins"]
    ok = (m["view"] >= MARGIN_PX) & (m["far"] >= MARGIN_PX) & (m["det"] >= MARGIN_DET)
    if eps > 0:  # (with eps = 0 no stop decision exists)
        ok &= m["eps"] >= MARGIN_EPS
    return ok


def level_differences(case, defect=None):
    """Per level of a table entry, the restatement's search from the definition's own starts against the definition:
    [(level, nodes, left out, statuses equal on the compared nodes, worst |d - definition| on them)]."""
    import c2fflow_f32 as R
    frame, psz, lv_f, maxiter, eps, _, step = case
    pa, pb = host_pyramids(frame, pad_of(case))
    out = []
    for s in host_run(case)[1]:
        keep = compared(s, eps)
        d, lost, status = R.search(pa, pb, s["level"], s["init"], step, psz, maxiter, eps, defect=defect)
        same = bool(np.array_equal(status[keep], s["status"][keep]))
        votes = keep & (s["status"] != 0) & ~lost
        diff = float(np.abs(d.astype(np.float64) - s["d"])[votes].max()) if votes.any() else 0.0
        out.append((s["level"], keep.size, int((~keep).sum()), same, diff))
    return out


# level -> worst |restatement - definition| of d in px over TABLE on the compared nodes, from the same starts; measured
# by test_c2fflow_cpu.py. Levels 0 and 1 are set by the status pair, whose runaway nodes move by several px per step; without
# it the table stays below 1.4e-5 / 6.0e-6.
D_DIFF = {0: 3.3e-4, 1: 5.4e-4, 2: 3.3e-6}
# worst |restatement - definition| of the final field in px over the entries with eps = 0 (whole runs, each from its own
# coarser field), measured there too
FIELD_DIFF = 1.1e-5
# the worst share of nodes left out at a level of 20 nodes or more (cap: LEFT_OUT_CAP), measured there too on the
# definition alone, with its entry
LEFT_OUT = (0.069, ("farxy-320x64", 15, 1))   # 22 of 320 nodes; most levels are at 0 - 3 %, nearly all the eps stop

# ---------------------------------------------------------------- usefulness
BIG_BG, BIG_RECT = (6.5, 2.0), (-8.5, 4.0)
USEFUL_PSZ, USEFUL_LV, STEP = 8, 3, 4


@functools.lru_cache(maxsize=None)
def big_scene(seed):
    """flowrefine_cases' two-layer scene with the motions BIG_BG / BIG_RECT: (img_a, img_b, truth, mask), mask 16 px
    inside the frame."""
    w, h = FC.SCENE_W, FC.SCENE_H
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x0, y0, x1, y1 = FC.RECT
    in_a = (x >= x0) & (x < x1) & (y >= y0) & (y < y1)
    a = np.where(in_a, FC.texture(w, h, 100 + seed), FC.texture(w, h, 200 + seed))
    xr, yr = x - BIG_RECT[0], y - BIG_RECT[1]
    in_b = (xr >= x0) & (xr < x1) & (yr >= y0) & (yr < y1)
    b = np.where(in_b, FC.texture(w, h, 100 + seed, lambda X, Y: (X - BIG_RECT[0], Y - BIG_RECT[1])),
                 FC.texture(w, h, 200 + seed, lambda X, Y: (X - BIG_BG[0], Y - BIG_BG[1])))
    truth = np.where(in_a[..., None], np.array(BIG_RECT), np.array(BIG_BG))
    mask = (x >= 16) & (x < w - 16) & (y >= 16) & (y < h - 16)
    return FC._noisy(a, 2 * seed + 1), FC._noisy(b, 2 * seed + 2), truth, mask


def useful_inputs(kind, seed):
    """(img_a, img_b, truth, mask) of a usefulness scene: "big" (big_scene), or a kind of flowrefine_cases.scene with the
    mask 16 px inside the frame."""
    if kind == "big":
        return big_scene(seed)
    a, b, _, truth, _ = FC.scene(kind, seed)
    h, w = a.shape
    y, x = np.mgrid[0:h, 0:w]
    return a, b, truth, (x >= 16) & (x < w - 16) & (y >= 16) & (y < h - 16)


def useful_errors(kind, seed, refine=None):
    """(baseline, coarse-to-fine) mean endpoint errors in px of the definitions: densify_flow_host on the host oracle's
    whole-pyramid nodes against c2f_flow_host, both at USEFUL_PSZ, step 4, USEFUL_LV."""
    from invcompcamtrack_amd import patchflow as pf
    from oracle import oracle as O
    a, b, truth, mask = useful_inputs(kind, seed)
    h, w = a.shape
    pa, pb = O.Pyramid(a, USEFUL_LV, USEFUL_PSZ), O.Pyramid(b, USEFUL_LV, USEFUL_PSZ)
    gx, gy = np.meshgrid(np.arange(STEP // 2, w, STEP, dtype=np.float32), np.arange(STEP // 2, h, STEP, dtype=np.float32))
    pts = np.stack([gx.ravel(), gy.ravel()], 1)
    new, ok, _ = NP.track_points(pa, pb, pts, USEFUL_PSZ, USEFUL_LV, 0, 10, 0.01)
    lost = ~np.asarray(ok, bool).reshape(gx.shape)
    d = np.asarray(new - pts, np.float32).reshape(gx.shape + (2,))
    d[lost] = 0
    base = pf.densify_flow_host(a, b, d, lost, STEP, USEFUL_PSZ)
    if refine is not None:
        base = pf.refine_flow_host(a, b, base, **refine)
    c2f = pf.c2f_flow_host(pa, pb, STEP, USEFUL_PSZ, USEFUL_LV, refine=refine)
    return FC.epe(base, truth, mask), FC.epe(c2f, truth, mask)


# "big": the definition's worst coarse-to-fine / baseline ratio over flowrefine_cases.SEEDS, measured by
# test_c2fflow_cpu.py on the host functions alone. The bar is flowrefine_cases.useful_bar's form: the worst seed's ratio
# plus a quarter of its gain.
# Mean endpoint errors baseline -> coarse-to-fine: 2.162 -> 1.027, 3.972 -> 2.212, 2.129 -> 1.497 px (ratios 0.475, 0.557,
# 0.703). Without a bar: "layers" 0.277 -> 0.275, 0.294 -> 0.289, 0.306 -> 0.298; "rotzoom" 0.105 -> 0.104, 0.074 -> 0.074,
# 0.094 -> 0.093; "big" with USEFUL_REFINE on both sides 1.876 -> 1.041, 3.711 -> 2.244, 1.866 -> 1.360.
USEFUL_BIG = 0.703
# scenes where no gain is expected: the coarse-to-fine error may be at most NO_WORSE x the baseline's
NO_WORSE = 1.05
USEFUL_REFINE = dict(n_outer=3, n_sor=5)   # the run with refinement, recorded without a bar


def useful_bar():
    return USEFUL_BIG + (1.0 - USEFUL_BIG) / 4
