"""Cases, oracle records and tolerances for the patch-flow kernel (csrc/ictr_patchflow.hip), shared by
test_patchflow_cpu.py, test_gpu_patchflow_forms.py and the child processes of the latter (patchflow_child.py).

A *job* is one launch of k_patchflow: a frame pair, a patch size, a pyramid padding, a level range, an iteration cap and
a point array. The jobs are listed per *group*: group 0 runs with the default dispatch, groups 1 and 2 with ICTR_PF_WPP=1
and 2 in the environment (read once per process, hence one child process each). The oracle is oracle/np_patchflow (f64
sums over the f32 patch values) on the planes of oracle.Pyramid, which are bit-equal to the device's.

Tolerances (nothing here is fitted to the device):
  one step   (new - pts) / 2^l against one_step's derived bound (np_patchflow's docstring) plus u |new| / 2^l, the half
             ulp of the f32 level-0 position the kernel returns, u = 2^-24
  full run   FULL_MARGIN * FULL_FACTOR * (sum of the one-step bounds of the oracle's steps, each * 2^l, + u |new|).
             FULL_FACTOR is the worst ratio of the f32 restatement (patchflow_f32.py) against the f64 oracle over the
             table, measured by test_patchflow_cpu.py, which fails if it is exceeded; FULL_MARGIN = 4 because the device
             adds in another order than the restatement.
  decisions  status and iters are demanded exactly. The inputs are chosen so that every decision of the oracle (in view,
             conditioning, convergence) is further from its threshold than the run's tolerance: check_margins.

The far jobs (FAR, far_jobs) are a second, short list on analytic frames of up to 576 px whose displacement is known in
advance: they hold the first-tap rule at coordinates of 256 and more and one ulp either side of an integer (check_truth,
check_continuity, check_grid), through the same compare_step and compare_full.
"""
from __future__ import annotations

import functools
from collections import OrderedDict, namedtuple

import numpy as np

from oracle import np_patchflow as NP

LV = 2                                  # every pyramid has levels 0..2
U = 2.0 ** -24
EPS, MAXITER = 0.005, 8                 # full runs
MIN_DET = 1e-4                          # the kernel's conditioning threshold (PFArgs.min_det)
FULL_FACTOR = 0.125                       # measured: see DESIGN.md "Patch flow: forms, bound, padding"; the CPU module checks it
FULL_MARGIN = 4.0
# det / tr^2 of an f32 evaluation differs from the oracle's by less than 2 (L + c) u < 3e-6 (L + c <= 24; the terms of
# hxx hyy and hxy^2 are all <= tr^2 / 4): a decision 1e-5 away from min_det cannot flip
DET_MARGIN = 1e-5
INTERIOR_COND = 0.01                    # every interior point has det > 0.01 tr^2 at every level (a condition on the inputs)

GROUP_PSZ = {0: (1, 8, 9, 15, 16, 17, 31, 32), 1: (17, 31, 32), 2: (8, 15)}
# psz -> NPL * 10 + WPP
GROUP_FORM = {0: {1: 11, 8: 11, 9: 41, 15: 41, 16: 41, 17: 82, 31: 82, 32: 82}, 1: {17: 161, 31: 161, 32: 161},
              2: {8: 82, 15: 82}}
RANGES = ((0, 0), (1, 1), (2, 2), (2, 1), (2, 0))
KS = (1, 2, 3, 4, 5, 9)
# per group: patch sizes of the K, padding and independence jobs (one per kernel form the group reaches)
GROUP_FORM_PSZ = {0: (8, 15, 31), 1: (31,), 2: (8,)}
PAD_EXTRA = (0, 1, 5)
ROLL = 6

SIZES = {"100x77": (100, 77), "67x53": (67, 53)}
SYNTH_SEED = {"100x77": 4, "67x53": 9}
N_INTERIOR = 10

Job = namedtuple("Job", "key kind frame psz pad lv_f lv_l maxiter pts group")


# ---------------------------------------------------------------- the far frames: coordinates of 256 and more
# name -> (w, h, s, t): A is an analytic texture, B the same function at (x - s, y - t), so the displacement A -> B is
# (s, t) exactly, at sub-pixel size, everywhere. They are not in SIZES: the table above does not grow by them; they have
# a short job list of their own (far_jobs). 320 and 576 are the smallest widths with integer coordinates >= 256 at level
# 0 and at level 1.
FAR = OrderedDict([("farx-320x64", (320, 64, 1.7, 0.0)), ("fary-64x320", (64, 320, 0.0, 1.7)),
                   ("farxy-320x64", (320, 64, 1.3, -0.9)), ("farx-576x64", (576, 64, 1.7, 0.0))])
# (wavelength px, direction degrees, amplitude, phase): wavelengths from 13 to 53 px keep levels 0..2 textured (3 to 13
# px at level 2) and keep a shift of 1.7 px inside every component's half wavelength at level 0
FAR_WAVES = ((13.0, 20.0, 22.0, 0.3), (19.0, 115.0, 18.0, 1.1), (31.0, 65.0, 26.0, 2.0), (53.0, 160.0, 30.0, 4.4))
# Triples (n - 1 ulp, n, n + 1 ulp) along the long axis: 100 - 1 ulp is 25 - 1 ulp at level 2; 512 and 514 are 256 and
# 257 at level 1.
FAR_N, FAR_N_576 = (24, 40, 63, 64, 100, 255, 256, 257, 300), (512, 514)
FAR_INTEGER = (40, 255, 256, 300, 512)              # their coordinate across is an integer too: three weights are exact zeros
# Further points on both sides of 256 (of 512 on the 576 frame): ("half", a) a point on half pixels near a, ("dec", a) a
# point with two decimals within 4 px of a.
FAR_SLOTS = (("half", 200.5), ("dec", 243.0), ("half", 251.5), ("half", 260.5), ("dec", 272.0), ("dec", 299.0))
FAR_SLOTS_576 = (("dec", 200.0), ("dec", 498.0), ("half", 511.5), ("half", 513.5), ("dec", 530.0))
# Per frame: the coordinate across of each triple, and the further points (along, across). Each is the first of its
# candidates (far_candidates) for which every decision of the oracle has its margin (check_margins) at every far job of
# every group, and on farx-320x64 at every far job of the 1-D search too: chosen on the oracle alone, and checked again
# by the CPU modules. (The steps of a run hardly depend on where the patch is in so smooth a texture, so a run that has
# a step near eps has it at many positions: hence the search.)
FAR_CROSS = {
    "farx-320x64": (33.79, 32.0, 33.44, 42.64, 40.04, 20.0, 38.0, 28.28, 38.0),
    "fary-64x320": (27.93, 32.0, 33.44, 42.64, 40.04, 32.0, 32.0, 37.93, 32.0),
    "farxy-320x64": (27.93, 32.0, 33.44, 42.64, 34.32, 26.0, 23.0, 37.93, 41.0),
    "farx-576x64": (26.0, 36.25),
}
FAR_MORE = {
    "farx-320x64": ((203.5, 33.5), (241.84, 33.19), (248.5, 29.5), (261.5, 35.5), (273.02, 36.51), (299.9, 28.95)),
    "fary-64x320": ((202.5, 29.5), (241.84, 33.19), (248.5, 29.5), (263.5, 31.5), (275.82, 26.15), (295.87, 40.63)),
    "farxy-320x64": ((199.5, 34.5), (241.84, 33.19), (248.5, 29.5), (263.5, 31.5), (268.68, 36.44), (295.87, 40.63)),
    "farx-576x64": ((200.6, 43.0), (500.65, 35.54), (508.5, 43.5), (516.5, 27.5), (527.18, 41.64)),
}
FAR_RANGES = ((0, 0), (1, 1), (2, 0))
FAR_MAXITER = 10
# |new - pts - (s, t)| (Euclidean, level-0 px) of a full run at every point, per patch size: twice the f64 oracle's
# worst error over the far jobs' points whose level-0 coordinates are all below 255 (where the tap rule was never in
# doubt), the factor 2 for the other points' other positions in the texture. Measured on the CPU by
# test_patchflow_cpu.py, which fails if a bar is exceeded there or is above 0.25 px, a quarter of the defect.
TRUTH_BAR = {8: 0.093, 15: 0.090, 31: 0.108}             # 2 x (0.0464, 0.0445, 0.0539), rounded up


def far_texture(w, h, s, t):
    """The texture at (x - s, y - t) on the w x h pixel grid, f64 arithmetic, rounded to f32 once."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.full((h, w), 128.0)
    for lam, deg, amp, ph in FAR_WAVES:
        th = np.deg2rad(deg)
        out += amp * np.sin(2 * np.pi * (np.cos(th) * (x - s) + np.sin(th) * (y - t)) / lam + ph)
    return np.ascontiguousarray(out, np.float32)


def far_shift(frame):
    return np.array(FAR[frame][2:], np.float64)


def frame_size(frame):
    if frame in FAR:
        return FAR[frame][:2]
    return SIZES[frame.split("-")[-1]]


@functools.lru_cache(maxsize=None)
def pair(frame):
    """(img_a, img_b) f32. 'WxH': a synth.make_scene pair with a few pixels of motion. 'roll-WxH': B is A rolled by ROLL
    pixels along x. 'flat-WxH': A = B with a constant rectangle (rows 8..h-8, columns 8..w-8). 'rows-WxH': A = B with
    the same rows all equal to one profile. A name of FAR: the analytic pair with its known shift."""
    if frame in FAR:
        w, h, s, t = FAR[frame]
        return far_texture(w, h, 0.0, 0.0), far_texture(w, h, s, t)
    from invcompcamtrack_amd import synth
    kind, _, size = frame.rpartition("-")
    w, h = SIZES[size]
    sc = synth.make_scene(w, h, n_points=4, seed=SYNTH_SEED[size],
                          dp_gt=np.array([0.1, -0.06, 0.05, 0.02, -0.015, 0.01]))
    a, b = sc["img_a"].copy(), sc["img_b"].copy()
    if kind == "roll":
        b = np.roll(a, ROLL, axis=1)
    elif kind == "flat":
        a[8:h - 8, 8:w - 8] = 100.0
        b = a.copy()
    elif kind == "rows":
        a[8:h - 8, :] = a[8, :]
        b = a.copy()
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)


_pyr = {}


def oracle_pyramids(O, frame, pad):
    key = (frame, pad)
    if key not in _pyr:
        a, b = pair(frame)
        _pyr[key] = (O.Pyramid(a, LV, pad), O.Pyramid(b, LV, pad))
    return _pyr[key]


# ---------------------------------------------------------------- point sets
# Points at least 8 px inside the frame; the first on integer coordinates (three of the four weights are exact zeros), the
# second on half pixels. They are the first of 120 uniform draws (two decimals) for which every decision of the oracle
# has its margin (check_margins) at every patch size, form and level range of the table, and det > 0.01 tr^2 at every
# level: chosen on the oracle alone, and checked again by test_patchflow_cpu.py.
INTERIOR = {
    "100x77": [[60, 67], [9.5, 19.5], [68.47, 8.63], [58.09, 30.91], [12.89, 54.64], [23.72, 33.92], [65.56, 29.52],
               [70.49, 35.71], [86.12, 8.54], [89.62, 57.21]],
    "67x53": [[31, 44], [44.5, 44.5], [31.25, 15.35], [13.3, 35.96], [44.88, 44.69], [20.82, 22.57], [9.17, 13.53],
              [48.22, 11.05], [34.28, 44.1], [9.77, 17.54]],
}


def interior(frame):
    return np.array(INTERIOR[frame.split("-")[-1]], np.float32)


def special(frame):
    """Corners of the frame ((w, h) is in view by the <= rule), a point inside level 0 but outside level 1 (h is odd:
    (h - 0.5) / 2 > h // 2), and points that are lost before anything is read."""
    w, h = frame_size(frame)
    return np.array([[0, 0], [w, h], [26.25, h - 0.5], [np.nan, 5], [5, np.nan], [-3, h / 2], [w / 2, -0.5],
                     [np.inf, 5], [w + 0.25, 5]], np.float32)


N_SPECIAL = 9


def leaving(frame):
    """Points within 3 px of the right edge: on the rolled pair the motion (+ROLL px along x) takes them out of view."""
    w, h = frame_size(frame)
    ys = np.linspace(12, h - 12, 6)
    xs = w - np.array([0.4, 1.1, 1.7, 2.2, 2.6, 2.9])
    return np.stack([xs, ys], 1).astype(np.float32)


def textureless(frame):
    w, h = frame_size(frame)
    return np.array([[w / 2, h / 2], [w / 2 - 3.3, h / 2 + 2.6], [w / 2 + 0.5, h / 2 - 1.25]], np.float32)


def nan_interleaved(pts):
    """Every live point followed by a lost one: in the two-wave form each live patch shares its workgroup with a lost
    one (NaN, out of view, NaN: the partner leaves at different places)."""
    out = np.full((2 * len(pts), 2), np.nan, np.float32)
    out[0::2] = pts
    out[3::4] = (-5.0, 3.0)
    return out


# ---------------------------------------------------------------- the job table
def _jobs(group):
    out = []

    def add(key, kind, frame, psz, lv_f, lv_l, maxiter, pts, extra=0):
        out.append(Job(f"g{group}-{key}", kind, frame, psz, psz + extra, lv_f, lv_l, maxiter,
                       np.ascontiguousarray(pts, np.float32), group))

    for psz in GROUP_PSZ[group]:
        for frame in SIZES:
            pts = np.concatenate([interior(frame), special(frame)])
            if psz > 1:  # psz 1 has det = 0 by construction: a status case only
                for l in range(LV + 1):
                    add(f"step-{frame}-p{psz}-l{l}", "step", frame, psz, l, l, 1, pts)
            for lv_f, lv_l in RANGES:
                add(f"full-{frame}-p{psz}-{lv_f}{lv_l}", "full", frame, psz, lv_f, lv_l, MAXITER, pts)
        add(f"leave-p{psz}-20", "full", "roll-100x77", psz, 2, 0, MAXITER, leaving("100x77"))
        add(f"leave-p{psz}-11", "full", "roll-100x77", psz, 1, 1, MAXITER, leaving("100x77"))
        for frame in ("flat-100x77", "rows-100x77"):
            add(f"{frame}-p{psz}-00", "lost", frame, psz, 0, 0, MAXITER, textureless("100x77"))
            if psz <= 17:  # the level-1 region holds the patch and the gradient's support
                add(f"{frame}-p{psz}-11", "lost", frame, psz, 1, 1, MAXITER, textureless("100x77"))
        if psz > 1:
            add(f"maxiter0-p{psz}", "maxiter0", "100x77", psz, 2, 0, 0,
                np.concatenate([interior("100x77"), special("100x77")]))
    for psz in GROUP_FORM_PSZ[group]:
        ipts = interior("100x77")
        for K in KS:
            add(f"K{K}-p{psz}", "full", "100x77", psz, 2, 0, MAXITER, ipts[:K])
        for extra in PAD_EXTRA:
            add(f"pad{extra}-p{psz}", "pad", "100x77", psz, 2, 0, MAXITER, ipts, extra)
        perm = np.random.default_rng(psz).permutation(len(ipts))
        add(f"indep-perm-p{psz}", "indep", "100x77", psz, 2, 0, MAXITER, ipts[perm])
        add(f"indep-nan-p{psz}", "indep", "100x77", psz, 2, 0, MAXITER, nan_interleaved(ipts))
        for k in range(len(ipts)):
            add(f"indep-one{k}-p{psz}", "indep", "100x77", psz, 2, 0, MAXITER, ipts[k:k + 1])
    return out


@functools.lru_cache(maxsize=None)
def jobs(group):
    return OrderedDict((j.key, j) for j in _jobs(group))


def perm_of(psz):
    return np.random.default_rng(psz).permutation(N_INTERIOR)


def form(job):
    return GROUP_FORM[job.group][job.psz]


def form_shape(job):
    """(L + c pieces) of the job's form: (L, WPP)."""
    f = form(job)
    wpp = f % 10
    return NP.lane_pixels(job.psz, wpp), wpp


# ---------------------------------------------------------------- oracle records
_rec = {}


def oracle_full(O, job):
    """(new, status, iters, detail) of the oracle for a job, with the bound summed for the job's form."""
    if job.key not in _rec:
        pa, pb = oracle_pyramids(O, job.frame, job.pad)
        L, wpp = form_shape(job)
        _rec[job.key] = NP.track_points(pa, pb, job.pts, job.psz, job.lv_f, job.lv_l, job.maxiter, EPS, MIN_DET,
                                        detail=True, nsum=L + 7 + (wpp - 1))
    return _rec[job.key]


_step = {}


def oracle_step(O, job):
    """(step, bound, det / tr^2) of one_step for a 'step' job."""
    if job.key not in _step:
        pa, pb = oracle_pyramids(O, job.frame, job.pad)
        L, wpp = form_shape(job)
        _step[job.key] = NP.one_step(pa, pb, job.pts, job.psz, job.lv_f, L, wpp, MIN_DET)
    return _step[job.key]


def full_tolerance(new_o, detail):
    """Per point, level-0 pixels."""
    with np.errstate(invalid="ignore"):
        out = U * np.nan_to_num(np.abs(new_o).max(axis=1))
    return FULL_MARGIN * FULL_FACTOR * (detail["bound"] + out)


def out_ulp(new_o):
    """Per point: the spacing of f32 at the returned position (its larger component), 0 for a lost point."""
    with np.errstate(invalid="ignore"):
        return np.nan_to_num(np.spacing(np.abs(new_o)).astype(np.float64).max(axis=1))


def is_far(job):
    return job.frame in FAR


def check_margins(job, new_o, detail):
    """Every decision the oracle took is further from its threshold than an f32 evaluation can move it. On the far
    frames that includes one spacing of f32 at the position (is_far: see compare_full)."""
    tol = full_tolerance(new_o, detail) + (out_ulp(new_o) if is_far(job) else 0.0)
    # positions at level l move by tol / 2^l <= tol
    assert np.all(detail["view"] > tol), (job.key, "pick another seed: in-view margin", detail["view"], tol)
    assert np.all(detail["eps_px"] > tol), (job.key, "pick another seed: convergence margin", detail["eps_px"], tol)
    assert np.all(detail["det"] > DET_MARGIN), (job.key, "pick another seed: conditioning margin", detail["det"])


def compare_step(job, new, status, iters, O):
    """One-step check of a device (or restatement) result; returns the worst ratio against the bound."""
    step, bound, _ = oracle_step(O, job)
    live = np.isfinite(step[:, 0])
    assert np.array_equal(status, live), (job.key, status, live)
    assert np.all(iters[live] == 1) and np.all(iters[~live] == 0), (job.key, iters)
    assert np.isnan(new[~live]).all(), job.key
    s = 2.0 ** job.lv_f
    got = (new[live].astype(np.float64) - job.pts[live].astype(np.float64)) / s
    err = np.abs(got - step[live])
    ratio = err / (bound[live] + U * np.abs(new[live].astype(np.float64)) / s)
    assert np.all(ratio <= 1.0), (job.key, "worst ratio", float(ratio.max()), "at", np.argwhere(ratio > 1.0).tolist())
    return float(ratio.max()) if ratio.size else 0.0


def compare_full(job, new, status, iters, O):
    """Full-run check: status and iters exactly, positions within full_tolerance; returns the worst ratio against
    bound-sum + u |new| (the quantity FULL_FACTOR scales).

    On the far frames (is_far) one spacing of f32 at the returned position is taken off the error first. Their texture
    is smooth and the arithmetic error of a run small (bound sums of 1e-5 to 6e-5 px), while the grid of positions is
    coarse (2^-15 = 3.05e-5 px from 256 on), so two evaluations whose p differ in the last bits return neighbouring
    floats, a whole spacing apart, where full_tolerance has a quarter of one (4 * 0.125 * u |new|). Everything above that
    spacing is held to the same tolerance and the same FULL_FACTOR as the rest of the table (test_patchflow_cpu.py
    asserts that every excess of the restatement is exactly one spacing); the old table's jobs are compared as before."""
    new_o, ok_o, it_o, det = oracle_full(O, job)
    check_margins(job, new_o, det)
    assert np.array_equal(status, ok_o), (job.key, status, ok_o)
    assert np.array_equal(iters, it_o), (job.key, iters, it_o)
    assert np.isnan(new[~ok_o]).all(), job.key
    if not ok_o.any():
        return 0.0
    err = np.abs(new[ok_o].astype(np.float64) - new_o[ok_o].astype(np.float64)).max(axis=1)
    if is_far(job):
        err = np.maximum(err - out_ulp(new_o)[ok_o], 0.0)
    tol = full_tolerance(new_o, det)[ok_o]
    assert np.all(err <= tol), (job.key, "worst error / tolerance", float((err / tol).max()))
    return float((err / tol).max() * FULL_MARGIN * FULL_FACTOR)


# ---------------------------------------------------------------- the far jobs
def far_axis(frame):
    """0 if the frame's long axis (the one that crosses 256) is x, 1 if it is y."""
    w, h = frame_size(frame)
    return 0 if w > h else 1


def _far_table(frame):
    big = max(frame_size(frame)) == 576
    return (FAR_N_576, FAR_SLOTS_576) if big else (FAR_N, FAR_SLOTS)


def far_candidates(n):
    """Coordinates across for the triple of n, in the order they are tried: integers of 20 .. 44, the middle of the 64
    pixels, for FAR_INTEGER, else two-decimal draws from 20 .. 44 seeded by n."""
    if n in FAR_INTEGER:
        return [32.0, 26.0, 38.0, 23.0, 41.0, 29.0, 35.0, 20.0, 44.0, 21.0, 43.0, 24.0, 40.0, 27.0, 37.0, 30.0, 34.0]
    return np.round(np.random.default_rng(n).uniform(20, 44, 40), 2).tolist()


def far_slot_candidates(kind, a):
    """(along, across) candidates of a further point, in the order they are tried, seeded by a."""
    rng = np.random.default_rng(int(round(10 * a)))
    if kind == "half":
        return [(a + float(j), float(c) + 0.5) for j, c in zip(rng.integers(-3, 4, 40), rng.integers(20, 44, 40))]
    return [(round(a + float(d), 2), round(float(c), 2)) for d, c in zip(rng.uniform(-4, 4, 40), rng.uniform(20, 44, 40))]


def far_rows(frame, cross, more):
    """(K, 2) f32 from the triples' coordinates across and the further points."""
    ns, slots = _far_table(frame)
    assert len(cross) == len(ns) and len(more) == len(slots)
    rows = []
    for n, c in zip(ns, cross):
        v = np.float32(n)
        rows += [(np.nextafter(v, np.float32(-np.inf)), c), (v, c), (np.nextafter(v, np.float32(np.inf)), c)]
    pts = np.array(rows + list(more), np.float32)
    return pts if far_axis(frame) == 0 else np.ascontiguousarray(pts[:, ::-1])


@functools.lru_cache(maxsize=None)
def _far_points(frame):
    return far_rows(frame, FAR_CROSS[frame], FAR_MORE[frame])


def far_points(frame):
    """(K, 2) f32: the triples of the frame's table, three rows each in the table's order, then the further points."""
    return _far_points(frame).copy()


def far_triples(frame):
    """[(n, [k0, k1, k2])]: the rows of far_points that hold n - 1 ulp, n, n + 1 ulp."""
    return [(n, [3 * i, 3 * i + 1, 3 * i + 2]) for i, n in enumerate(_far_table(frame)[0])]


def far_low(frame):
    """Points whose level-0 coordinates are all below 255 and that are not the lower point of a triple of n <= 256 (one
    ulp below an integer <= 64 at level 0, or at level 2 where n / 4 is one): the tap rule was never in doubt there."""
    pts = _far_points(frame)
    near = np.zeros(len(pts), bool)
    for n, ks in far_triples(frame):
        near[ks[0]] = n <= 4 * 64
    return np.all(pts < 255, axis=1) & ~near


def _far_jobs(group, pts_of=far_points, frames=None):
    out = []
    for psz in GROUP_FORM_PSZ[group]:
        for frame in frames or FAR:
            pts = pts_of(frame)
            big = max(frame_size(frame)) == 576
            for l in range(1 if big else 0, LV + 1):
                out.append(Job(f"g{group}-far-step-{frame}-p{psz}-l{l}", "step", frame, psz, psz, l, l, 1, pts, group))
            for lv_f, lv_l in FAR_RANGES[1 if big else 0:]:
                out.append(Job(f"g{group}-far-full-{frame}-p{psz}-{lv_f}{lv_l}", "full", frame, psz, psz, lv_f, lv_l,
                               FAR_MAXITER, pts, group))
    return out


@functools.lru_cache(maxsize=None)
def far_jobs(group):
    """The far frames' own short list: per launch form of the group one patch size, 'step' at each level and 'full'
    over FAR_RANGES (on the 576 frame levels 1, 2 and the ranges (1,1), (2,0))."""
    return OrderedDict((j.key, j) for j in _far_jobs(group))


def truth_error(job, new):
    """|new - pts - (s, t)| per point, level-0 px (NaN where new is)."""
    d = new.astype(np.float64) - job.pts.astype(np.float64) - far_shift(job.frame)
    return np.hypot(d[:, 0], d[:, 1])


def check_truth(job, new, status):
    """A full far job: every point is kept and is within the patch size's bar of the known shift. Returns the worst
    error."""
    assert status.all(), (job.key, "lost", np.nonzero(~status)[0].tolist())
    err = truth_error(job, new)
    bad = np.nonzero(~(err <= TRUTH_BAR[job.psz]))[0]
    assert bad.size == 0, (job.key, "truth: |new - pts - shift| above", TRUTH_BAR[job.psz], "at",
                           [(job.pts[k].tolist(), round(float(err[k]), 4)) for k in bad])
    return float(err.max())


def discontinuous(job, new, status, iters, O):
    """[(n, largest difference of the displacements inside the triple, iters)] of the triples that break the rule of
    check_continuity, and the largest difference over all triples."""
    new_o, _, _, det = oracle_full(O, job)
    tol = full_tolerance(new_o, det)
    d = new.astype(np.float64) - job.pts.astype(np.float64)
    worst, bad = 0.0, []
    for n, ks in far_triples(job.frame):
        diff = float(np.abs(d[ks][:, None, :] - d[ks][None, :, :]).max()) if status[ks].all() else np.inf
        worst = max(worst, diff)
        if not diff <= 4 * tol[ks].max() or len(set(iters[ks].tolist())) != 1:
            bad.append((n, round(diff, 6), iters[ks].tolist()))
    return bad, worst


def check_continuity(job, new, status, iters, O):
    """A full far job: the three points of a triple are one ulp apart and the sampling is continuous across an integer,
    so their displacements differ by no more than 4 x the job's tolerance, and status and iters are equal. Returns the
    largest difference."""
    bad, worst = discontinuous(job, new, status, iters, O)
    assert not bad, (job.key, "continuity: (n, largest difference inside the triple, iters)", bad)
    return worst


# ---------------------------------------------------------------- the flow grid on a far pair
GRID_STEP, GRID_PSZ, GRID_LV = 4, 15, 2     # FlowGrid(w, h, 4).compute(..., psz=15, lv_f=2) with its default maxiter, eps
GRID_INSIDE = GRID_PSZ - 1                  # interior node: this far from every border (its level-0 patch, moved by the
#                                             shift, lies in the frame)


def grid_nodes(frame):
    """(ny, nx, 2) f64 node coordinates of the step grid and the interior mask (ny, nx)."""
    w, h = frame_size(frame)
    gx, gy = np.meshgrid(np.arange(GRID_STEP // 2, w, GRID_STEP), np.arange(GRID_STEP // 2, h, GRID_STEP))
    xy = np.stack([gx, gy], -1).astype(np.float64)
    inside = ((xy[..., 0] >= GRID_INSIDE) & (xy[..., 0] <= w - GRID_INSIDE)
              & (xy[..., 1] >= GRID_INSIDE) & (xy[..., 1] <= h - GRID_INSIDE))
    return xy, inside


def check_grid(frame, field, lost, bar):
    """The dense field (h, w, 2) of a flow grid on a far pair, read at the node pixels (so after the fill), and the
    grid's lost mask: no interior node is lost, every interior node is within the bar of the known shift, and the
    median error over the interior nodes with a coordinate >= 256 is not above twice the median over the others.
    Returns (largest error, median below 256, median from 256 on)."""
    xy, inside = grid_nodes(frame)
    h2 = GRID_STEP // 2
    d = field[h2::GRID_STEP, h2::GRID_STEP].astype(np.float64) - far_shift(frame)
    assert d.shape == xy.shape and lost.shape == inside.shape
    assert not lost[inside].any(), (frame, "interior nodes lost", np.argwhere(lost & inside).tolist())
    err = np.hypot(d[..., 0], d[..., 1])
    far = inside & (xy.max(axis=-1) >= 256)
    near = inside & ~far
    assert far.sum() >= 100 and near.sum() >= 100
    bad = inside & ~(err <= bar)
    assert not bad.any(), (frame, "nodes above", bar, [(xy[i, j].tolist(), round(float(err[i, j]), 4))
                                                       for i, j in np.argwhere(bad)[:12]], int(bad.sum()))
    med_near, med_far = float(np.median(err[near])), float(np.median(err[far]))
    assert med_far <= 2 * med_near, (frame, "median error from 256 on", med_far, "below", med_near)
    return float(err[inside].max()), med_near, med_far
