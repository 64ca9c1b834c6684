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


def frame_size(frame):
    return SIZES[frame.split("-")[-1]]


@functools.lru_cache(maxsize=None)
def pair(frame):
    """(img_a, img_b) f32. 'WxH': a synth.make_scene pair with a few pixels of motion. 'roll-WxH': B is A rolled by ROLL
    pixels along x. 'flat-WxH': A = B with a constant rectangle (rows 8..h-8, columns 8..w-8). 'rows-WxH': A = B with
    the same rows all equal to one profile."""
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


def check_margins(job, new_o, detail):
    """Every decision the oracle took is further from its threshold than an f32 evaluation can move it."""
    tol = full_tolerance(new_o, detail)
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
    bound-sum + u |new| (the quantity FULL_FACTOR scales)."""
    new_o, ok_o, it_o, det = oracle_full(O, job)
    check_margins(job, new_o, det)
    assert np.array_equal(status, ok_o), (job.key, status, ok_o)
    assert np.array_equal(iters, it_o), (job.key, iters, it_o)
    assert np.isnan(new[~ok_o]).all(), job.key
    if not ok_o.any():
        return 0.0
    err = np.abs(new[ok_o].astype(np.float64) - new_o[ok_o].astype(np.float64)).max(axis=1)
    tol = full_tolerance(new_o, det)[ok_o]
    assert np.all(err <= tol), (job.key, "worst error / tolerance", float((err / tol).max()))
    return float((err / tol).max() * FULL_MARGIN * FULL_FACTOR)
