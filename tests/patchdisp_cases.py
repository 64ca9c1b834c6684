"""Cases, oracle records and tolerances for the 1-D patch search k_patchdisp (csrc/ictr_patchflow.hip), shared by
test_patchdisp_cpu.py and test_gpu_patchdisp.py.

A *job* is one launch of k_patchdisp: a frame pair, a patch size, a pyramid padding, a level range, an iteration cap and
a point array. The launcher chooses the form by the patch size alone, so there is one group. The oracle is
tests/patchdisp_np.py (f64 sums over the f32 patch values) on the planes of oracle.Pyramid, which are bit-equal to the
device's. The frames, the special, leaving and textureless point sets are patchflow_cases'; "cols-WxH" is new: A = B with
the same columns all equal to one profile (horizontal edges alone: no x gradient, no disparity).

Tolerances (nothing here is fitted to the device):
  one step   (new_x - x) / 2^l against one_step's derived bound (patchdisp_np's docstring) plus u |new_x| / 2^l
  full run   FULL_MARGIN * FULL_FACTOR * (sum of the one-step bounds of the oracle's steps, each * 2^l, + u |new_x|).
             FULL_FACTOR is the worst ratio of the f32 restatement (patchdisp_f32.py) against the f64 oracle over the
             table, measured on the CPU by test_patchdisp_cpu.py, which fails if it is exceeded; FULL_MARGIN = 4 as in
             the 2-D tests, because the device adds in another order than the restatement.
  decisions  status and iters are demanded exactly. The interior points are chosen so that every decision of the oracle
             (in view along x, conditioning, convergence) is further from its threshold than the run's tolerance.

The far jobs (far_jobs) run patchflow_cases' x-shift far frame and points through the three forms: x of 256 and more with
a displacement known in advance (check_truth, check_continuity, and patchflow_cases.check_grid for compute_x).
"""
from __future__ import annotations

import functools
from collections import OrderedDict, namedtuple

import numpy as np

import patchdisp_np as DN
import patchflow_cases as PC
from oracle import np_patchflow as NP

LV = PC.LV
U = PC.U
EPS, MAXITER = PC.EPS, PC.MAXITER       # full runs: 0.005, 8
MIN_HX = DN.MIN_HX
FULL_FACTOR = 0.14                      # measured on the CPU: 0.1364 (form 41); test_patchdisp_cpu.py re-checks it
FULL_MARGIN = 4.0
# hxx / tr of an f32 evaluation differs from the oracle's by less than 2 (L + c) u < 3e-6 (L + c <= 24; hxx <= tr), and
# f32(1e-2) from 1e-2 by 3e-10: a decision 1e-5 away from min_hx cannot flip
HX_MARGIN = 1e-5

PSZ = (1, 8, 9, 15, 16, 17, 31, 32)
FORM = {1: 11, 8: 11, 9: 41, 15: 41, 16: 41, 17: 82, 31: 82, 32: 82}      # psz -> NPL * 10 + WPP
RANGES = PC.RANGES                      # (0,0) (1,1) (2,2) (2,1) (2,0)
KS = PC.KS                              # 1 2 3 4 5 9
FORM_PSZ = (8, 15, 31)                  # one per form: the K, padding and independence jobs
PAD_EXTRA = PC.PAD_EXTRA                # 0 1 5
ROLL = PC.ROLL
N_INTERIOR = 10

Job = namedtuple("Job", "key kind frame psz pad lv_f lv_l maxiter pts")


@functools.lru_cache(maxsize=None)
def pair(frame):
    """patchflow_cases.pair, and 'cols-WxH': A = B with columns 8..w-8 all equal to column 8."""
    kind, _, size = frame.rpartition("-")
    if kind != "cols":
        return PC.pair(frame)
    w, h = PC.SIZES[size]
    a = PC.pair(size)[0].copy()
    a[:, 8:w - 8] = a[:, 8:9]
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(a.copy(), np.float32)


_pyr = {}


def oracle_pyramids(O, frame, pad):
    key = (frame, pad)
    if key not in _pyr:
        a, b = pair(frame)
        _pyr[key] = (O.Pyramid(a, LV, pad), O.Pyramid(b, LV, pad))
    return _pyr[key]


# ---------------------------------------------------------------- point sets
# Points at least 8 px inside the frame (one on half pixels, one on an integer row). They are the first ten, among the 2-D
# tests' interior points followed by candidates(), for which every decision of the oracle has its margin (margins_ok) at
# every patch size, form and level range of the table, and on the rolled pair at psz 15: chosen on the oracle alone, and
# checked again by test_patchdisp_cpu.py.
INTERIOR = {
    "100x77": [[23.72, 33.92], [38.75, 56.88], [75.06, 10.39], [66.63, 46.17], [13.08, 19.27], [46.81, 30.57],
               [81.04, 48.49], [32.94, 17.8], [53.21, 32.54], [17.35, 60.73]],
    "67x53": [[44.5, 44.5], [35.73, 21.52], [50.91, 19.35], [24.91, 30.71], [33.7, 42.0], [58.18, 35.41],
              [48.71, 35.23], [56.93, 34.3], [46.95, 14.49], [53.19, 29.07]],
}


def candidates(frame, n=120):
    """Uniform draws at least 8 px inside the frame, two decimals."""
    w, h = PC.frame_size(frame)
    rng = np.random.default_rng(PC.SYNTH_SEED[frame] + 100)
    xy = np.stack([rng.uniform(8, w - 8, n), rng.uniform(8, h - 8, n)], 1)
    return np.round(xy, 2).astype(np.float32)


def interior(frame):
    return np.array(INTERIOR[frame.split("-")[-1]], np.float32)


special, leaving, textureless, nan_interleaved = PC.special, PC.leaving, PC.textureless, PC.nan_interleaved


# ---------------------------------------------------------------- the job table
def _jobs(ipts_of=interior):
    out = []

    def add(key, kind, frame, psz, lv_f, lv_l, maxiter, pts, extra=0):
        out.append(Job(key, kind, frame, psz, psz + extra, lv_f, lv_l, maxiter, np.ascontiguousarray(pts, np.float32)))

    for psz in PSZ:
        for frame in PC.SIZES:
            pts = np.concatenate([ipts_of(frame), special(frame)])
            for l in range(LV + 1):
                add(f"step-{frame}-p{psz}-l{l}", "step", frame, psz, l, l, 1, pts)
            for lv_f, lv_l in RANGES:
                add(f"full-{frame}-p{psz}-{lv_f}{lv_l}", "full", frame, psz, lv_f, lv_l, MAXITER, pts)
        add(f"leave-p{psz}-20", "full", "roll-100x77", psz, 2, 0, MAXITER, leaving("100x77"))
        add(f"leave-p{psz}-11", "full", "roll-100x77", psz, 1, 1, MAXITER, leaving("100x77"))
        for frame in ("flat-100x77", "cols-100x77"):
            add(f"{frame}-p{psz}-00", "lost", frame, psz, 0, 0, MAXITER, textureless("100x77"))
            if psz <= 17:  # the level-1 region holds the patch and the gradient's support
                add(f"{frame}-p{psz}-11", "lost", frame, psz, 1, 1, MAXITER, textureless("100x77"))
        for lv_f, lv_l in ((0, 0), (2, 0), (2, 1)):
            add(f"rows-p{psz}-{lv_f}{lv_l}", "rows", "rows-100x77", psz, lv_f, lv_l, MAXITER, ipts_of("100x77"))
        add(f"maxiter0-p{psz}", "maxiter0", "100x77", psz, 2, 0, 0, np.concatenate([ipts_of("100x77"), special("100x77")]))
    add("roll-p15-20", "full", "roll-100x77", 15, 2, 0, MAXITER, ipts_of("100x77"))
    for psz in FORM_PSZ:
        ipts = ipts_of("100x77")
        for K in KS:
            add(f"K{K}-p{psz}", "full", "100x77", psz, 2, 0, MAXITER, ipts[:K])
        for extra in PAD_EXTRA:
            add(f"pad{extra}-p{psz}", "pad", "100x77", psz, 2, 0, MAXITER, ipts, extra)
        add(f"indep-perm-p{psz}", "indep", "100x77", psz, 2, 0, MAXITER, ipts[perm_of(psz)])
        add(f"indep-nan-p{psz}", "indep", "100x77", psz, 2, 0, MAXITER, nan_interleaved(ipts))
        for k in range(len(ipts)):
            add(f"indep-one{k}-p{psz}", "indep", "100x77", psz, 2, 0, MAXITER, ipts[k:k + 1])
    return out


@functools.lru_cache(maxsize=None)
def jobs():
    return OrderedDict((j.key, j) for j in _jobs())


# ---------------------------------------------------------------- the far jobs: coordinates of 256 and more
FAR_FRAME = "farx-320x64"               # patchflow_cases' analytic pair with B = A shifted by 1.7 px along x
# |new_x - x - 1.7| px of a full run at every point, per patch size: twice the f64 oracle's worst error over the far
# jobs' points with x < 255 (patchflow_cases.far_low). Measured on the CPU by test_patchdisp_cpu.py, which fails if a
# bar is exceeded there or is above 0.25 px.
TRUTH_BAR = {8: 0.069, 15: 0.055, 31: 0.053}             # 2 x (0.0342, 0.0273, 0.0264), rounded up


def _far_jobs(pts_of=PC.far_points):
    out = []
    pts = pts_of(FAR_FRAME)
    for psz in FORM_PSZ:
        for l in range(LV + 1):
            out.append(Job(f"far-step-p{psz}-l{l}", "step", FAR_FRAME, psz, psz, l, l, 1, pts))
        for lv_f, lv_l in PC.FAR_RANGES:
            out.append(Job(f"far-full-p{psz}-{lv_f}{lv_l}", "full", FAR_FRAME, psz, psz, lv_f, lv_l, PC.FAR_MAXITER, pts))
    return out


@functools.lru_cache(maxsize=None)
def far_jobs():
    """patchflow_cases' far frame and points for the three forms: 'step' at each level and 'full' over FAR_RANGES."""
    return OrderedDict((j.key, j) for j in _far_jobs())


def perm_of(psz):
    return np.random.default_rng(psz).permutation(N_INTERIOR)


def form(job):
    return FORM[job.psz]


def form_shape(job):
    """(L, WPP): the most pixels a lane adds in the job's form, and its waves per patch."""
    wpp = form(job) % 10
    return NP.lane_pixels(job.psz, wpp), wpp


# ---------------------------------------------------------------- oracle records
_rec = {}


def oracle_full(O, job):
    """(new, status, iters, detail) of the oracle for a job, with the bound summed for the job's form."""
    if job.key not in _rec:
        pa, pb = oracle_pyramids(O, job.frame, job.pad)
        L, wpp = form_shape(job)
        _rec[job.key] = DN.track_disparity(pa, pb, job.pts, job.psz, job.lv_f, job.lv_l, job.maxiter, EPS, MIN_HX,
                                           detail=True, nsum=L + 7 + (wpp - 1))
    return _rec[job.key]


_step = {}


def oracle_step(O, job):
    """(step, bound, hxx / tr) of one_step for a 'step' job."""
    if job.key not in _step:
        pa, pb = oracle_pyramids(O, job.frame, job.pad)
        L, wpp = form_shape(job)
        _step[job.key] = DN.one_step(pa, pb, job.pts, job.psz, job.lv_f, L, wpp, MIN_HX)
    return _step[job.key]


def base_tolerance(new_o, detail):
    """bound sum + u |new_x| per point, level-0 pixels: the quantity FULL_FACTOR scales."""
    return detail["bound"] + U * np.nan_to_num(np.abs(new_o[:, 0]).astype(np.float64))


def full_tolerance(new_o, detail):
    return FULL_MARGIN * FULL_FACTOR * base_tolerance(new_o, detail)


def out_ulp(new_o):
    """Per point: the spacing of f32 at the returned x, 0 for a lost point."""
    with np.errstate(invalid="ignore"):
        return np.nan_to_num(np.spacing(np.abs(new_o[:, 0])).astype(np.float64))


def margins_ok(new_o, detail, far=False):
    """Per point: every decision the oracle took is further from its threshold than an f32 evaluation can move it (far:
    one spacing of f32 at the position included, see patchflow_cases.compare_full)."""
    tol = full_tolerance(new_o, detail) + (out_ulp(new_o) if far else 0.0)  # positions at level l move by tol / 2^l <= tol
    return (detail["view"] > tol) & (detail["eps_px"] > tol) & (detail["hx"] > HX_MARGIN)


def check_margins(job, new_o, detail):
    tol = full_tolerance(new_o, detail) + (out_ulp(new_o) if PC.is_far(job) else 0.0)
    assert np.all(detail["view"] > tol), (job.key, "pick other points: in-view margin", detail["view"], tol)
    assert np.all(detail["eps_px"] > tol), (job.key, "pick other points: convergence margin", detail["eps_px"], tol)
    assert np.all(detail["hx"] > HX_MARGIN), (job.key, "pick other points: conditioning margin", detail["hx"])


def _ybits_ok(job, new, status):
    y_in = np.ascontiguousarray(job.pts[:, 1]).view(np.uint32)
    y_out = np.ascontiguousarray(new[:, 1]).view(np.uint32)
    assert np.array_equal(y_out[status], y_in[status]), (job.key, "y does not have the input's bits")


def compare_step(job, new, status, iters, O):
    """One-step check of a device (or restatement) result; returns the worst ratio against the bound."""
    step, bound, _ = oracle_step(O, job)
    live = np.isfinite(step)
    assert np.array_equal(status, live), (job.key, status, live)
    assert np.all(iters[live] == 1) and np.all(iters[~live] == 0), (job.key, iters)
    assert np.isnan(new[~live]).all(), job.key
    _ybits_ok(job, new, live)
    s = 2.0 ** job.lv_f
    got = (new[live, 0].astype(np.float64) - job.pts[live, 0].astype(np.float64)) / s
    ratio = np.abs(got - step[live]) / (bound[live] + U * np.abs(new[live, 0].astype(np.float64)) / s)
    assert np.all(ratio <= 1.0), (job.key, "worst ratio", float(ratio.max()), "at", np.argwhere(ratio > 1.0).tolist())
    return float(ratio.max()) if ratio.size else 0.0


def compare_full(job, new, status, iters, O):
    """Full-run check: status and iters exactly, x within full_tolerance, y with the input's bits, lost points NaN;
    returns the worst ratio of the x error against bound sum + u |new_x|. On the far frame one spacing of f32 at the
    returned x is taken off the error first, as in patchflow_cases.compare_full and for its reason."""
    new_o, ok_o, it_o, det = oracle_full(O, job)
    check_margins(job, new_o, det)
    assert np.array_equal(status, ok_o), (job.key, status, ok_o)
    assert np.array_equal(iters, it_o), (job.key, iters, it_o)
    assert np.isnan(new[~ok_o]).all(), job.key
    _ybits_ok(job, new, ok_o)
    if not ok_o.any():
        return 0.0
    err = np.abs(new[ok_o, 0].astype(np.float64) - new_o[ok_o, 0].astype(np.float64))
    if PC.is_far(job):
        err = np.maximum(err - out_ulp(new_o)[ok_o], 0.0)
    base = base_tolerance(new_o, det)[ok_o]
    assert np.all(err <= FULL_MARGIN * FULL_FACTOR * base), (job.key, "worst error / tolerance",
                                                            float((err / (FULL_MARGIN * FULL_FACTOR * base)).max()))
    return float((err / base).max())


# ---------------------------------------------------------------- the usefulness scene
SCENE_W, SCENE_H, SCENE_SHIFT = 160, 96, 3.3
SCENE_TILTS, SCENE_SEEDS = (20, 45), (1, 2, 3)
SCENE_PSZ, SCENE_LV = 15, 2
BAR_1D, BAR_2D = 0.05, 0.3              # median |x error| px: the 1-D search at most, the 2-D tracker at least


@functools.lru_cache(maxsize=None)
def scene(tilt, seed):
    """(A, B) float32, 160x96: 12 gratings within +-2.5 degrees of `tilt`, B shifted by 3.3 px along x (the truth of
    A -> B is -3.3 px), sigma = 2 grey levels of noise on each."""
    rng = np.random.default_rng(seed)
    rs = rng.random((12, 2)) - [0.5, 0]
    amp = 8 + 8 * rng.random(12)
    ph = 6.28 * rng.random(12)
    y, x = np.mgrid[0:SCENE_H, 0:SCENE_W].astype(np.float64)

    def img(xs):
        out = np.full((SCENE_H, SCENE_W), 128.0)
        for k in range(12):
            th = np.deg2rad(tilt + 5 * rs[k, 0])
            lam = 8 + 40 * rs[k, 1]
            out += amp[k] * np.sin(2 * np.pi * (np.cos(th) * xs + np.sin(th) * y) / lam + ph[k])
        return out

    a = img(x) + 2 * rng.standard_normal((SCENE_H, SCENE_W))
    b = img(x + SCENE_SHIFT) + 2 * rng.standard_normal((SCENE_H, SCENE_W))
    return a.astype(np.float32), b.astype(np.float32)


def scene_nodes():
    gx, gy = np.meshgrid(np.arange(24, 129, 8), np.arange(20, 69, 8))
    return np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float32)


def scene_errors(new, ok):
    """(kept, median |x error|, max |x error|) against the truth -3.3 px."""
    e = np.abs((new[ok, 0].astype(np.float64) - scene_nodes()[ok, 0]) + SCENE_SHIFT)
    return int(ok.sum()), float(np.median(e)) if e.size else np.inf, float(e.max()) if e.size else np.inf


# ---------------------------------------------------------------- the far jobs' checks
def truth_error(job, new):
    """|new_x - x - s| per point, level-0 px (NaN where new is)."""
    return np.abs(new[:, 0].astype(np.float64) - job.pts[:, 0].astype(np.float64) - PC.far_shift(job.frame)[0])


def check_truth(job, new, status):
    """A full far job: every point is kept and is within the patch size's bar of the known shift."""
    assert status.all(), (job.key, "lost", np.nonzero(~status)[0].tolist())
    err = truth_error(job, new)
    bad = np.nonzero(~(err <= TRUTH_BAR[job.psz]))[0]
    assert bad.size == 0, (job.key, "truth: |new_x - x - shift| above", TRUTH_BAR[job.psz], "at",
                           [(job.pts[k].tolist(), round(float(err[k]), 4)) for k in bad])
    return float(err.max())


def discontinuous(job, new, status, iters, O):
    """[(n, largest difference of the x displacements inside the triple, iters)] of the triples that break the rule of
    check_continuity, and the largest difference over all triples."""
    new_o, _, _, det = oracle_full(O, job)
    tol = full_tolerance(new_o, det)
    d = new[:, 0].astype(np.float64) - job.pts[:, 0].astype(np.float64)
    worst, bad = 0.0, []
    for n, ks in PC.far_triples(job.frame):
        diff = float(d[ks].max() - d[ks].min()) if status[ks].all() else np.inf
        worst = max(worst, diff)
        if not diff <= 4 * tol[ks].max() or len(set(iters[ks].tolist())) != 1:
            bad.append((n, round(diff, 6), iters[ks].tolist()))
    return bad, worst


def check_continuity(job, new, status, iters, O):
    """A full far job: inside a triple (three x one ulp apart) the displacements differ by no more than 4 x the job's
    tolerance, and status and iters are equal. Returns the largest difference."""
    bad, worst = discontinuous(job, new, status, iters, O)
    assert not bad, (job.key, "continuity: (n, largest difference inside the triple, iters)", bad)
    return worst
