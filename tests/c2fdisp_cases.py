"""Cases, recorded differences and usefulness figures for the 1-D (x only) form of the coarse-to-fine dense flow
(CoarseToFineFlow(x_only=True): the XONLY forms of k_c2f_level, the refinement along x), shared by test_c2fdisp_cpu.py and
test_gpu_c2fdisp.py.

The definition is patchflow.c2f_flow_host(..., x_only=True) (f64). c2fdisp_f32.py restates the kernels in f32; the GPU
tests demand its bits of the device, per level (d, status, bias, field) and of the final field. The CPU module compares the
restatement with the definition level by level from the SAME starts on the nodes where every decision of the definition
has its margin (c2fflow_cases.MARGIN_EPS, MARGIN_PX; the conditioning decision patchdisp_cases.HX_MARGIN); the worst
differences are RECORDED here and measured again by test_c2fdisp_cpu.py, which fails above a record or below half of it.
Nothing here is fitted to the device.

Every entry runs twice: plain on c2fflow_cases.pair's frames, and with patnorm on (A, B + 20).
"""
from __future__ import annotations

import functools

import numpy as np

import c2fflow_cases as CC
import patchdisp_cases as DC
import patnorm_cases as PN

PAD_EXTRA = CC.PAD_EXTRA
REFINE = CC.REFINE
HX_MARGIN = DC.HX_MARGIN
STRIPES = "stripes-48x32"
# c2fflow_cases' table and its status pair in the other two forms, then vertical stripes: Gy ~ 0, so hxy ~ 0 and det ~ 0; the
# 2-D conditioning test refuses every such node and the 1-D test keeps it (the only content that tells the two apart).
TABLE = CC.TABLE + CC.STATUS_FORMS + ((STRIPES, 8, 1, 10, 0.01, None, 4),)
STRIPE_CASE = TABLE[-1]
STATUS_CASES = tuple(c for c in TABLE if c[0] == "status-96x64")
MODES = (False, True)   # patnorm


def pad_of(case):
    return case[1] + PAD_EXTRA[TABLE.index(case) % 3]


def refine_of(case):
    return REFINE if case[5] else None


@functools.lru_cache(maxsize=None)
def stripes(w=48, h=32, seed=5):
    """Vertical stripes of two periods, B shifted by 1.7 px along x, sigma = 0.02 grey levels of noise on each."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)

    def img(xs):
        return 128 + 40 * np.sin(2 * np.pi * xs / 11.0) + 25 * np.sin(2 * np.pi * xs / 23.0 + 1.0)

    a = img(x) + 0.02 * rng.standard_normal((h, w))
    b = img(x + 1.7) + 0.02 * rng.standard_normal((h, w))
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)


def frame_size(frame):
    return (48, 32) if frame == STRIPES else CC.frame_size(frame)


def pair(frame, patnorm=False):
    """(A, B) of a frame; the patnorm run reads B + 20."""
    a, b = stripes() if frame == STRIPES else CC.pair(frame)
    return a, PN.changed(b, "+20" if patnorm else "none")


_pyr = {}


def pyramids_of(case, patnorm):
    """(oracle.Pyramid A, B) of a table entry; shared, do not write to them. Needs the built oracle."""
    from oracle import oracle as O
    key = (case[0], bool(patnorm), pad_of(case), case[2])
    if key not in _pyr:
        a, b = pair(case[0], patnorm)
        _pyr[key] = (O.Pyramid(a, case[2], pad_of(case)), O.Pyramid(b, case[2], pad_of(case)))
    return _pyr[key]


@functools.lru_cache(maxsize=None)
def host_run(case, patnorm, x_only=True):
    """(field, stages) of the definition on a table entry."""
    from invcompcamtrack_amd import patchflow as pf
    frame, psz, lv_f, maxiter, eps, _, step = case
    st = []
    out = pf.c2f_flow_host(*pyramids_of(case, patnorm), step, psz, lv_f, maxiter, eps, refine=refine_of(case), _stages=st,
                           patnorm=patnorm, x_only=x_only)
    return out, st


@functools.lru_cache(maxsize=None)
def restated(case, patnorm, defect=None):
    """(field, [(level, field, d, status, bias)]) of the f32 restatement on a table entry."""
    import c2fdisp_f32 as R
    frame, psz, lv_f, maxiter, eps, _, step = case
    st = []
    out = R.run(*pyramids_of(case, patnorm), step, psz, lv_f, maxiter, eps, refine=refine_of(case), patnorm=patnorm,
                defect=defect, stages=st)
    return out, st


def compared(stage, eps):
    """(ny, nx) bool: the nodes of a definition's level whose decisions all have their margins."""
    m = stage["margins"]
    ok = (m["view"] >= CC.MARGIN_PX) & (m["far"] >= CC.MARGIN_PX) & (m["det"] >= HX_MARGIN)
    if eps > 0:  # (with eps = 0 no stop decision exists)
        ok &= m["eps"] >= CC.MARGIN_EPS
    return ok


def level_differences(case, patnorm, defect=None):
    """Per level of a table entry, the restatement's search (and bias) from the definition's own starts against the
    definition: [(level, nodes, left out, statuses equal on the compared nodes, worst |d - definition|, worst |beta -
    definition| (0 without patnorm), on them)]."""
    import c2fdisp_f32 as R
    frame, psz, lv_f, maxiter, eps, _, step = case
    pa, pb = pyramids_of(case, patnorm)
    out = []
    for s in host_run(case, patnorm)[1]:
        keep = compared(s, eps)
        d, lost, status, bias = R.search(pa, pb, s["level"], s["init"], step, psz, maxiter, eps, patnorm, defect)
        same = bool(np.array_equal(status[keep], s["status"][keep]))
        votes = keep & (s["status"] != 0) & ~lost
        diff = float(np.abs(d.astype(np.float64) - s["d"])[votes].max()) if votes.any() else 0.0
        bdiff = float(np.abs(bias.astype(np.float64) - s["bias"])[keep].max()) if patnorm and keep.any() else 0.0
        out.append((s["level"], keep.size, int((~keep).sum()), same, diff, bdiff))
    return out


# level -> worst |restatement - definition| over TABLE on the compared nodes, from the same starts, of d in px (plain and
# patnorm runs together) and of beta in grey levels (patnorm runs); measured by test_c2fdisp_cpu.py.
# Level 0 is set by the status pair, whose runaway nodes move by several px per step over a ramp of 2.5 grey levels per
# px (d: plain psz 8; beta: patnorm psz 8); without it the table stays below 9.0e-5 px and 1.5e-4.
D_DIFF = {0: 1.3e-3, 1: 3.1e-5, 2: 3.0e-6}
BIAS_DIFF = {0: 1.1e-3, 1: 6.1e-4, 2: 6.7e-5}
# worst |restatement - definition| of the final field in px over the entries with eps = 0 (whole runs, plain and patnorm)
FIELD_DIFF = 4.5e-5
# the worst share of nodes left out at a level of 20 nodes or more (cap: c2fflow_cases.LEFT_OUT_CAP), with its entry
# (frame, psz, lv_f, step, level, patnorm)
LEFT_OUT = (0.0834, ("67x53", 8, 1, 4, 1, True))   # 4 of 48 nodes; the stripes leave out as many of level 0 (8 of 96,
# plain; the table's order decides the tie), 320x64 at psz 8 6 of 80 at level 2 (plain); most levels are at 0 - 4 %
# status counts 0 .. 4 over the three levels of the restatement's run on the status pair, per (psz, patnorm)
STATUS_COUNTS = {(8, False): (40, 386, 72, 0, 6), (8, True): (40, 392, 72, 0, 0),
                 (15, False): (16, 420, 44, 24, 0), (15, True): (16, 420, 44, 24, 0),
                 (17, False): (16, 421, 43, 24, 0), (17, True): (16, 418, 43, 27, 0)}
# Over the whole table every form holds the statuses 0 - 3, plain and with patnorm: <4,1> and <8,2> on the status pair
# above, <1,1> with status 3 from 100x77 (plain: 5 nodes), 64x320 (patnorm: 3) and the stripes (patnorm: 8). Status 4 in
# form <1,1>: plain 100x77 (10), 67x53 (2), 64x320 (5) and the status pair (6); patnorm 100x77 (2) and 64x320 (1).

# ---------------------------------------------------------------- usefulness, on the host definition alone
USEFUL_PSZ, USEFUL_LV, STEP = (8, 15), 2, 4


@functools.lru_cache(maxsize=None)
def useful_field(tilt, seed, psz, x_only, patnorm=False, offset=False):
    """c2f_flow_host's field on patchdisp_cases.scene (right frame + 20 with `offset`), pad = psz."""
    from invcompcamtrack_amd import patchflow as pf
    from oracle import oracle as O
    a, b = DC.scene(tilt, seed)
    b = PN.changed(b, "+20" if offset else "none")
    pa, pb = O.Pyramid(a, USEFUL_LV, psz), O.Pyramid(b, USEFUL_LV, psz)
    return pf.c2f_flow_host(pa, pb, STEP, psz, USEFUL_LV, patnorm=patnorm, x_only=x_only)


def useful_error(tilt, seed, psz, x_only, patnorm=False, offset=False):
    """(mean, median) |x error| in px of that field against the truth -3.3 px, 16 px inside the frame."""
    e = np.abs(useful_field(tilt, seed, psz, x_only, patnorm, offset)[16:-16, 16:-16, 0].astype(np.float64)
               + DC.SCENE_SHIFT)
    return float(e.mean()), float(np.median(e))


# the definition's worst 1-D / 2-D ratio of the mean |x error| over tilts 20 / 45, seeds 1 - 3, psz 8 / 15, with its scene
# (tilt, psz, seed); the bar is the project's form, the worst ratio plus a quarter of its gain. Measured by
# test_c2fdisp_cpu.py, which also holds every 1-D median to patchdisp_cases.BAR_1D.
# Mean |x error| in px, seeds 1 / 2 / 3, 2-D (y dropped) -> 1-D:
#   20 deg, psz 8    0.7833 / 1.0974 / 1.4163 -> 0.0291 / 0.0217 / 0.0273
#   20 deg, psz 15   0.6321 / 0.5214 / 0.4148 -> 0.0127 / 0.0089 / 0.0105
#   45 deg, psz 8    2.8072 / 1.4975 / 3.3484 -> 0.0389 / 0.0283 / 0.0428
#   45 deg, psz 15   1.0063 / 0.9444 / 1.1809 -> 0.0152 / 0.0105 / 0.0196
# Recorded without a bar, the 1-D form on (A, B + 20), plain -> patnorm:
#   20 deg, psz 8    2.1867 / 1.3652 / 2.0789 -> 0.0334 / 0.0238 / 0.0350
#   20 deg, psz 15   0.9067 / 0.8326 / 1.0069 -> 0.0133 / 0.0095 / 0.0107
#   45 deg, psz 8    2.4426 / 2.0066 / 2.4357 -> 0.0411 / 0.0311 / 0.0534
#   45 deg, psz 15   1.2466 / 1.2204 / 1.4550 -> 0.0165 / 0.0116 / 0.0204
USEFUL_RATIO = (0.0373, (20, 8, 1))
USEFUL_MEDIAN = 0.0314   # the worst 1-D median |x error| in px (45 deg, psz 8, seed 1)


def useful_bar():
    return USEFUL_RATIO[0] + (1.0 - USEFUL_RATIO[0]) / 4
