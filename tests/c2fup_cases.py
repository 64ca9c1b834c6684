"""Shapes, fields, recorded differences and usefulness figures for a finest level above 0 of the coarse-to-fine dense flow
(CoarseToFineFlow(lv_l=...), k_flow_upsample), shared by test_c2fup_cpu.py and test_gpu_c2fup.py.

The definition is patchflow.upsample_flow_host (f64 on the f32 taps, rounded once) and patchflow.c2f_flow_host(lv_l=...).
c2fup_f32.py restates the kernel in f32; the GPU tests demand its bits of the device. The CPU module holds the restatement
to the definition within a derived bound and RECORDS the worst measured difference, which it measures again and fails above
the record or below half of it. Nothing here is fitted to the device.
"""
from __future__ import annotations

import functools

import numpy as np

import c2fflow_cases as CC
import flowrefine_cases as FC

# (w, h, lv): 5x3 -> 2x2; 3x2 -> 2x1 (both y taps clamped to row 0); 9x7 -> 4x4 (8 < 9 and 8 > 7); 67x53 -> 34x26 and
# 17x13 (over in x, under in y); 100x77; 320x64 and 64x320 (many workgroups along one axis); 1242x375 once.
SHAPES = ((5, 3, 1), (3, 2, 1), (9, 7, 1), (67, 53, 1), (67, 53, 2), (100, 77, 1), (320, 64, 1), (64, 320, 1),
          (1242, 375, 1))
M = 8.0   # the random fields' taps lie in [-M, M]


def level_size(w, h, lv):
    from invcompcamtrack_amd import patchflow as pf
    return pf.pyramid_level_size(w, h, lv)


@functools.lru_cache(maxsize=None)
def field(w, h, lv, seed=0):
    """A seeded random field (h_l, w_l, 2) f32 of level lv of a w x h pyramid, uniform in [-M, M]; do not write to it."""
    wl, hl = level_size(w, h, lv)
    rng = np.random.default_rng(1000 * seed + 31 * w + 7 * h + lv)
    f = rng.uniform(-M, M, (hl, wl, 2)).astype(np.float32)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def restated(w, h, lv, x_only, seed=0):
    """The f32 restatement's up-sampled field of `field`; shared, do not write to it."""
    import c2fup_f32 as R
    out = R.upsample(field(w, h, lv, seed), w, h, lv, x_only)
    out.setflags(write=False)
    return out


def bound(lv, m=M):
    """|restatement - definition| <= 6 u s M with u = 2^-24: a lerp of two rounded products and a rounded sum is within
    2 u of the exact convex combination (relative to the taps' bound M); the second lerp carries that through a convex
    combination and adds its own 2 u: 4 u; the product with s is exact; the definition's own final rounding adds u.
    5 u, rounded up to 6 u for the second-order terms."""
    return 6.0 * 2.0 ** -24 * (1 << lv) * m


# the worst |restatement - definition| / bound(lv) over SHAPES, x_only off and on, seeds 0 and 1; measured by
# test_c2fup_cpu.py, which fails above the record or below half of it
WORST_OVER_BOUND = 0.34   # 1 / 3: two units in the last place of a result between s M / 2 and s M

# ---------------------------------------------------------------- the stage: table entries run with lv_l
# (c2fflow_cases entry, lv_l, patnorm, x_only)
_E = {(c[0], c[5], c[6]): c for c in CC.TABLE if c[1] == 8 and c[2] == 2 and c[4] == 0.01}
STAGE_CASES = tuple((_E[k], lv_l, False, False) for k in (("67x53", None, 4), ("67x53", None, 3), ("100x77", "refine", 4))
                    for lv_l in (1, 2)) + ((_E["67x53", None, 4], 1, True, False), (_E["67x53", None, 4], 1, False, True))


def pair(case, patnorm):
    """(A, B) of a stage case's frames; the patnorm run reads B + 20 (patnorm_cases' change)."""
    a, b = CC.pair(case[0])
    return (a, np.ascontiguousarray(b + np.float32(20))) if patnorm else (a, b)


_pyr = {}


def host_pyramids(case, patnorm):
    """(oracle.Pyramid A, B) of a stage case; shared, do not write to them. Needs the built oracle."""
    from oracle import oracle as O
    key = (case[0], CC.pad_of(case), case[2], bool(patnorm))
    if key not in _pyr:
        _pyr[key] = tuple(O.Pyramid(im, case[2], CC.pad_of(case)) for im in pair(case, patnorm))
    return _pyr[key]


@functools.lru_cache(maxsize=None)
def restated_run(case, lv_l, patnorm, x_only):
    """(result (H, W, 2), stages of the levels lv_f .. lv_l) of the f32 restatement of a run with lv_l."""
    import c2fup_f32 as R
    frame, psz, lv_f, maxiter, eps, _, step = case
    st = []
    out = R.run(*host_pyramids(case, patnorm), step, psz, lv_f, lv_l, maxiter, eps, refine=CC.refine_of(case),
                patnorm=patnorm, x_only=x_only, stages=st)
    return out, st


# ---------------------------------------------------------------- usefulness, on the host definitions alone
KINDS = ("big", "layers", "rotzoom")
LV_LS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def useful_fields(kind, seed, refined=False):
    """{lv_l: c2f_flow_host's field at that finest level} on a usefulness scene of c2fflow_cases (psz 8, step 4, lv_f 3),
    from ONE run's stages (a level's field does not depend on finer levels; test_c2fup_cpu.py asserts that a run with
    lv_l returns these bits), and the scene's (img_a, img_b, truth, mask)."""
    from invcompcamtrack_amd import patchflow as pf
    from oracle import oracle as O
    a, b, truth, mask = CC.useful_inputs(kind, seed)
    h, w = a.shape
    pa, pb = O.Pyramid(a, CC.USEFUL_LV, CC.USEFUL_PSZ), O.Pyramid(b, CC.USEFUL_LV, CC.USEFUL_PSZ)
    st = []
    out = pf.c2f_flow_host(pa, pb, CC.STEP, CC.USEFUL_PSZ, CC.USEFUL_LV, refine=CC.USEFUL_REFINE if refined else None,
                           _stages=st)
    fields = {0: out}
    for s in st:
        if s["level"] in LV_LS[1:]:
            fields[s["level"]] = pf.upsample_flow_host(s["field"], w, h, s["level"])
    return fields, (a, b, truth, mask)


def useful_errors(kind, seed, refined=False):
    """(mean endpoint error in px at lv_l 0, 1, 2)."""
    fields, (_, _, truth, mask) = useful_fields(kind, seed, refined)
    return tuple(FC.epe(fields[k], truth, mask) for k in LV_LS)


@functools.lru_cache(maxsize=None)
def baseline_error(kind, seed):
    """The whole-pyramid grid, densified: c2fflow_cases.useful_errors' baseline."""
    return CC.useful_errors(kind, seed)[0]


# Mean endpoint errors in px over flowrefine_cases.SEEDS (0 / 1 / 2), measured by test_c2fup_cpu.py on the host functions:
#   scene     lv_l 0                  lv_l 1                  lv_l 2                  whole-pyramid grid, densified
#   big       1.027 / 2.212 / 1.497   1.351 / 2.604 / 1.600   2.911 / 3.864 / 2.297   2.162 / 3.972 / 2.129
#   layers    0.275 / 0.289 / 0.298   0.396 / 0.376 / 0.352   0.762 / 0.647 / 0.667   0.277 / 0.294 / 0.306
#   rotzoom   0.104 / 0.074 / 0.093   0.105 / 0.094 / 0.085   0.165 / 0.196 / 0.178   0.105 / 0.074 / 0.094
# With refine = c2fflow_cases.USEFUL_REFINE on every level:
#   big       1.041 / 2.244 / 1.360   1.333 / 2.419 / 1.293   2.404 / 3.346 / 1.792
#   layers    0.200 / 0.191 / 0.243   0.310 / 0.250 / 0.300   0.662 / 0.466 / 0.542
#   rotzoom   0.071 / 0.053 / 0.064   0.080 / 0.076 / 0.061   0.102 / 0.135 / 0.125
# refine_flow_host at level 0 (USEFUL_REFINE) on the up-sampled lv_l 1 field of the run without refinement, what
# FlowRefiner.run(src=c2f) gives, seed 0:  big 1.351 -> 1.105, layers 0.396 -> 0.272, rotzoom 0.105 -> 0.070
REFINED_AFTER = {"big": 1.105, "layers": 0.272, "rotzoom": 0.070}
RECORDED = {
    ("big", False): ((1.027, 2.212, 1.497), (1.351, 2.604, 1.600), (2.911, 3.864, 2.297)),
    ("layers", False): ((0.275, 0.289, 0.298), (0.396, 0.376, 0.352), (0.762, 0.647, 0.667)),
    ("rotzoom", False): ((0.104, 0.074, 0.093), (0.105, 0.094, 0.085), (0.165, 0.196, 0.178)),
    ("big", True): ((1.041, 2.244, 1.360), (1.333, 2.419, 1.293), (2.404, 3.346, 1.792)),
    ("layers", True): ((0.200, 0.191, 0.243), (0.310, 0.250, 0.300), (0.662, 0.466, 0.542)),
    ("rotzoom", True): ((0.071, 0.053, 0.064), (0.080, 0.076, 0.061), (0.102, 0.135, 0.125)),
}
RECORDED_TOL = 6e-4   # the records are rounded to three decimals
# "big": the worst seed's error at lv_l = 1 over the whole-pyramid baseline's (1.600 / 2.129, seed 2); the bar is
# c2fflow_cases.useful_bar's form, the worst ratio plus a quarter of its gain
USEFUL_LVL1 = 0.752


def useful_bar():
    return USEFUL_LVL1 + (1.0 - USEFUL_LVL1) / 4
