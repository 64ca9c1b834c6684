"""Cases, recorded differences and usefulness figures for the patch-mean normalisation of the coarse-to-fine dense flow
(patnorm: the MEAN forms of k_c2f_level with their bias tail, k_densify<true, 1>), shared by test_patnorm_cpu.py and
test_gpu_patnorm.py.

The definition is patchflow.c2f_flow_host(..., patnorm=True) (f64). patnorm_f32.py restates the kernels in f32; the GPU
tests demand its bits of the device, per level (d, status, bias, field) and of the final field. The CPU module compares the
restatement with the definition level by level from the SAME starts on the nodes where every decision of the definition
has its margin (c2fflow_cases.MARGIN_*; the bias tail's view decision joins the "view" margin); the worst differences are
RECORDED here and measured again by test_patnorm_cpu.py, which fails above a record or below half of it. Nothing here is
fitted to the device.

The frames are c2fflow_cases.pair's with a change of brightness applied to frame B.
"""
from __future__ import annotations

import functools

import numpy as np

import c2fflow_cases as CC
import flowrefine_cases as FC

PAD_EXTRA = CC.PAD_EXTRA       # pyramids padded by psz + one of these, in rotation over the table
REFINE = CC.REFINE


def changed(b, change):
    """Frame B under a change of brightness: "+20", "ramp" (0.15 x + 0.05 y), "gain" (1.15 B + 8) or "none"."""
    b = np.asarray(b, np.float64)
    if change == "+20":
        b = b + 20.0
    elif change == "ramp":
        y, x = np.mgrid[0:b.shape[0], 0:b.shape[1]]
        b = b + 0.15 * x + 0.05 * y
    elif change == "gain":
        b = 1.15 * b + 8.0
    else:
        assert change == "none", change
    return np.ascontiguousarray(b, np.float32)


# (frame, psz, lv_f, maxiter, eps, refine, step, change): psz 8 / 15 / 23, 32 and 17 reach the forms <1,1> / <4,1> / <8,2>;
# every form has an entry with eps = 0 (no stop decision: every node runs maxiter); the step-3 entry is the clamp row of
# c2fflow_cases; the status pair holds stopped nodes of every kind in every form.
TABLE = (
    ("100x77", 8, 2, 10, 0.0, None, 4, "ramp"),
    ("100x77", 15, 2, 10, 0.01, None, 4, "+20"),
    ("67x53", 15, 2, 10, 0.0, None, 4, "gain"),
    ("67x53", 23, 2, 10, 0.01, None, 4, "+20"),
    ("67x53", 32, 2, 10, 0.0, None, 4, "ramp"),
    ("67x53", 8, 2, 10, 0.01, None, 3, "+20"),
    ("67x53", 8, 1, 2, 0.01, "refine", 4, "gain"),
    ("status-96x64", 8, 2, 10, 0.01, None, 4, "none"),
    ("status-96x64", 15, 2, 10, 0.01, None, 4, "none"),
    ("status-96x64", 17, 2, 10, 0.01, None, 4, "+20"),
)
STATUS_CASES = tuple(c for c in TABLE if c[0] == "status-96x64")
# the status values that occur over the three levels of the definition's and the restatement's run on the status pair
STATUS_REACHED = {8: (0, 1, 2, 3, 4), 15: (0, 1, 2, 3, 4), 17: (0, 1, 2, 3)}


def pad_of(case):
    return case[1] + PAD_EXTRA[TABLE.index(case) % 3]


def refine_of(case):
    return REFINE if case[5] else None


_pyr = {}


def host_pyramids(frame, change, pad, lv_f=2):
    """(oracle.Pyramid A, B) of a frame pair with B changed; shared, do not write to them. Needs the built oracle."""
    from oracle import oracle as O
    key = (frame, change, pad, lv_f)
    if key not in _pyr:
        a, b = CC.pair(frame)
        _pyr[key] = (O.Pyramid(a, lv_f, pad), O.Pyramid(changed(b, change), lv_f, pad))
    return _pyr[key]


def pyramids_of(case):
    return host_pyramids(case[0], case[7], pad_of(case), case[2])


@functools.lru_cache(maxsize=None)
def host_run(case):
    """(field, stages) of the definition with patnorm on a table entry."""
    from invcompcamtrack_amd import patchflow as pf
    frame, psz, lv_f, maxiter, eps, _, step, _ = case
    st = []
    out = pf.c2f_flow_host(*pyramids_of(case), step, psz, lv_f, maxiter, eps, refine=refine_of(case), _stages=st,
                           patnorm=True)
    return out, st


@functools.lru_cache(maxsize=None)
def restated(case, defect=None):
    """(field, [(level, field, d, status, bias)]) of the f32 restatement on a table entry."""
    import patnorm_f32 as R
    frame, psz, lv_f, maxiter, eps, _, step, _ = case
    st = []
    out = R.run(*pyramids_of(case), step, psz, lv_f, maxiter, eps, refine=refine_of(case), defect=defect, stages=st)
    return out, st


def level_differences(case, defect=None):
    """Per level of a table entry, the restatement's search and bias from the definition's own starts against the
    definition: [(level, nodes, left out, statuses equal on the compared nodes, worst |d - definition|, worst |beta -
    definition|, on them)]."""
    import patnorm_f32 as R
    frame, psz, lv_f, maxiter, eps, _, step, _ = case
    pa, pb = pyramids_of(case)
    out = []
    for s in host_run(case)[1]:
        keep = CC.compared(s, eps)
        d, lost, status, bias = R.search(pa, pb, s["level"], s["init"], step, psz, maxiter, eps, defect=defect)
        same = bool(np.array_equal(status[keep], s["status"][keep]))
        votes = keep & (s["status"] != 0) & ~lost
        diff = float(np.abs(d.astype(np.float64) - s["d"])[votes].max()) if votes.any() else 0.0
        bdiff = float(np.abs(bias.astype(np.float64) - s["bias"])[keep].max()) if keep.any() else 0.0
        out.append((s["level"], keep.size, int((~keep).sum()), same, diff, bdiff))
    return out


# level -> worst |restatement - definition| over TABLE on the compared nodes, from the same starts, of d in px and of beta
# in grey levels; measured by test_patnorm_cpu.py. Levels 0 and 1 are set by the status pair, whose runaway nodes move by
# several px per step over a ramp of 2.5 grey levels per px; without it the table stays below 6.2e-5 px and 9.0e-5.
D_DIFF = {0: 6.7e-4, 1: 1.2e-4, 2: 3.9e-6}
BIAS_DIFF = {0: 5.7e-3, 1: 1.4e-3, 2: 8.4e-5}
# worst |restatement - definition| of the final field in px over the entries with eps = 0 (whole runs), measured there too
FIELD_DIFF = 1.9e-5
# the worst share of nodes left out at a level of 20 nodes or more (cap: c2fflow_cases.LEFT_OUT_CAP), with its entry
LEFT_OUT = (0.0834, ("67x53", 8, 3, 2))   # (frame, psz, step, level): 2 of 24 nodes; (100x77, 8, eps 0.01, +20) would
# leave out 4 of 30 at level 2, which is why its eps is 0 here

# ---------------------------------------------------------------- offset invariance and usefulness, on the definitions
USEFUL_PSZ, USEFUL_LV, STEP = CC.USEFUL_PSZ, CC.USEFUL_LV, CC.STEP
KINDS = ("layers", "rotzoom")


@functools.lru_cache(maxsize=None)
def useful_field(kind, seed, change, patnorm):
    """c2f_flow_host's field on a usefulness scene of c2fflow_cases with frame B changed."""
    from invcompcamtrack_amd import patchflow as pf
    from oracle import oracle as O
    a, b, _, _ = CC.useful_inputs(kind, seed)
    pa, pb = O.Pyramid(a, USEFUL_LV, USEFUL_PSZ), O.Pyramid(changed(b, change), USEFUL_LV, USEFUL_PSZ)
    return pf.c2f_flow_host(pa, pb, STEP, USEFUL_PSZ, USEFUL_LV, patnorm=patnorm)


def useful_error(kind, seed, change, patnorm):
    """Its mean endpoint error in px, 16 px inside the frame."""
    _, _, truth, mask = CC.useful_inputs(kind, seed)
    return FC.epe(useful_field(kind, seed, change, patnorm), truth, mask)


# worst |field(A, B + 20) - field(A, B)| in px of the definition with patnorm over both scenes and flowrefine_cases.SEEDS
# ("rotzoom" seed 1, where one stop decision falls the other way; the other five stay below 2.5e-6 px)
OFFSET_DIFF = 0.21
# (A, B + 20): the definition's worst patnorm / plain error ratio over both scenes and the seeds, with its scene; the bar
# is the project's form, the worst seed's ratio plus a quarter of its gain.
# Mean endpoint errors in px, seeds 0 / 1 / 2, plain -> patnorm:
#   layers  B       0.2755 / 0.2890 / 0.2979 -> 0.3107 / 0.3143 / 0.3605   (the cost: 13, 9, 21 %)
#   layers  B + 20  1.8631 / 2.2934 / 2.2299 -> 0.3107 / 0.3143 / 0.3605
#   layers  ramp    1.3575 / 1.7504 / 1.5722 -> 0.3157 / 0.3234 / 0.3721
#   layers  gain    2.3689 / 2.7414 / 2.4223 -> 0.3204 / 0.3787 / 0.3993   (1.15 B + 8)
#   rotzoom B       0.1042 / 0.0744 / 0.0933 -> 0.1161 / 0.0841 / 0.1054   (the cost: 11, 13, 13 %)
#   rotzoom B + 20  3.0750 / 1.9160 / 2.1771 -> 0.1161 / 0.0841 / 0.1054
#   rotzoom ramp    2.0998 / 1.3731 / 1.5003 -> 0.1303 / 0.0919 / 0.1098
#   rotzoom gain    3.8874 / 2.3399 / 2.6364 -> 0.2017 / 0.1243 / 0.1707
USEFUL_OFFSET = (0.167, ("layers", 0))


def useful_bar():
    return USEFUL_OFFSET[0] + (1.0 - USEFUL_OFFSET[0]) / 4
