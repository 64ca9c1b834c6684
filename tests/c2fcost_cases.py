"""Cases, recorded differences and usefulness figures for the Huber patch cost of the coarse-to-fine dense flow (cost="huber":
the ROBUST forms of k_c2f_level, csrc/ictr_c2fflow_robust.hip), shared by test_c2fcost_cpu.py and test_gpu_c2fcost.py.

The definition is patchflow.c2f_flow_host(..., cost="huber", huber_k=k) (f64). c2fcost_f32.py restates the kernels in f32;
the GPU tests demand its bits of the device, per level (d, status, bias under patnorm, field) and of the final field. The
CPU module compares the restatement with the definition level by level from the SAME starts on the nodes where every
decision of the definition has its margin (c2fflow_cases.compared: a clip is continuous and adds no decision); the worst
differences are RECORDED here and measured again by test_c2fcost_cpu.py, which fails above a record or below half of it.
Nothing here is fitted to the device.

The frames are c2fflow_cases.pair's (grey) and c2frgb_cases.colour_pair's (colour) with frame B SALTED, per channel:
rng = numpy.random.default_rng(SALT_SEED + channel); a pixel is salted where rng.random(shape) < SALT_SHARE, and a salted
pixel is 0 where a second draw rng.random(shape) < 0.5 and 255 otherwise. Under patnorm frame B is then changed by
patnorm_cases.changed(B, "+20") (the salt moves with it), so that the removed means matter.
"""
from __future__ import annotations

import functools

import numpy as np

import c2fflow_cases as CC
import c2frgb_cases as RC
import flowrefine_cases as FC
import patnorm_cases as PN

PAD_EXTRA = CC.PAD_EXTRA       # pyramids padded by psz + one of these, in rotation over the table
REFINE = CC.REFINE
SALT_SEED, SALT_SHARE = 4100, 0.08
CHANGE = "+20"                 # patnorm_cases.changed's change of frame B in the patnorm entries


def salted(b, channel=0, seed=SALT_SEED):
    """Frame B (h, w) with SALT_SHARE of its pixels set to 0 or 255 by the rule above; float32."""
    rng = np.random.default_rng(seed + channel)
    hit = rng.random(b.shape) < SALT_SHARE
    low = rng.random(b.shape) < 0.5
    return np.ascontiguousarray(np.where(hit, np.where(low, 0.0, 255.0), b), np.float32)


# (frame, psz, lv_f, maxiter, eps, step, x_only, patnorm, channels, huber_k, lv_l); lv_l = "refine-1": lv_l 1 with the
# refinement REFINE at every level. psz 8 / 15 / 17, 23, 32 are the forms <1,1> / <4,1> / <8,2>; each of them runs 2-D and
# x_only, with and without patnorm, on grey frames, and with and without patnorm on colour frames; every form has entries
# with eps = 0 (no stop decision: every node runs maxiter); k is 5 or 1.5; the status pair holds stopped nodes of every kind;
# the step-3 entry is the clamp row of c2fflow_cases. <8,2> with patnorm on colour frames (72 template floats and 24 kept
# window values per lane) runs 2-D and x_only.
TABLE = (
    ("100x77", 8, 2, 10, 0.0, 4, False, False, 1, 5.0, 0),
    ("67x53", 8, 2, 10, 0.01, 4, False, True, 1, 1.5, 0),
    ("67x53", 8, 2, 10, 0.0, 4, True, False, 1, 1.5, 0),
    ("67x53", 8, 2, 10, 0.01, 4, True, True, 1, 5.0, 0),
    ("67x53", 15, 2, 10, 0.01, 4, False, False, 1, 1.5, 0),
    ("100x77", 15, 2, 10, 0.0, 4, False, True, 1, 5.0, 0),
    ("67x53", 15, 2, 10, 0.01, 4, True, False, 1, 5.0, 0),
    ("67x53", 15, 2, 10, 0.0, 4, True, True, 1, 1.5, 0),
    ("67x53", 17, 2, 10, 0.0, 4, False, False, 1, 5.0, 0),
    ("67x53", 23, 2, 10, 0.0, 4, False, True, 1, 1.5, 0),
    ("67x53", 17, 2, 10, 0.01, 4, True, False, 1, 1.5, 0),
    ("67x53", 32, 2, 10, 0.0, 4, True, True, 1, 5.0, 0),
    ("67x53", 8, 2, 10, 0.01, 4, False, False, 3, 5.0, 0),
    ("67x53", 8, 2, 10, 0.0, 4, False, True, 3, 1.5, 0),
    ("67x53", 15, 2, 10, 0.0, 4, False, False, 3, 1.5, 0),
    ("100x77", 15, 2, 10, 0.01, 4, True, True, 3, 5.0, 0),
    ("67x53", 17, 2, 10, 0.01, 4, False, False, 3, 5.0, 0),
    ("67x53", 17, 2, 10, 0.0, 4, False, True, 3, 5.0, 0),
    ("67x53", 17, 2, 10, 0.01, 4, True, True, 3, 1.5, 0),
    ("status-96x64", 8, 2, 10, 0.01, 4, False, False, 1, 5.0, 0),
    ("status-96x64", 17, 2, 10, 0.01, 4, False, True, 1, 5.0, 0),
    ("67x53", 8, 2, 10, 0.01, 3, False, True, 1, 5.0, 0),
    ("100x77", 8, 2, 10, 0.01, 4, False, True, 1, 5.0, "refine-1"),
)
FORM = {8: (1, 1), 15: (4, 1), 17: (8, 2), 23: (8, 2), 32: (8, 2)}
for _form in ((1, 1), (4, 1), (8, 2)):
    _e = [c for c in TABLE if FORM[c[1]] == _form]
    assert {(c[6], c[7]) for c in _e if c[8] == 1} == {(False, False), (False, True), (True, False), (True, True)}
    assert {c[7] for c in _e if c[8] == 3} == {False, True}
    assert any(c[4] == 0.0 for c in _e)
assert {c[9] for c in TABLE} == {5.0, 1.5} and any(c[5] == 3 for c in TABLE) and any(c[10] == "refine-1" for c in TABLE)


def case_id(case):
    return "-".join(str(v) for v in case)


def pad_of(case):
    return case[1] + PAD_EXTRA[TABLE.index(case) % 3]


def refine_of(case):
    return REFINE if case[10] == "refine-1" else None


def lv_l_of(case):
    return 1 if case[10] == "refine-1" else case[10]


frame_size = CC.frame_size


@functools.lru_cache(maxsize=None)
def frames(frame, channels, patnorm):
    """(A, B) of a table entry: (h, w) float32 each, (3, h, w) on colour frames; B salted and, under patnorm, changed."""
    if channels == 1:
        a, b = CC.pair(frame)
        b = salted(b)
        b = PN.changed(b, CHANGE) if patnorm else b
    else:
        a, b = RC.colour_pair(frame)
        b = np.stack([salted(b[c], c) for c in range(3)])
        b = np.stack([PN.changed(b[c], CHANGE) for c in range(3)]) if patnorm else b
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    for arr in (a, b):
        arr.setflags(write=False)
    return a, b


_pyr = {}


def pyramids_of(case):
    """(oracle.Pyramid A, B) of a table entry, lists of three on colour frames; shared, do not write to them. Needs the
    built oracle."""
    from oracle import oracle as O
    frame, psz, lv_f, channels, patnorm = case[0], case[1], case[2], case[8], case[7]
    key = (frame, pad_of(case), lv_f, channels, patnorm)
    if key not in _pyr:
        a, b = frames(frame, channels, patnorm)
        if channels == 1:
            _pyr[key] = (O.Pyramid(a, lv_f, pad_of(case)), O.Pyramid(b, lv_f, pad_of(case)))
        else:
            _pyr[key] = ([O.Pyramid(a[c], lv_f, pad_of(case)) for c in range(3)],
                         [O.Pyramid(b[c], lv_f, pad_of(case)) for c in range(3)])
    return _pyr[key]


@functools.lru_cache(maxsize=None)
def host_run(case, cost="huber"):
    """(field, stages) of the definition on a table entry."""
    from invcompcamtrack_amd import patchflow as pf
    frame, psz, lv_f, maxiter, eps, step, x_only, patnorm, _, k, _ = case
    st = []
    out = pf.c2f_flow_host(*pyramids_of(case), step, psz, lv_f, maxiter, eps, _stages=st, patnorm=patnorm, x_only=x_only,
                           lv_l=lv_l_of(case), refine=refine_of(case), cost=cost, huber_k=k)
    return out, st


@functools.lru_cache(maxsize=None)
def restated(case, defect=None, huber_k=None):
    """(field, [(level, field, d, status, bias)]) of the f32 restatement on a table entry (huber_k: instead of the
    entry's)."""
    import c2fcost_f32 as R
    frame, psz, lv_f, maxiter, eps, step, x_only, patnorm, _, k, _ = case
    st = []
    out = R.run(*pyramids_of(case), step, psz, lv_f, lv_l_of(case), maxiter, eps, patnorm, x_only,
                k if huber_k is None else huber_k, refine_of(case), defect, st)
    return out, st


@functools.lru_cache(maxsize=None)
def restated_l2(case):
    """The final field of the L2 restatements (c2fflow_f32, patnorm_f32, c2fdisp_f32, c2frgb_f32 under c2fup_f32's lv_l) on
    a table entry's frames."""
    import c2frgb_f32 as RGB
    import c2fup_f32 as UP
    frame, psz, lv_f, maxiter, eps, step, x_only, patnorm, channels, _, _ = case
    pa, pb = pyramids_of(case)
    if channels == 3:
        return RGB.run(pa, pb, step, psz, lv_f, lv_l_of(case), maxiter, eps, patnorm=patnorm, x_only=x_only,
                       refine_params=refine_of(case))
    return UP.run(pa, pb, step, psz, lv_f, lv_l_of(case), maxiter, eps, refine=refine_of(case), patnorm=patnorm,
                  x_only=x_only)


# ---------------------------------------------------------------- restatement against definition
def level_differences(case, defect=None):
    """Per level of a table entry, the restatement's search from the definition's own starts against the definition:
    [(level, nodes, left out, statuses equal on the compared nodes, worst |d - definition|, worst |beta - definition|)]."""
    import c2fcost_f32 as R
    frame, psz, lv_f, maxiter, eps, step, x_only, patnorm, _, k, _ = case
    pa, pb = pyramids_of(case)
    out = []
    for s in host_run(case)[1]:
        keep = CC.compared(s, eps)
        d, lost, status, bias = R.search(pa, pb, s["level"], s["init"], step, psz, maxiter, eps, patnorm, x_only, k, defect)
        same = bool(np.array_equal(status[keep], s["status"][keep]))
        votes = keep & (s["status"] != 0) & ~lost & (status == s["status"])
        diff = float(np.abs(d.astype(np.float64) - s["d"])[votes].max()) if votes.any() else 0.0
        bdiff = float(np.abs(bias.astype(np.float64) - s["bias"])[votes].max()) if patnorm and votes.any() else 0.0
        out.append((s["level"], keep.size, int((~keep).sum()), same, diff, bdiff))
    return out


# level -> worst |restatement - definition| over TABLE on the compared nodes, from the same starts, of d in px and (the
# patnorm entries) of beta in grey levels; measured by test_c2fcost_cpu.py.
# Level 0 of both is the step-3 entry's (a node that moves by px per step near the border); without it the table stays
# below 3.8e-4 px and 3.5e-4 grey levels.
D_DIFF = {0: 1.2e-3, 1: 5.4e-6, 2: 1.8e-6}
BIAS_DIFF = {0: 3.0e-3, 1: 5.0e-5, 2: 3.1e-5}
# worst |restatement - definition| of the final field in px over the entries with eps = 0 (whole runs, each from its own
# coarser field), measured there too
FIELD_DIFF = 8.0e-4     # TABLE[0] (100x77, psz 8, k = 5); the others stay below 3.2e-4
# the worst share of nodes left out at a level of 20 nodes or more (cap: c2fflow_cases.LEFT_OUT_CAP), on the definition
# alone, with its entry's index in TABLE and the level
LEFT_OUT = (0.0834, (21, 2))   # 2 of 24 nodes, the step-3 entry. ("100x77", psz 8, x_only, patnorm, eps 0.01) would leave
# out 3 of 30 at level 2, the cap itself, and with eps = 0 one of its nodes never settles; that form runs on 67x53 instead.

# The patnorm forms at huber_k = 1e30, where no residual is clipped, against the L2 patnorm forms (restatements; the device
# has their bits): the direct form rounds differently from b = s + mean(I) sum G. Worst |field difference| in px over the
# patnorm entries of TABLE with eps = 0; the test fails above the record or below half of it. Without patnorm the bits are
# equal.
IDENTITY_K = 1e30
IDENTITY_PATNORM_DIFF = 7.4e-4   # ("67x53", psz 23, k = 1.5's frames); the other five entries 3.7e-5 .. 3.6e-4

# ---------------------------------------------------------------- usefulness, on the definitions alone
USEFUL_PSZ, USEFUL_LV, STEP, USEFUL_K = CC.USEFUL_PSZ, CC.USEFUL_LV, CC.STEP, 5.0
KINDS = ("rotzoom", "layers")


@functools.lru_cache(maxsize=None)
def useful_error(kind, seed, salt, cost, patnorm=False):
    """Mean endpoint error in px, 16 px inside the frame, of c2f_flow_host on a usefulness scene of c2fflow_cases, frame B
    salted (salted(B, seed=SALT_SEED + 10 seed)) or clean, at USEFUL_PSZ, step 4, USEFUL_LV, huber_k = USEFUL_K."""
    from invcompcamtrack_amd import patchflow as pf
    from oracle import oracle as O
    a, b, truth, mask = CC.useful_inputs(kind, seed)
    if salt:
        b = salted(b, seed=SALT_SEED + 10 * seed)
    pa, pb = O.Pyramid(a, USEFUL_LV, USEFUL_PSZ), O.Pyramid(np.ascontiguousarray(b, np.float32), USEFUL_LV, USEFUL_PSZ)
    return FC.epe(pf.c2f_flow_host(pa, pb, STEP, USEFUL_PSZ, USEFUL_LV, cost=cost, huber_k=USEFUL_K, patnorm=patnorm),
                  truth, mask)


# Mean endpoint errors in px of the definitions, seeds 0 / 1 / 2, L2 -> Huber (k = 5), measured by test_c2fcost_cpu.py (the
# rows with a bar) and by a run of useful_error (the others):
#   rotzoom, B salted   0.9192 / 0.6353 / 0.7678 -> 0.2116 / 0.1564 / 0.1763   (ratios 0.230 / 0.246 / 0.230; bar 0.435)
#   layers,  B salted   0.7537 / 0.8786 / 0.8966 -> 0.3203 / 0.3444 / 0.3939   (ratios 0.425 / 0.392 / 0.439; bar 0.580)
#   rotzoom, clean      0.1042 / 0.0744 / 0.0933 -> 0.1037 / 0.0740 / 0.0934   (at most NO_WORSE x L2)
#   layers,  clean      0.2755 / 0.2890 / 0.2979 -> 0.2346 / 0.2273 / 0.2539   (at most NO_WORSE x L2)
# Recorded without a bar:
#   big (6.5, 2.0) / (-8.5, 4.0), clean   1.0265 / 2.2121 / 1.4965 -> 2.6109 / 3.9567 / 1.3209   (ratios 2.54 / 1.79 / 0.88)
#     With large motion the Huber cost is WORSE: the clipped residual has more local minima at the coarse levels, and a
#     node that starts several px off is held there. Neither more iterations nor a re-weighted H change that.
#   patnorm, rotzoom, B salted   0.9295 / 0.6682 / 0.8020 -> 0.6171 / 0.3843 / 0.4573   (the salt moves the removed means)
#   patnorm, layers,  B salted   0.8047 / 0.9154 / 0.9399 -> 0.5297 / 0.5988 / 0.6243
#   x_only on patchdisp_cases.scene(tilt, seed), B salted, psz 8, lv_f 2, mean |x error| in px, seeds 1 / 2 / 3:
#     20 deg   0.3615 / 0.2970 / 0.3303 -> 0.0492 / 0.0358 / 0.0432
#     45 deg   0.4801 / 0.4581 / 0.4639 -> 0.0636 / 0.0594 / 0.0690
USEFUL_SALTED = {"rotzoom": 0.246, "layers": 0.439}   # the worst seed's Huber / L2 ratio on the salted scene


def useful_bar(kind):
    """The project's form: the worst seed's ratio plus a quarter of its gain."""
    return USEFUL_SALTED[kind] + (1.0 - USEFUL_SALTED[kind]) / 4
