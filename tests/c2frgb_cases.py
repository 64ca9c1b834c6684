"""Cases, recorded differences and usefulness scenes for the coarse-to-fine dense flow on colour frames (the NCH = 3 forms of
csrc/ictr_c2fflow.hip and k_densify<BIAS, 3> of csrc/ictr_densify.hip), shared by test_c2frgb_cpu.py and test_gpu_c2frgb.py.

The definition is patchflow.c2f_flow_host on triples of pyramids (f64). c2frgb_f32.py restates the kernels in f32; the GPU
tests demand its bits of the device, per level and of the final field. The CPU module compares the restatement with the
definition level by level from the SAME starts, on the nodes where every decision of the definition keeps
c2fflow_cases.MARGIN_*; the worst differences are RECORDED here and measured again by test_c2frgb_cpu.py, which fails above
a record or below half of it. Nothing here is fitted to the device.

The channels of a frame differ: independent textures per channel under one motion, and for the patnorm runs frame B's
channels are offset by +20 / -10 / 0 grey levels, so that a swapped or repeated channel shows."""
from __future__ import annotations

import functools

import numpy as np

import c2fflow_cases as CC
import flowrefine_cases as FC
import patchflow_cases as PC

PAD_EXTRA = (0, 1, 5)          # pyramids padded by psz + one of these, in rotation over the table
OFFSETS = (20.0, -10.0, 0.0)   # frame B's per-channel brightness offsets in the patnorm runs
REFINE = dict(n_outer=1, n_sor=2)
# The status pair's channels are c2fflow_cases.status_pair at these seeds: of ten triples tried on the restatement, this one
# keeps every status value 0..4 in all three forms (psz 8 / 15 / 17; counts in test_c2frgb_cpu.py's output). With (0, 1, 2)
# psz 17 has no runaway node.
STATUS_SEEDS = (0, 1, 3)
# (frame, psz, lv_f, maxiter, eps, step, x_only, lv_l); lv_l = "refine": lv_l 0 with the refinement REFINE at every level.
# Every entry runs plain and with patnorm. 100x77 and 67x53 halve
# oddly; psz 8 / 15 / 17 are the forms <1,1> / <4,1> / <8,2> (17: the smallest two-wave patch), each with an entry at
# eps = 0; psz 32 once (eight full pixels per lane); lv_f 1 with maxiter 2; step 3 on 67x53 reaches the clamp row of the
# start; the status pair; two entries x_only; one with lv_l = 1.
TABLE = (
    ("100x77", 8, 2, 10, 0.01, 4, False, 0),
    ("100x77", 15, 2, 10, 0.0, 4, False, 0),
    ("67x53", 8, 2, 10, 0.0, 4, False, 0),
    ("67x53", 17, 2, 10, 0.0, 4, False, 0),
    ("67x53", 32, 2, 10, 0.01, 4, False, 0),
    ("67x53", 8, 1, 2, 0.01, 4, False, 0),
    ("67x53", 8, 2, 10, 0.01, 3, False, 0),
    ("status-96x64", 8, 2, 10, 0.01, 4, False, 0),
    ("100x77", 8, 2, 10, 0.01, 4, True, 0),
    ("67x53", 17, 2, 10, 0.01, 4, True, 0),
    ("100x77", 15, 2, 10, 0.01, 4, False, 1),
    ("67x53", 8, 2, 10, 0.01, 4, False, "refine"),
)
assert {c[1] for c in TABLE if c[4] == 0.0} == {8, 15, 17}
# the coloured status pair in the other two forms (plain), as c2fflow_cases.STATUS_FORMS
STATUS_FORMS = (("status-96x64", 15, 2, 10, 0.01, 4, False, 0), ("status-96x64", 17, 2, 10, 0.01, 4, False, 0))
RUNS = tuple((c, pn) for c in TABLE for pn in (False, True))
DEFECT_CASE = TABLE[-1]        # the entry the injected defects are shown on, with patnorm (beta exists) and refinement


def case_id(case):
    return "-".join(str(v) for v in case)


def pad_of(case):
    return case[1] + (1 if case in STATUS_FORMS else PAD_EXTRA[TABLE.index(case) % 3])


frame_size = CC.frame_size


@functools.lru_cache(maxsize=None)
def colour_pair(frame, offsets=False):
    """(A, B): two (3, h, w) float32 colour frames. 'WxH': patchflow_cases' scene and motion with three texture seeds.
    'status-96x64': c2fflow_cases.status_pair with three seeds (the flat band and the jumping ramp block are in every
    channel). offsets: frame B's channels + OFFSETS."""
    if frame == "status-96x64":
        ch = [CC.status_pair(seed) for seed in STATUS_SEEDS]
    else:
        from invcompcamtrack_amd import synth
        w, h = PC.SIZES[frame]
        ch = []
        for k in range(3):
            sc = synth.make_scene(w, h, n_points=4, seed=PC.SYNTH_SEED[frame], tex_seed=1234 + k,
                                  dp_gt=np.array([0.1, -0.06, 0.05, 0.02, -0.015, 0.01]))
            ch.append((sc["img_a"], sc["img_b"]))
    a = np.ascontiguousarray(np.stack([c[0] for c in ch]), np.float32)
    b = np.stack([c[1] for c in ch]).astype(np.float64)
    if offsets:
        b = b + np.array(OFFSETS)[:, None, None]
    b = np.ascontiguousarray(b, np.float32)
    for arr in (a, b):
        arr.setflags(write=False)
    return a, b


_pyr = {}


def host_pyramids(frame, pad, lv_f=2, offsets=False, equal=False):
    """([oracle.Pyramid A_c], [B_c]) of a colour pair; shared, do not write to them. equal: channel 0 three times.
    Needs the built oracle."""
    from oracle import oracle as O
    key = (frame, pad, lv_f, offsets, equal)
    if key not in _pyr:
        a, b = colour_pair(frame, offsets)
        pa = [O.Pyramid(a[c], lv_f, pad) for c in range(3)]
        pb = [O.Pyramid(b[c], lv_f, pad) for c in range(3)]
        _pyr[key] = ([pa[0]] * 3, [pb[0]] * 3) if equal else (pa, pb)
    return _pyr[key]


def refine_of(case):
    return REFINE if case[7] == "refine" else None


def lv_l_of(case):
    return 0 if case[7] == "refine" else case[7]


def pyramids_of(case, patnorm):
    return host_pyramids(case[0], pad_of(case), case[2], offsets=patnorm)


@functools.lru_cache(maxsize=None)
def host_run(case, patnorm):
    """(field, stages) of the definition on a table entry."""
    from invcompcamtrack_amd import patchflow as pf
    frame, psz, lv_f, maxiter, eps, step, x_only, lv_l = case
    st = []
    out = pf.c2f_flow_host(*pyramids_of(case, patnorm), step, psz, lv_f, maxiter, eps, _stages=st, patnorm=patnorm,
                           x_only=x_only, lv_l=lv_l_of(case), refine=refine_of(case))
    return out, st


@functools.lru_cache(maxsize=None)
def restated(case, patnorm, defect=None):
    """(field, [(level, field, d, status, bias)]) of the f32 restatement on a table entry."""
    import c2frgb_f32 as R
    frame, psz, lv_f, maxiter, eps, step, x_only, lv_l = case
    st = []
    out = R.run(*pyramids_of(case, patnorm), step, psz, lv_f, lv_l_of(case), maxiter, eps, patnorm=patnorm, x_only=x_only,
                defect=defect, stages=st, refine_params=refine_of(case))
    return out, st


# ---------------------------------------------------------------- restatement against definition
compared = CC.compared


def level_differences(case, patnorm, defect=None):
    """Per level of a table entry, the restatement's search from the definition's own starts against the definition:
    [(level, nodes, left out, statuses equal on the compared nodes, worst |d - definition|, worst |beta - definition|)]."""
    import c2frgb_f32 as R
    frame, psz, lv_f, maxiter, eps, step, x_only, lv_l = case
    pa, pb = pyramids_of(case, patnorm)
    out = []
    for s in host_run(case, patnorm)[1]:
        keep = compared(s, eps)
        d, lost, status, bias = R.search(pa, pb, s["level"], s["init"], step, psz, maxiter, eps, patnorm, x_only, defect)
        same = bool(np.array_equal(status[keep], s["status"][keep]))
        votes = keep & (s["status"] != 0) & ~lost & (status == s["status"])
        diff = float(np.abs(d.astype(np.float64) - s["d"])[votes].max()) if votes.any() else 0.0
        bdiff = float(np.abs(bias.astype(np.float64) - s["bias"])[votes].max()) if patnorm and votes.any() else 0.0
        out.append((s["level"], keep.size, int((~keep).sum()), same, diff, bdiff))
    return out


# level -> worst |restatement - definition| of d in px over RUNS on the compared nodes, from the same starts; measured by
# test_c2frgb_cpu.py. As in c2fflow_cases.D_DIFF, levels 0 and 1 are set by the status pair's runaway nodes.
D_DIFF = {0: 5.3e-4, 1: 1.9e-4, 2: 1.7e-6}
# worst |restatement - definition| of beta in grey levels over the patnorm runs, likewise
BETA_DIFF = 5.3e-4     # the status pair's runaway nodes; without it 7.2e-5
# worst |restatement - definition| of the final field in px over the runs with eps = 0 (whole runs, each from its own
# coarser field)
FIELD_DIFF = 1.9e-5
# the same of the entry with the refinement (eps = 0.01: its nodes' stop decisions are the definition's here), plain
# and patnorm
REFINE_FIELD_DIFF = 7.2e-6
# the worst share of nodes left out at a level of 20 nodes or more (cap: c2fflow_cases.LEFT_OUT_CAP), on the definition
# alone, with its run
LEFT_OUT = (0.083, (("status-96x64", 8, 2, 10, 0.01, 4, False, 0), False, 2))   # 2 of 24 nodes, plain, level 2

# Three equal channels (channel 0 three times) against the grey rule on that channel: TABLE[0], the status entry and the
# entry with the refinement (search, bias, vote AND the refinement's joint weights and channel means against the grey
# coefficients), each plain and patnorm. The definition: to within f64 rounding (EQUAL_HOST, px). The f32 restatement:
# equal statuses and a field that is close, not equal in bits, because H, b and the coefficients are summed three times
# (EQUAL_F32, px, per (entry, patnorm); the status pair's is its runaway nodes').
EQUAL_CASES = (TABLE[0], TABLE[7], TABLE[-1])
EQUAL_HOST = 1e-9       # measured: 0.0 in all six runs (the sums of three equal terms and their quotients are exact here)
# the refinement alone (test_c2frgb_cpu.py: 67x53, a smooth field, 3 outer x 5 SOR), f32 restatements, by x_only, px
EQUAL_REFINE_F32 = {False: 3.3e-4, True: 6.3e-6}
EQUAL_F32 = {(0, False): 3.4e-6, (0, True): 1.9e-3, (1, False): 0.14, (1, True): 4.5e-3, (2, False): 1.7e-5, (2, True): 3.8e-3}

# ---------------------------------------------------------------- usefulness, on the host definition
USEFUL_PSZ, USEFUL_LV, STEP = 8, 3, 4


@functools.lru_cache(maxsize=None)
def isoluminant_scene(seed, kind="iso"):
    """flowrefine_cases.scene("layers")'s two layers with the texture a placed isoluminantly: channels 128 + a', 128 - a',
    128 with a' = a - 128, so that the channel mean is flat. Returns (A, B (3, h, w) f32, truth, mask 16 px inside).
    kind "mixed": the foreground rectangle isoluminant, the background's texture in all three channels (luminance)."""
    w, h = FC.SCENE_W, FC.SCENE_H
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x0, y0, x1, y1 = FC.RECT
    in_a = (x >= x0) & (x < x1) & (y >= y0) & (y < y1)
    xr, yr = x - FC.D_RECT[0], y - FC.D_RECT[1]
    in_b = (xr >= x0) & (xr < x1) & (yr >= y0) & (yr < y1)
    fg_a = FC.texture(w, h, 100 + seed) - 128.0
    bg_a = FC.texture(w, h, 200 + seed) - 128.0
    fg_b = FC.texture(w, h, 100 + seed, lambda X, Y: (X - FC.D_RECT[0], Y - FC.D_RECT[1])) - 128.0
    bg_b = FC.texture(w, h, 200 + seed, lambda X, Y: (X - FC.D_BG[0], Y - FC.D_BG[1])) - 128.0
    iso = lambda t: np.stack([128.0 + t, 128.0 - t, np.full_like(t, 128.0)])
    lum = lambda t: np.stack([128.0 + t] * 3)
    bg = iso if kind == "iso" else lum
    a = np.where(in_a[None], iso(fg_a), bg(bg_a))
    b = np.where(in_b[None], iso(fg_b), bg(bg_b))
    rng_a, rng_b = np.random.default_rng(2 * seed + 1), np.random.default_rng(2 * seed + 2)
    if kind == "iso":  # noise that keeps the channel mean flat: the grey search sees nothing at all but its own noise
        na, nb = rng_a.normal(0, 2.0, (h, w)), rng_b.normal(0, 2.0, (h, w))
        a = a + np.stack([na, -na, np.zeros_like(na)])
        b = b + np.stack([nb, -nb, np.zeros_like(nb)])
    else:
        a, b = a + rng_a.normal(0, 2.0, a.shape), b + rng_b.normal(0, 2.0, b.shape)
    truth = np.where(in_a[..., None], np.array(FC.D_RECT), np.array(FC.D_BG))
    mask = (x >= 16) & (x < w - 16) & (y >= 16) & (y < h - 16)
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32), truth, mask


def useful_errors(seed, kind="iso"):
    """Mean endpoint errors in px of the definitions at USEFUL_PSZ, step 4, USEFUL_LV: (grey c2f_flow_host on the channel
    mean, colour c2f_flow_host, grey c2f_flow_host on the luminance twin 128 + a')."""
    from invcompcamtrack_amd import patchflow as pf
    from oracle import oracle as O
    a, b, truth, mask = isoluminant_scene(seed, kind)
    pyr = lambda img: O.Pyramid(np.ascontiguousarray(img, np.float32), USEFUL_LV, USEFUL_PSZ)
    mean = lambda f: f.astype(np.float64).mean(axis=0)
    grey = pf.c2f_flow_host(pyr(mean(a)), pyr(mean(b)), STEP, USEFUL_PSZ, USEFUL_LV)
    col = pf.c2f_flow_host([pyr(c) for c in a], [pyr(c) for c in b], STEP, USEFUL_PSZ, USEFUL_LV)
    twin = pf.c2f_flow_host(pyr(a[0]), pyr(b[0]), STEP, USEFUL_PSZ, USEFUL_LV)
    return FC.epe(grey, truth, mask), FC.epe(col, truth, mask), FC.epe(twin, truth, mask)


# the definition's worst colour / grey ratio over flowrefine_cases.SEEDS on the isoluminant scene, measured by
# test_c2frgb_cpu.py; the bar is the project's form: the worst seed's ratio plus a quarter of its gain
# Mean endpoint errors grey -> colour (grey on the luminance twin): 1.512 -> 0.282 (0.275), 1.512 -> 0.299 (0.289),
# 1.512 -> 0.306 (0.298) px; ratios 0.186, 0.198, 0.202. The grey error is the motion itself: every node is held by the
# conditioning test. Mixed scene, no bar: 0.923 -> 0.258, 0.863 -> 0.274, 0.917 -> 0.288 px.
USEFUL_ISO = 0.203


def useful_bar():
    return USEFUL_ISO + (1.0 - USEFUL_ISO) / 4
