"""Cases, recorded differences and usefulness figures for the densification of a flow grid (csrc/ictr_densify.hip),
shared by test_densify_cpu.py and test_gpu_densify.py.

The definition is patchflow.densify_flow_host (f64). densify_f32.py restates the kernel in f32; its worst difference to the
definition over TABLE is RECORDED here (DIFF). test_densify_cpu.py measures it again and fails above the record or below
half of it; the GPU tests demand the restatement's bits of the device, so every figure here is the restatement's. Nothing
here is fitted to the device.

Frames: flowrefine_cases' 100x77, 67x53, farxy-320x64, its transpose, and the 9x7 crop, in which every footprint is clipped
on all sides. Node tables are injected (FlowGrid.set_nodes on the device): the tracker is not under test.
"""
from __future__ import annotations

import functools

import numpy as np

import flowrefine_cases as FC
from oracle import np_patchflow as NP

FRAMES = FC.FRAMES
# (step, psz): the defaults, psz = 2 step, a tiling (psz = step, even), stripes (psz < step), odd step under a wide even
# patch, every node a pixel, the 1-pixel patch, the widest patch
GEOMS = ((4, 15), (4, 8), (8, 8), (5, 4), (3, 16), (1, 3), (4, 1), (4, 32))
POWERS = (1, 2, 4)
PAD_EXTRA = (0, 1, 5)
BOUNDARY_PX, BOUNDARY_SHARE = 1e-3, 0.005  # pixels with a vote this close to the inside boundary may be left out
MINERR = 2.0
# kinds of node table:
#   smooth    a seeded smooth field sampled at the nodes, 30 % of the nodes lost
#   lost0     the same field, no node lost;   lost100   every node lost;   toprows   the node rows of the top third lost
#   outside   the field plus an offset that pushes the votes of the nodes near each of the four sides out of the frame there
#   tracked   the host oracle's tracking of the pair (oracle/np_patchflow.track_points), (4, 15) and (4, 8) only
KINDS = ("smooth", "lost0", "lost100", "toprows", "outside", "tracked")
# The smooth field's mean per frame, and its amplitude: four waves of at most AMP / 2 each keep every component within 0.4 px
# of a mean whose fraction is .45 or .55, so no seeded displacement comes within 0.05 px of a whole number, and no vote of
# a seeded table within 0.05 px of the inside boundary (with a wide patch a whole boundary row or column would otherwise
# collect such votes from its 64 nodes: 0.9 % of 67x53 at psz 32 with flowrefine_cases' field). Only the tracked tables
# have near pixels.
MEAN = {"farxy-320x64": (1.45, -0.55), "farxy-64x320": (-0.55, 1.45), "9x7": (0.45, -0.45)}
AMP = 0.2


def grid_dims(w, h, step):
    return len(range(step // 2, w, step)), len(range(step // 2, h, step))


def _table():
    out = []
    for f, frame in enumerate(FRAMES):
        for g, (step, psz) in enumerate(GEOMS):
            out.append((frame, step, psz, "smooth", POWERS[(f + g) % 3]))  # every frame x geometry
            out.append((frame, step, psz, "outside", POWERS[(f + g + 1) % 3]))
    for frame in ("100x77", "67x53", "9x7"):
        for step, psz in ((4, 15), (4, 8), (8, 8), (5, 4)):
            for k, kind in enumerate(("lost0", "lost100", "toprows")):
                out.append((frame, step, psz, kind, POWERS[k]))
    for frame in ("100x77", "67x53"):
        for step, psz in ((4, 15), (4, 8)):
            for power in POWERS:  # every power on the tracked tables and on the defaults' smooth table
                if (frame, step, psz) != NEAR_TRACKED:
                    out.append((frame, step, psz, "tracked", power))
                if (frame, step, psz, "smooth", power) not in out:
                    out.append((frame, step, psz, "smooth", power))
    return tuple(out)


# The oracle's tracking of 67x53 at psz 15 has one node whose d_y is within 1e-3 of -2: the 19 pixels of row 2 under its
# footprint (0.535 % of the frame) have a vote on the inside boundary, above BOUNDARY_SHARE. The table is not recorded
# against the definition; the device is held to the restatement's bits on it like on every other (GPU_TABLE).
NEAR_TRACKED = ("67x53", 4, 15)
TABLE = _table()  # (frame, step, psz, kind, power)
GPU_TABLE = TABLE + tuple(NEAR_TRACKED + ("tracked", p) for p in POWERS)


@functools.lru_cache(maxsize=None)
def oracle_nodes(frame_or_scene, step, psz, lv_f=2):
    """(d (ny, nx, 2) f32, lost (ny, nx) bool) of the host oracle's tracking A -> B; a lost node's d is 0. The pair is a
    frame's name or a (kind, seed) of flowrefine_cases.scene."""
    from oracle import oracle as O
    a, b = FC.pair(frame_or_scene) if isinstance(frame_or_scene, str) else FC.scene(*frame_or_scene)[:2]
    h, w = a.shape
    pa, pb = O.Pyramid(a, lv_f, psz), O.Pyramid(b, lv_f, psz)
    gx, gy = np.meshgrid(np.arange(step // 2, w, step, dtype=np.float32), np.arange(step // 2, h, step, dtype=np.float32))
    pts = np.stack([gx.ravel(), gy.ravel()], 1)
    new, ok, _ = NP.track_points(pa, pb, pts, psz, lv_f, 0, 10, 0.01)
    lost = ~np.asarray(ok, bool).reshape(gx.shape)
    d = np.asarray(new - pts, np.float32).reshape(gx.shape + (2,))
    d[lost] = 0
    d.setflags(write=False)
    lost.setflags(write=False)
    return d, lost


@functools.lru_cache(maxsize=None)
def nodes(frame, step, kind, psz=15):
    """(d (ny, nx, 2) f32, lost (ny, nx) bool) of a table entry; shared, do not write to them. psz matters to "tracked"."""
    if kind == "tracked":
        return oracle_nodes(frame, step, psz)
    w, h = FC.frame_size(frame)
    nx, ny = grid_dims(w, h, step)
    f = FC.smooth_field(w, h, 11 * len(frame) + w + step, MEAN.get(frame, (-0.45, -2.45)), AMP)
    d = np.ascontiguousarray(f[step // 2::step, step // 2::step])
    assert d.shape == (ny, nx, 2)
    rng = np.random.default_rng(1000 * step + w)
    lost = np.zeros((ny, nx), bool)
    if kind == "smooth":
        lost = rng.random((ny, nx)) < 0.3
    elif kind == "lost100":
        lost[:] = True
    elif kind == "toprows":
        lost[:max(ny // 3, 1)] = True
    elif kind == "outside":
        # the nodes in the outer fifth of the frame on each side (at least the outermost) move out over that side, by more
        # than the frame's fifth
        gi, gj = np.meshgrid(np.arange(nx), np.arange(ny))
        gx, gy = gi * step + step // 2, gj * step + step // 2
        ox, oy = float(round(0.2 * w) + 1), float(round(0.2 * h) + 1)  # whole pixels: see MEAN
        d = d.copy()
        d[..., 0] += np.where((gx < 0.2 * w) | (gi == 0), -ox, 0) + np.where((gx >= 0.8 * w) | (gi == nx - 1), ox, 0)
        d[..., 1] += np.where((gy < 0.2 * h) | (gj == 0), -oy, 0) + np.where((gy >= 0.8 * h) | (gj == ny - 1), oy, 0)
        d = d.astype(np.float32)
        lost = rng.random((ny, nx)) < 0.1
    elif kind != "lost0":
        raise KeyError(kind)
    d.setflags(write=False)
    lost.setflags(write=False)
    return d, lost


def filled(d, lost, w, h, step):
    """The node table after the grid's fill (what FlowGrid.nodes returns), on the host: dense_flow's fill."""
    from invcompcamtrack_amd import patchflow as pf
    out = np.array(d, np.float32)
    pf._dense_from_nodes(out, np.asarray(lost, bool), w, h, step)  # fills `out` in place
    return out


@functools.lru_cache(maxsize=None)
def host_run(frame, step, psz, kind, power):
    """(field, stages, near) of the definition; near marks the pixels with a vote within BOUNDARY_PX of the inside
    boundary. The tables are chosen so that these stay within BOUNDARY_SHARE of the frame."""
    from invcompcamtrack_amd import patchflow as pf
    a, b = FC.pair(frame)
    d, lost = nodes(frame, step, kind, psz)
    st = {}
    out = pf.densify_flow_host(a, b, d, lost, step, psz, MINERR, power, _stages=st)
    near = st["edge"] < BOUNDARY_PX
    assert near.mean() <= BOUNDARY_SHARE, (frame, step, psz, kind, "choose another table: votes at the inside boundary",
                                            near.mean())
    return out, st, near


@functools.lru_cache(maxsize=None)
def restated(frame, step, psz, kind, power, defect=None):
    """(field, stages) of the f32 restatement on the host's fill of the table."""
    import densify_f32 as R
    a, b = FC.pair(frame)
    d, lost = nodes(frame, step, kind, psz)
    w, h = FC.frame_size(frame)
    st = {}
    out = R.densify(a, b, filled(d, lost, w, h, step), lost, step, psz, MINERR, power, defect=defect, stages=st)
    return out, st


def differences(case, got, stages):
    """(worst |field - definition|, worst relative |wsum - definition|, count planes equal) outside the near pixels."""
    ref, st, near = host_run(*case)
    keep = ~near
    e_f = float(np.abs(got.astype(np.float64) - ref.astype(np.float64))[keep].max()) if keep.any() else 0.0
    voted = keep & (st["count"] > 0)
    e_w = float((np.abs(stages["wsum"].astype(np.float64) - st["wsum"])[voted] / st["wsum"][voted]).max()) if voted.any() else 0.0
    same = bool(np.array_equal(stages["count"].astype(np.int64)[keep], st["count"][keep]))
    return e_f, e_w, same


# ---------------------------------------------------------------- recorded differences of the f32 restatement
# power -> (worst |restatement - definition| of the field in px, worst relative difference of the summed weight) over
# TABLE, near pixels left out. Measured by test_densify_cpu.py, which fails above a record or below half of it.
DIFF = {1: (3.3e-4, 1.1e-4), 2: (2.5e-3, 2.0e-4), 4: (1.1e-3, 3.7e-4)}
# the worst share of near pixels of a table entry (bar: BOUNDARY_SHARE), measured there too
NEAR_SHARE = 0.0

# A constant table: the geometries (4, 16, 36 and 64 votes per pixel), the constants, and the worst distance in ulps of f32
# of a pixel that took a vote from the constant, measured by test_densify_cpu.py. The rule states 2 ulp for the f32 form.
CONST_GEOMS = ((4, 8), (4, 15), (3, 16), (4, 32))
CONSTANTS = ((0.3, -0.7), (1.37, 0.001), (-2.6, 3.3))
CONST_ULP = {"definition": 0, "restatement": 0}

# ---------------------------------------------------------------- usefulness
# (scene kind, power) -> the definition's worst after / before over flowrefine_cases.SEEDS: mean endpoint errors over the
# scene's mask of the densified field against the up-sampled one, nodes tracked by the host oracle at psz 15, step 4.
# Measured by test_densify_cpu.py on the host function alone. The bar is flowrefine_cases.useful_bar's: after <= (ratio +
# (1 - ratio) / 4) before, the worst seed's ratio plus a quarter of its gain, so that the definition holds it on all three
# seeds without picking seeds.
USEFUL_PSZ, USEFUL_STEP = 15, 4
# layers: 0.945 -> 0.766 / 0.665 px (power 1 / 2), 0.923 -> 0.761 / 0.655, 0.977 -> 0.800 / 0.699; rotzoom: 0.104 -> 0.075 /
# 0.084, 0.077 -> 0.056 / 0.070, 0.084 -> 0.060 / 0.071.
USEFUL = {("layers", 1): 0.825, ("layers", 2): 0.716, ("rotzoom", 1): 0.730, ("rotzoom", 2): 0.908}
# densified (power 1) + refined (8 outer) against refined alone on "layers", mean endpoint errors per seed; no bar
REFINED = {0: (0.4635, 0.4584), 1: (0.4190, 0.4214), 2: (0.6524, 0.6282)}  # seed -> (refined alone, densified + refined)


def useful_bar(kind, power):
    ratio = USEFUL[kind, power]
    return ratio + (1.0 - ratio) / 4


def useful_inputs(kind, seed):
    """(img_a, img_b, d, lost, up-sampled field, truth, mask) of a usefulness scene."""
    a, b, f, truth, mask = FC.scene(kind, seed)  # tracked at flowrefine_cases' defaults: psz 15, step 4, lv_f 2
    d, lost = oracle_nodes((kind, seed), USEFUL_STEP, USEFUL_PSZ)
    return a, b, d, lost, f, truth, mask
