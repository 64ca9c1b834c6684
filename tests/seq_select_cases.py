"""Synthetic worlds for the between-pairs selection of a sequence (k_seq_select_count / _scatter / _finish,
ictr_sequence.hip) and the NumPy restatement of the finish kernel's f64 sums.

A workgroup of the count and scatter kernels owns C = 4096 consecutive world points (256 threads x 16 steps; one 64-bit
survivor mask per wave and step). The worlds choose, per world index, whether a point survives the cull, so that
ranks, stride phases and the cap limit cross workgroup bounds in known places. Nothing here needs a GPU:
``select_points`` decides what each case reaches (tests/test_sequence_cpu.py), the device is compared with it in
tests/test_gpu_sequence_select.py.

Identity-pose worlds (p0 = 0, G = I exactly): the device and ``select_points`` form ``fx * X / Z + cx`` from the same
f64 operands in the same order, so the keep decision is the same in the bits, also for a point exactly on a bound.
The camera's fc and cc are dyadic (32 and 0), so a point at Z = 1 lands on the pixel it was built from, exactly.
"""
import functools

import numpy as np

C = 4096            # kSeqChunk: world points per workgroup
BLOCK = 256         # kSeqBlock: threads per workgroup (nblk > BLOCK: seq_prefix's loop takes a second trip)
FINISH = 256        # kSeqFinish: threads of the finish workgroup
W, H = 64, 48       # frame size of every case (two levels, padding 8)
CAM_ID = dict(fc=np.array([32.0, 32.0], np.float32), cc=np.array([0.0, 0.0], np.float32), wh=np.array([W, H], np.int32))
CAM_GEN = dict(fc=np.array([30.0, 32.0], np.float32), cc=np.array([20.0, 15.0], np.float32), wh=np.array([W, H], np.int32))
P_ZERO = np.zeros(6)
P_GEN = np.array([0.05, -0.02, 0.1, 0.01, -0.02, 0.03])  # (test_select_points_general_pose_and_cap's)
GEN_SEED = 2
# launch forms: psz 4 runs one workgroup per tracking up to 2048 points; psz 8 with a cap in (128, 8192] runs a team
SINGLE, TEAM = "single", "team"
PSZ = {SINGLE: 4, TEAM: 8}


def _world(keep, rng):
    """(3, nw) f64: kept points inside the view (u in [2, 62], v in [2, 46], Z in [1, 3]), dropped ones far outside."""
    keep = np.asarray(keep, bool)
    n = keep.size
    u, v, z = rng.uniform(2, 62, n), rng.uniform(2, 46, n), rng.uniform(1, 3, n)
    X = np.stack([u * z / 32.0, v * z / 32.0, z])
    out = np.stack([1000.0 + rng.uniform(0, 1, n), rng.uniform(-1, 1, n), np.ones(n)])
    X[:, ~keep] = out[:, ~keep]
    return np.ascontiguousarray(X)


def bounds_specials():
    """(3, 15) points at identity pose and their keep flags: on each of the four bounds, one f64 ulp outside each, both
    corners, NaN X, infinite Y, Z = 0, behind the camera with u, v inside (kept: there is no depth test) and outside."""
    dn, up = -np.inf, np.inf
    uv = [(1, 10), (W, 10), (10, 1), (10, H),
          (np.nextafter(1.0, dn), 10), (np.nextafter(float(W), up), 10), (10, np.nextafter(1.0, dn)),
          (10, np.nextafter(float(H), up)),
          (1, 1), (W, H)]
    pts = [(u / 32.0, v / 32.0, 1.0) for u, v in uv]
    keep = [True] * 4 + [False] * 4 + [True] * 2
    pts += [(np.nan, 10 / 32.0, 1.0), (10 / 32.0, np.inf, 1.0), (0.5, 0.5, 0.0),
            (-10 / 32.0, -10 / 32.0, -1.0), (1000.0, -10 / 32.0, -1.0)]
    keep += [False, False, False, True, False]
    return np.array(pts, np.float64).T.copy(), np.array(keep)


def _slots_keep():
    """Exactly one kept point per (step, wave) slot of each of two workgroups, each at a different lane."""
    keep = np.zeros(2 * C, bool)
    for blk, (mul, add) in enumerate(((37, 11), (29, 5))):  # odd multipliers: permutations of the 64 lanes
        for step in range(C // BLOCK):
            for wave in range(BLOCK // 64):
                j = step * (BLOCK // 64) + wave
                keep[blk * C + step * BLOCK + wave * 64 + (j * mul + add) % 64] = True
    return keep


@functools.lru_cache(maxsize=None)
def world(name):
    """dict(X (3, nw) f64, p0, cam, keep: the intended survivors or None where the pose decides)."""
    rng = np.random.default_rng(abs(hash_name(name)))
    cam, p0 = CAM_ID, P_ZERO
    if name == "tail1":
        keep = np.ones(C + 1, bool)
    elif name == "edge_pairs":
        keep = np.zeros(3 * C, bool)
        keep[[C - 1, C, 2 * C - 1, 2 * C]] = True
    elif name == "phase":
        keep = np.ones(2 * C + 100, bool)
    elif name == "cap_at_bound":
        keep = np.ones(3 * C, bool)
    elif name == "holes":
        keep = rng.uniform(size=4 * C + 613) < 0.5
        keep[:C] = False
        keep[2 * C:3 * C] = False
    elif name == "slots":
        keep = _slots_keep()
    elif name == "none":
        keep = np.zeros(2 * C + 100, bool)
    elif name == "sparse":
        keep = rng.uniform(size=5 * C + 613) < 0.01
    elif name == "bounds":
        sp, kp = bounds_specials()
        k = sp.shape[1]
        keep = np.zeros(3 * C, bool)
        X = _world(keep, rng)
        for blk in range(3):
            for at, shift in ((blk * C, blk), (blk * C + C - k, blk + 3)):  # rotated: another point on each end lane
                X[:, at:at + k] = np.roll(sp, shift, axis=1)
                keep[at:at + k] = np.roll(kp, shift)
        return dict(X=np.ascontiguousarray(X), p0=p0, cam=cam, keep=keep)
    elif name in ("many_wg_30", "many_wg_01"):
        keep = rng.uniform(size=257 * C + 5) < (0.3 if name == "many_wg_30" else 0.001)
        keep[-1] = True  # the five-point last workgroup counts a survivor
    elif name == "general":
        g = np.random.default_rng(GEN_SEED)
        n = 3 * C + 37
        X = np.ascontiguousarray(np.stack([g.uniform(-3, 6, n), g.uniform(-3, 5, n), g.uniform(2, 4, n)]))
        return dict(X=X, p0=P_GEN, cam=CAM_GEN, keep=None)
    else:
        raise KeyError(name)
    return dict(X=_world(keep, rng), p0=p0, cam=cam, keep=keep)


def hash_name(name):
    """A seed from the case's name (the same in every process, unlike hash())."""
    return int.from_bytes(name.encode()[:7].ljust(7, b"\0"), "little") % (2 ** 31)


_BOTH = ((SINGLE, 2048), (TEAM, 4096))
# case -> world, [(stride, [(form, cap), ...]), ...], the workgroups whose points the case's selections must contain
# (the union over its runs). Caps are multiples of 4, as ictr_optparam_init leaves them; so cap * stride cannot be
# C + 1 or 2 C + 1777 (both odd): cap_at_bound takes the nearest admissible limits, C + 4 and 2 C + 1780, and adds
# (1366, 4), whose last selected rank 3 * 1366 = C + 2 is the third point of workgroup 1.
TABLE = {
    "tail1": ("tail1", [(1, [(SINGLE, 2048), (TEAM, 8192)])], {0, 1}),
    "edge_pairs": ("edge_pairs", [(1, _BOTH)], {0, 1, 2}),
    "phase": ("phase", [(s, _BOTH) for s in (3, 7, 64, C, C + 1, 2 * C + 100, 2 * C + 101)], {0, 1, 2}),
    "cap_at_bound": ("cap_at_bound", [(2, [(SINGLE, 2048)]), (1, [(TEAM, 4096)]),          # cap * s = C
                                      (41, [(SINGLE, 100)]), (1, [(TEAM, 4100)]),           # C + 4
                                      (1366, [(SINGLE, 4)]),                                # last rank C + 2
                                      (9, [(SINGLE, 1108), (TEAM, 1108)])], {0, 1, 2}),     # 2 C + 1780
    "holes": ("holes", [(1, _BOTH), (5, _BOTH)], {1, 3, 4}),
    "slots": ("slots", [(1, _BOTH), (2, _BOTH)], {0, 1}),
    "sparse": ("sparse", [(1, _BOTH), (10, _BOTH)], {0, 1, 2, 3, 4, 5}),
    "bounds": ("bounds", [(1, _BOTH)], {0, 1, 2}),
    "many_wg_30": ("many_wg_30", [(1000, _BOTH), (1, _BOTH)], {0, 128, 256}),
    "many_wg_01": ("many_wg_01", [(1000, _BOTH), (1, _BOTH)], {0, 128, 256, 257}),
    "none": ("none", [(1, _BOTH), (3, _BOTH)], set()),  # nothing selected: the pose is carried
    "general": ("general", [(1, _BOTH), (3, _BOTH), (10, _BOTH)], {0, 1, 2, 3}),
}
CAP_LIMITS = {(2, 2048): C, (1, 4096): C, (41, 100): C + 4, (1, 4100): C + 4, (1366, 4): 4 * 1366, (9, 1108): 2 * C + 1780}


def runs(case=None):
    """[(case, stride, form, cap)] of the whole table, or of one case."""
    out = []
    for name, (_, strides, _) in TABLE.items():
        if case is None or case == name:
            out += [(name, s, form, cap) for s, forms in strides for form, cap in forms]
    return out


def nblk(nw):
    return (nw + C - 1) // C


@functools.lru_cache(maxsize=None)
def survivors(case):
    """World indices that survive the cull at the case's pose (stride 1, no cap)."""
    from invcompcamtrack_amd import sequence as sq
    wd = world(TABLE[case][0])
    s = sq.select_points(wd["X"], wd["p0"], wd["cam"], 1)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def expected(case, stride, cap):
    """The reference selection of one run (shared, read-only)."""
    from invcompcamtrack_amd import sequence as sq
    wd = world(TABLE[case][0])
    s = sq.select_points(wd["X"], wd["p0"], wd["cam"], stride, cap)
    s.setflags(write=False)
    return s


def _kernel_order_sum(terms):
    """Sum of `terms` as k_seq_select_finish forms it: thread tid adds terms[tid], terms[tid + 256], ... left to right
    onto 0.0, then the halving tree over the 256 partial sums (slot tid += slot tid + h for h = 128, 64, ..., 1)."""
    terms = np.asarray(terms, np.float64)
    part = np.zeros(FINISH, np.float64)
    for at in range(0, terms.size, FINISH):
        seg = terms[at:at + FINISH]
        part[:seg.size] = part[:seg.size] + seg
    h = FINISH // 2
    while h > 0:
        part[:h] = part[:h] + part[h:2 * h]
        h //= 2
    return part[0]


def finish_sums(X, sel):
    """(ms (3,) f64, varval f64) of the selected points in the finish kernel's order: the mean of each coordinate, then
    the mean of the squared radii p1*p1 + p2*p2 + p3*p3 about it (each product and sum rounded, no FMA)."""
    sel = np.asarray(sel, np.int64)
    n = float(sel.size)
    P = np.asarray(X, np.float64)[:, sel]
    ms = np.array([_kernel_order_sum(P[c]) / n for c in range(3)])
    p1, p2, p3 = P[0] - ms[0], P[1] - ms[1], P[2] - ms[2]
    return ms, _kernel_order_sum(p1 * p1 + p2 * p2 + p3 * p3) / n
