"""Inputs of the window camera RANSAC tests: seeded windows with known poses, the wrong-depth scenes of the usefulness test
and crafted inputs that random windows do not reach. Every crafted case names the branch it is made for;
test_camransac_cpu.py asserts on the host that it gets there."""
import functools

import numpy as np

import camfit_cases as K

CAM = K.CAM
OFFSET = np.array([K.BASELINE, 0.0, 0.0])
XCAM = ((1024.0, 512.0), (0.0, 0.0))   # the exact camera of ransac_cases: integer pixels carry no rounding
SHAPES_N = (4, 5, 63, 64, 65, 257, 1025)
SHAPES_FS = ((1, 1), (2, 2), (3, 2), (8, 2))
TRIALS = 64


def project(X, R, t, cam=CAM):
    (fx, fy), (cx, cy) = cam
    Xc = R @ X + np.asarray(t, np.float64)[:, None]
    return np.stack([fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy])


def _case(X, xy, reaches="", cam=CAM, offset=None, mask=None, ntrials=TRIALS, thresh=2.0, seed=0):
    xy = np.ascontiguousarray(xy, np.float64)
    if offset is None and xy.shape[0] == 2:
        offset = OFFSET
    return dict(X=np.ascontiguousarray(X, np.float64), xy=xy, cam=cam, offset=offset, mask=mask, ntrials=ntrials,
                thresh=thresh, seed=seed, reaches=reaches)


def window(n, nframes, nsides, seed, noise=0.3, outliers=0.2, cam=CAM):
    """X (3, n), xy (S, F, 2, n), G (F, 3, 4): the motion grows with the frame, the last share of the points is displaced by
    30 px in every frame after the first, on both sides."""
    rng = np.random.default_rng(seed)
    X = K.points(n, rng)
    out = np.arange(n) >= n - int(outliers * n)
    xy, G = np.empty((nsides, nframes, 2, n)), np.empty((nframes, 3, 4))
    for f in range(nframes):
        R, t = K.pose(0.05 * f, rng) if f else (np.eye(3), np.zeros(3))
        G[f] = np.hstack([R, t[:, None]])
        for s in range(nsides):
            p = project(X, R, t + s * OFFSET, cam)
            if f > 0:
                ang = rng.uniform(0, 2 * np.pi, n)
                p = p + out * 30.0 * np.stack([np.cos(ang), np.sin(ang)])
            xy[s, f] = p + rng.normal(0, 1.0, (2, n)) * noise
    return X, xy, G


def mask_of(n):
    """Clears every seventh point; the last word is partial unless 64 divides n."""
    return np.arange(n) % 7 != 3


@functools.lru_cache(maxsize=None)
def seeded(n, nframes, nsides, masked):
    X, xy, _ = window(n, nframes, nsides, seed=9000 + 10 * n + nframes)
    return _case(X, xy, mask=mask_of(n) if masked else None, seed=n + nframes)


def seeded_cases():
    return [(n, f, s, m) for n in SHAPES_N for (f, s) in SHAPES_FS for m in (False, True)]


# ---------------------------------------------------------------- crafted
def drawn_masked():
    X, xy, _ = window(6, 3, 2, seed=9101, outliers=0.0)
    mask = np.ones(6, bool)
    mask[2] = False
    return _case(X, xy, "a drawn point that does not count (mask)", mask=mask)


def drawn_nan():
    X, xy, _ = window(6, 3, 2, seed=9102, outliers=0.0)
    X = X.copy()
    X[1, 3] = np.nan
    return _case(X, xy, "a drawn point that does not count (NaN)")


def nan_right_one_frame():
    X, xy, _ = window(40, 4, 2, seed=9103)
    xy = xy.copy()
    xy[1, 2, 0, 7] = np.nan
    return _case(X, xy, "a NaN observation in one frame on the right side only")


def degenerate_frame():
    """Frame 1 shows points 0, 1 and 2 on one pixel row, in integer pixels of the exact camera: the 2-D triple product of a
    quadruple that holds all three is exactly 0 there and nowhere else."""
    X, xy, _ = window(5, 3, 2, seed=9104, outliers=0.0, cam=XCAM)
    xy = xy.copy()
    xy[0, 1, 0, :3] = np.round(xy[0, 1, 0, :3])
    xy[0, 1, 1, :3] = 64.0
    return _case(X, xy, "one frame's quadruple is degenerate", cam=XCAM)


def all_fail():
    """N = 4 and X2 = X0 + X1 in dyadic numbers: every trial draws all four, and the 3-D triple (0, 1, 2) is coplanar with
    the origin."""
    X = np.array([[1.0, 0.5, 4.0], [-0.75, 1.25, 8.0], [0.25, 1.75, 12.0], [-1.25, -0.25, 2.0]]).T.copy()
    xy = np.stack([np.stack([project(X, np.eye(3), np.array([0.125 * f, 0.0, 0.0]) + s * OFFSET) for f in range(2)])
                   for s in range(2)])
    return _case(X, xy, "every trial fails")


def exact_all_inliers():
    """Dyadic points seen without noise by cameras that only translate, and an infinite threshold, which also passes the
    trials whose P3P took a wrong root: every successful trial counts all N, so the lowest successful trial wins."""
    g = np.array([(x, y, z) for z in (2.0, 4.0, 8.0) for y in (-0.5, 0.25, 1.0) for x in (-1.0, -0.25, 0.5, 0.75)]).T
    X = g.copy()
    X[0] += 0.125 * X[2] * (np.arange(X.shape[1]) % 3)   # off the grid planes: no triple coplanar with the origin
    xy = np.stack([np.stack([project(X, np.eye(3), np.array([0.25 * f, -0.125 * f, 0.5 * f]) + s * OFFSET, XCAM)
                             for f in range(3)]) for s in range(2)])
    return _case(X, xy, "every successful trial counts all N", cam=XCAM, thresh=float("inf"))


def one_side():
    X, xy, _ = window(70, 4, 1, seed=9107)
    return _case(X, xy, "S = 1")


def one_frame():
    X, xy, _ = window(70, 1, 2, seed=9108)
    return _case(X, xy, "F = 1")


def depth_zero():
    """Point 9 lies in the camera plane of frame 1 (Zc = 0 under the true pose): its distance there is huge or not finite
    under every hypothesis, and it is never an inlier."""
    X, xy, G = window(30, 3, 2, seed=9109, outliers=0.0)
    X = X.copy()
    R, t = G[1][:, :3], G[1][:, 3]
    X[:, 9] = R.T @ (np.array([0.75, -0.25, 0.0]) - t)
    for s in range(2):
        for f in range(3):
            xy[s, f, :, 9] = (700.0, 300.0) if f == 1 else project(X[:, 9:10], G[f][:, :3], G[f][:, 3] + s * OFFSET)[:, 0]
    return _case(X, xy, "Zc = 0 for one point in one frame")


CRAFTED = dict(drawn_masked=drawn_masked, drawn_nan=drawn_nan, nan_right_one_frame=nan_right_one_frame,
               degenerate_frame=degenerate_frame, all_fail=all_fail, exact_all_inliers=exact_all_inliers,
               one_side=one_side, one_frame=one_frame, depth_zero=depth_zero)


@functools.lru_cache(maxsize=None)
def crafted(name):
    return CRAFTED[name]()


@functools.lru_cache(maxsize=None)
def host(name):
    """window_ransac_host of a crafted case with every trial's record, computed once."""
    from invcompcamtrack_amd import camransac as R
    c = crafted(name)
    return R.window_ransac_host(c["X"], c["xy"], c["cam"], c["offset"], c["mask"], c["ntrials"], c["thresh"], c["seed"],
                                detail=True)


@functools.lru_cache(maxsize=None)
def host_seeded(n, nframes, nsides, masked):
    from invcompcamtrack_amd import camransac as R
    c = seeded(n, nframes, nsides, masked)
    return R.window_ransac_host(c["X"], c["xy"], c["cam"], c["offset"], c["mask"], c["ntrials"], c["thresh"], c["seed"],
                                detail=True)


# ---------------------------------------------------------------- the scenes of the usefulness test
def stereo_inputs(xy_t):
    """The window as the RANSAC takes it: X (3, N) from the first view's disparity, xy (2, F, 2, N)."""
    from invcompcamtrack_amd import camfit as F
    X = F.points_from_first_view(xy_t, CAM, F.depth_from_disparity(xy_t, K.FC[0], K.BASELINE))
    left, right = F.observations_from_stereo_tracks(xy_t)
    return X, np.stack([left, right])


def wrong_depth_window(seed, shift=5.0):
    """stereo_window(seed=seed) with a fifth of the static points' right x of frame 0 moved by +-shift px (default_rng(5)):
    (xy_t, moving, moved, G)."""
    xy_t, moving, G = K.stereo_window(seed=seed)
    rng = np.random.default_rng(5)
    static = np.nonzero(~moving)[0]
    pick = rng.choice(static, len(static) // 5, replace=False)
    xy_t = xy_t.copy()
    xy_t[pick, 2, 0] += shift * rng.choice([-1.0, 1.0], len(pick))
    moved = np.zeros(len(moving), bool)
    moved[pick] = True
    return xy_t, moving, moved, G
