"""Inputs of the camera-fit tests: seeded scenes with known poses, crafted inputs that random scenes do not reach, and the
geometric stereo window of the chain split -> depth -> fit. Every crafted case names the branch it is made for;
test_camfit_cpu.py asserts on the host that it gets there."""
import numpy as np

FC, CC = (1000.0, 1000.0), (640.0, 360.0)
CAM = (FC, CC)
MOTIONS = (0.02, 0.1, 0.3, 0.6)   # rad and units
NOISES = (0.0, 0.3)               # px
BASELINE = -0.5                   # P1[0, 3] of the script: the right camera sees x_cam + (BASELINE, 0, 0)


def rot(w):
    """Rodrigues' formula (the tests' own, shared with nothing in the package)."""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def project(X, R, t):
    Xc = R @ X + np.asarray(t, np.float64)[:, None]
    return np.stack([FC[0] * Xc[0] / Xc[2] + CC[0], FC[1] * Xc[1] / Xc[2] + CC[1]])


def points(n, rng):
    z = rng.uniform(4.0, 12.0, n)
    return np.stack([rng.uniform(-0.5, 0.5, n) * z, rng.uniform(-0.3, 0.3, n) * z, z])


def pose(motion, rng):
    """A rotation by `motion` rad about a random axis and a translation of length `motion`."""
    w, t = rng.normal(size=3), rng.normal(size=3)
    return rot(w / np.linalg.norm(w) * motion), t / np.linalg.norm(t) * motion


def scene(n, motion, noise, seed):
    """One frame: X (3, n), xy (1, 2, n), the true pose G (3, 4)."""
    rng = np.random.default_rng(seed)
    X = points(n, rng)
    R, t = pose(motion, rng)
    xy = project(X, R, t) + rng.normal(0, 1.0, (2, n)) * noise
    return X, xy[None], np.hstack([R, t[:, None]])


def judged_scenes():
    """The 8 scenes of the judge: N = 200 .. 500, every motion at both noise levels."""
    out = []
    for i, (motion, noise) in enumerate((m, s) for s in NOISES for m in MOTIONS):
        out.append((motion, noise) + scene(200 + 100 * (i % 4), motion, noise, seed=500 + i))
    return out


def window(n, nframes, noise, seed):
    """nframes frames of the same n points, the motion growing with the frame (0.05 (f + 1)): X, xy (F, 2, n), G."""
    rng = np.random.default_rng(seed)
    X = points(n, rng)
    xy, G = np.empty((nframes, 2, n)), np.empty((nframes, 3, 4))
    for f in range(nframes):
        R, t = pose(0.05 * (f + 1), rng)
        xy[f] = project(X, R, t) + rng.normal(0, 1.0, (2, n)) * noise
        G[f] = np.hstack([R, t[:, None]])
    return X, xy, G


def identity(nframes=1):
    return np.tile(np.eye(3, 4)[None], (nframes, 1, 1))


# ---------------------------------------------------------------- crafted: dict(X, xy, mask, init, schedule, reaches)
def _case(X, xy, reaches, mask=None, init=None, **schedule):
    return dict(X=X, xy=xy, mask=mask, init=identity(xy.shape[0]) if init is None else init, schedule=schedule,
                reaches=reaches)


def few_by_mask():
    X, xy, _ = scene(50, 0.1, 0.0, 601)
    mask = np.zeros(50, bool)
    mask[[7, 31]] = True
    return _case(X, xy, "fewer than 3 counted", mask=mask)


def few_by_nan():
    X, xy, _ = scene(50, 0.1, 0.0, 602)
    xy = xy.copy()
    xy[0, 0, :48] = np.nan
    return _case(X, xy, "fewer than 3 counted")


def all_masked():
    X, xy, _ = scene(70, 0.1, 0.0, 603)
    return _case(X, xy, "fewer than 3 counted", mask=np.zeros(70, bool))


def depth_zero_at_start():
    X, xy, _ = scene(80, 0.1, 0.0, 604)
    X = X.copy()
    X[:, 5] = (1.0, 1.0, 0.0)
    return _case(X, xy, "start cost not finite")


def far_start():
    """The start is a turn of 2 rad away from the true pose: the first trial steps are rejected."""
    X, xy, G = scene(300, 0.3, 0.0, 605)
    init = np.hstack([rot([0.0, 2.0, 0.0]) @ G[:, :3], G[:, 3:4] + np.array([[2.0], [-1.0], [3.0]])])
    return _case(X, xy, "a rejected step", init=init[None], noiter=50)


def on_one_line():
    """Every point on the optical axis of the start pose, the observations off the principal point: the columns of t_z
    and w_z are exactly zero, so the third pivot is exactly 0 at every damping."""
    z = np.array([2.0, 4.0, 8.0, 16.0, 32.0, 64.0])
    X = np.stack([np.zeros(6), np.zeros(6), z])
    xy = np.stack([np.full(6, CC[0] + 3.0), np.full(6, CC[1] - 2.0)])[None]
    return _case(X, xy, "failed solve")


def nan_masked_and_not():
    """Two NaN observations, one under a cleared mask bit, and a cleared bit over a finite observation."""
    X, xy, _ = scene(300, 0.1, 0.3, 606)
    xy = xy.copy()
    xy[0, 1, 64] = np.nan   # masked out as well
    xy[0, 0, 255] = np.nan  # not masked: left out by the finite test
    mask = np.ones(300, bool)
    mask[[64, 100]] = False
    return _case(X, xy, "n = N - 3", mask=mask)


def no_iterations():
    X, xy, _ = scene(100, 0.1, 0.0, 607)
    return _case(X, xy, "noiter = 0", noiter=0)


def exact_dyadic():
    """Dyadic points and a power-of-two focal length seen from the identity: every projection is exact, c = 0."""
    g = np.array([(x, y, z) for z in (2.0, 4.0, 8.0) for y in (-0.5, 0.25, 1.0) for x in (-1.0, -0.25, 0.5, 0.75)]).T
    xy = np.stack([1024.0 * g[0] / g[2] + 640.0, 1024.0 * g[1] / g[2] + 360.0])[None]
    c = _case(g, xy, "c = 0 at the start")
    c["cam"] = ((1024.0, 1024.0), CC)
    return c


CRAFTED = dict(few_by_mask=few_by_mask, few_by_nan=few_by_nan, all_masked=all_masked,
               depth_zero_at_start=depth_zero_at_start, far_start=far_start, on_one_line=on_one_line,
               nan_masked_and_not=nan_masked_and_not, no_iterations=no_iterations, exact_dyadic=exact_dyadic)


def crafted(name):
    c = CRAFTED[name]()
    c.setdefault("cam", CAM)
    return c


# ---------------------------------------------------------------- the chain
def stereo_window(n=600, bsize=8, moving_share=0.3, noise=0.3, seed=700):
    """The script's block xy_t (n, 4, bsize) = left x, y, right x, y per frame, made from geometry alone: points in front
    of the first left camera, a camera path that moves on every frame, the right camera BASELINE beside the left one.
    The last share of the points, shuffled, is displaced by 30 px in every later frame, in a direction drawn per frame
    and camera. Returns (xy_t, moving (n,), G (bsize, 3, 4) the true left poses)."""
    rng = np.random.default_rng(seed)
    X = points(n, rng)
    moving = np.zeros(n, bool)
    moving[rng.permutation(n)[:int(round(moving_share * n))]] = True
    xy_t, G = np.empty((n, 4, bsize)), np.empty((bsize, 3, 4))
    off = np.array([BASELINE, 0.0, 0.0])
    step_w, step_t = rng.normal(0, 0.01, 3), np.array([0.06, -0.02, 0.12]) + rng.normal(0, 0.01, 3)
    for f in range(bsize):
        R, t = rot(step_w * f), step_t * f
        G[f] = np.hstack([R, t[:, None]])
        for c, tc in ((0, t), (2, t + off)):
            p = project(X, R, tc)
            if f > 0:
                ang = rng.uniform(0, 2 * np.pi, n)
                p = p + moving * 30.0 * np.stack([np.cos(ang), np.sin(ang)])
            xy_t[:, c:c + 2, f] = (p + rng.normal(0, 1.0, (2, n)) * noise).T
    return xy_t, moving, G


def chain_host(xy_t):
    """pairs_from_stereo_tracks -> split_static_host -> depth_from_disparity -> fit_cameras_host on the inliers -> both
    reprojection means."""
    from invcompcamtrack_amd import camfit as F
    from invcompcamtrack_amd import fsplit as S
    pairs, rows = S.pairs_from_stereo_tracks(xy_t)
    split = S.split_static_host(pairs)
    xy = xy_t[rows]
    X = F.points_from_first_view(xy, CAM, F.depth_from_disparity(xy, FC[0], BASELINE))
    left, right = F.observations_from_stereo_tracks(xy)
    fit = F.fit_cameras_host(X, left, CAM, mask=split["words"])
    return split, X, left, right, fit
