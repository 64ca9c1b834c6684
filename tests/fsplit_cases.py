"""Inputs of the static-split tests: seeded two-camera scenes and crafted point sets that random scenes do not reach.
Every crafted set states, through `reaches`, the branch of the fit it is made for; test_fsplit_cpu.py asserts on the host
that it gets there."""
import numpy as np

FC, CC = 1000.0, (640.0, 360.0)


def _rot(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = np.asarray(w) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _project(X, R, t):
    Xc = R @ X + t[:, None]
    assert (Xc[2] > 0.5).all()
    return np.stack([FC * Xc[0] / Xc[2] + CC[0], FC * Xc[1] / Xc[2] + CC[1]])


def scene(n, npairs=1, static=1.0, noise=0.0, seed=0):
    """pairs (npairs, 4, n) f64 and moving (n,) bool. Camera a is the world frame, every pair has its own camera b; the
    points lie in front of both. The last round((1 - static) n) points, shuffled, move: displaced by 30 px in image b,
    in a direction drawn per pair."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(4.0, 20.0, n)
    X = np.stack([rng.uniform(-0.55, 0.55, n) * z, rng.uniform(-0.3, 0.3, n) * z, z])
    moving = np.zeros(n, bool)
    moving[rng.permutation(n)[:int(round((1.0 - static) * n))]] = True
    pairs = np.empty((npairs, 4, n))
    xa = _project(X, np.eye(3), np.zeros(3))
    for p in range(npairs):
        R = _rot(rng.normal(0, 0.03, 3))
        t = rng.normal(0, 0.4, 3) + np.array([0.6, 0.0, 0.0]) * (1 if p % 2 == 0 else -1)
        xb = _project(X, R, t)
        ang = rng.uniform(0, 2 * np.pi, n)
        xb = xb + moving * 30.0 * np.stack([np.cos(ang), np.sin(ang)])
        pairs[p, 0:2] = xa + rng.normal(0, 1.0, (2, n)) * noise
        pairs[p, 2:4] = xb + rng.normal(0, 1.0, (2, n)) * noise
    return pairs, moving


SCENES = [(static, noise) for noise in (0.0, 0.3) for static in (1.0, 0.7, 0.5)]


def coincident():
    """N = 8, every point the same in image a: the mean distance of the sample is 0 in every trial."""
    pairs, _ = scene(8, 2, seed=31)
    pairs[:, 0, :] = 100.0
    pairs[:, 1, :] = 50.0
    return pairs, "mean distance 0"


def duplicate():
    """N = 8 with point 7 a copy of point 0: two equal rows of the design matrix, whatever is drawn; elimination
    subtracts equal values (factor exactly 1), so the last pivot is exactly 0."""
    pairs, _ = scene(8, 2, seed=32)
    pairs[:, :, 7] = pairs[:, :, 0]
    return pairs, "zero pivot"


def nan_drawn():
    """N = 8: every trial draws the point with the NaN."""
    pairs, _ = scene(8, 1, seed=33)
    pairs[0, 2, 3] = np.nan
    return pairs, "non-finite F"


def nan_not_drawn(seed, trial):
    """N = 200 with a NaN (and an infinite) coordinate in two points that `trial` of `seed` does not draw: the trial
    stays valid, the two points are never inliers."""
    from invcompcamtrack_amd.fsplit import draw_indices_n
    pairs, _ = scene(200, 2, seed=34)
    drawn = set(draw_indices_n(seed, trial, 200, 8))
    free = [i for i in range(200) if i not in drawn]
    pairs[1, 0, free[0]] = np.nan
    pairs[0, 3, free[1]] = np.inf
    return pairs, (free[0], free[1])


def fronto_parallel():
    """Dyadic points of a plane parallel to both image planes, camera b shifted along x: image b is image a moved by
    exactly 16 px. The design matrix is rank-deficient (every F = [e]x H of the plane's homography fits), its entries
    exact in f64."""
    g = np.array([(x, y) for y in (-96.0, -32.0, 32.0, 96.0) for x in (-128.0, -64.0, 0.0, 64.0, 128.0)]).T
    pairs = np.empty((1, 4, g.shape[1]))
    pairs[0, 0], pairs[0, 1] = g[0] + 640.0, g[1] + 360.0
    pairs[0, 2], pairs[0, 3] = g[0] + 656.0, g[1] + 360.0
    return pairs, "rank-deficient design"


def tie():
    """Every point static and noise-free, a generous threshold: every valid trial counts all N points, the lowest trial
    index must win."""
    pairs, _ = scene(120, 2, seed=35)
    return pairs, 50.0



def _plane_coords(w, h, fc, cc, G_ref, G_k, depth):
    """Per pixel of the frame seen through pose G_k: the reference-frame pixel (ua, va) of the point it sees on the plane
    Z = depth of the reference camera (the ray / plane intersection of synth._render)."""
    Ra, ta, Rb, tb = G_ref[:, :3], G_ref[:, 3], G_k[:, :3], G_k[:, 3]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    R = Rb @ Ra.T
    t = tb - R @ ta
    rx, ry = (xx - cc[0]) / fc[0], (yy - cc[1]) / fc[1]
    n = R[:, 2]
    lam = (depth + n @ t) / (n[0] * rx + n[1] * ry + n[2])
    XA = R.T @ (np.stack([lam * rx, lam * ry, lam], 0).reshape(3, -1) - t[:, None])
    return (XA[0] / XA[2] * fc[0] + cc[0]).reshape(h, w), (XA[1] / XA[2] * fc[1] + cc[1]).reshape(h, w)


def moving_patch_sequence(w=320, h=240, nframes=8, size=72, near_depth=4.0, x_cut=120.0, rot_deg=4.0, speed=2.5):
    """A rendered sequence with depth and a moving patch, for the chain PointTracker -> pairs_from_tracks -> split.

    Two textured planes parallel to camera 0's image plane: a far one (depth 10) and, where its reference-frame pixel
    column is below x_cut, a near one (near_depth) in front of it, so the static scene has parallax and pins the
    epipolar geometry. (On a single plane a translating patch is a second plane of a rigid scene: one F fits both.) On
    top a square patch of a third texture moves across the epipolar lines by `speed` px per frame and turns by rot_deg
    per frame about its centre. Returns (frames, info): info = dict(centres (nframes, 2), size, x_cut)."""
    from invcompcamtrack_amd import synth
    step = np.array([0.05, -0.03, 0.04, 0.005, -0.004, 0.0075])
    base = np.array([0.3, -0.2, 0.5, 0.02, -0.03, 0.01])
    Gs = [synth.se3_exp(base + k * step) for k in range(nframes)]
    fc = np.array([1000.0, 1200.0]) * (w / 1280.0)
    cc = np.array([20.0, 30.0]) * (w / 1280.0) + np.array([w, h]) / 2.0
    tex_far, tex_near, tex_patch = synth.texture(1234), synth.texture(77), synth.texture(1003)
    c0 = np.array([0.68 * w, 0.5 * h])
    epi = cc + fc * step[:2] / step[2]             # where a pure translation along `step` would put the epipole
    along = (epi - c0) / np.hypot(*(epi - c0))
    vel = speed * np.array([-along[1], along[0]])  # across the lines through it
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    frames, centres = [], []
    for k, G in enumerate(Gs):
        f = tex_far(*_plane_coords(w, h, fc, cc, Gs[0], G, 10.0))
        if near_depth is not None:
            ua, va = _plane_coords(w, h, fc, cc, Gs[0], G, near_depth)
            f = np.where(ua < x_cut, tex_near(ua, va), f)
        c = c0 + (k - (nframes - 1) / 2.0) * vel
        a = np.deg2rad(rot_deg) * k
        lx = np.cos(a) * (xx - c[0]) + np.sin(a) * (yy - c[1])
        ly = -np.sin(a) * (xx - c[0]) + np.cos(a) * (yy - c[1])
        inside = (np.abs(lx) < size / 2.0) & (np.abs(ly) < size / 2.0)
        f = np.where(inside, tex_patch(3.0 * lx + 200.0, 3.0 * ly + 300.0), f)
        frames.append(np.round(f).astype(np.float32))
        centres.append(c)
    return frames, dict(centres=np.array(centres), size=float(size), x_cut=float(x_cut))


def patch_truth(xy0, info, margin=10.0):
    """(moving, static) masks of frame-0 positions xy0 (K, 2). Moving: inside the patch of frame 0 by `margin`. Static:
    outside, by `margin`, of every circle that holds the patch during the window, and 30 px away from the column where
    the near plane ends (its edge moves by the parallax during the window). What straddles is in neither."""
    c, half = info["centres"], info["size"] / 2.0
    d0 = np.abs(xy0 - c[0])
    moving = (d0[:, 0] <= half - margin) & (d0[:, 1] <= half - margin)
    static = np.abs(xy0[:, 0] - info["x_cut"]) >= 30.0
    for ck in c:
        static &= np.hypot(xy0[:, 0] - ck[0], xy0[:, 1] - ck[1]) >= half * np.sqrt(2.0) + margin
    return moving, static
