"""Inputs of the bundle-adjustment tests: seeded windows with known poses and points, and crafted inputs that random
windows do not reach. Every crafted case names the branch it is made for; test_bundle_cpu.py asserts on the host that it
gets there."""
import numpy as np

import camfit_cases as K

CAM = K.CAM
OFFSET = (K.BASELINE, 0.0, 0.0)   # P1[:, 3] of the script


def window(n, nframes, nsides, noise, seed, depth_err=0.03, pose_err=0.0):
    """A camera path that starts at the identity and moves on every frame, seen from nsides sides. Returns dict: X (the
    true points, in the first view's frame), G (the true poses), xy (S, F, 2, n), X0 (the points with a relative depth
    error drawn per point), G0 (the poses with a turn and a shift of size pose_err on every frame but the first)."""
    rng = np.random.default_rng(seed)
    X = K.points(n, rng)
    step_w, step_t = rng.normal(0, 0.01, 3), np.array([0.06, -0.02, 0.12]) + rng.normal(0, 0.01, 3)
    xy, G, G0 = np.empty((nsides, nframes, 2, n)), np.empty((nframes, 3, 4)), np.empty((nframes, 3, 4))
    for f in range(nframes):
        R, t = K.rot(step_w * f), step_t * f
        G[f] = np.hstack([R, t[:, None]])
        dR, dt = K.pose(pose_err, rng) if f and pose_err else (np.eye(3), np.zeros(3))
        G0[f] = np.hstack([dR @ R, (t + dt)[:, None]])
        for s in range(nsides):
            xy[s, f] = K.project(X, R, t + np.array(OFFSET) * s) + rng.normal(0, 1.0, (2, n)) * noise
    X0 = X * (1.0 + rng.normal(0, 1.0, n) * depth_err)
    return dict(X=X, G=G, xy=xy, X0=X0, G0=G0)


def spotted_mask(n, seed):
    """A mask with cleared bits on wave, row and chunk boundaries and a few drawn ones."""
    rng = np.random.default_rng(seed)
    mask = np.ones(n, bool)
    for m in (0, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, n - 1):
        if m < n:
            mask[m] = False
    mask[rng.integers(0, n, max(1, n // 11))] = False
    return mask


# ---------------------------------------------------------------- crafted: dict(X, xy, cam, offset, mask, init, schedule)
def _case(w, reaches, nsides, mask=None, X=None, xy=None, init=None, cam=CAM, **schedule):
    return dict(X=w["X0"] if X is None else X, xy=w["xy"] if xy is None else xy, cam=cam,
                offset=OFFSET if nsides == 2 else None, mask=mask, init=w["G0"] if init is None else init,
                schedule=schedule, reaches=reaches)


def all_masked():
    return _case(window(40, 3, 2, 0.3, 901), "fewer than 3 adjusted", 2, mask=np.zeros(40, bool))


def two_adjusted():
    mask = np.zeros(70, bool)
    mask[[7, 66]] = True
    return _case(window(70, 3, 2, 0.3, 902), "fewer than 3 adjusted", 2, mask=mask)


def nan_observation():
    """One coordinate of one side of one frame is NaN: the point leaves every frame."""
    w = window(130, 4, 2, 0.3, 903)
    xy = w["xy"].copy()
    xy[1, 2, 0, 64] = np.nan
    return _case(w, "n = N - 1", 2, xy=xy)


def depth_zero_at_start():
    w = window(80, 3, 2, 0.0, 904)
    X = w["X0"].copy()
    X[:, 5] = (1.0, 1.0, 0.0)
    return _case(w, "start cost not finite", 2, X=X)


def on_the_axis():
    """Every point on the optical axis of identity poses, one side: the third column of every point's Jacobian is exactly
    zero, so the third pivot of every 3 x 3 is exactly 0 at every damping."""
    z = np.array([2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 3.0, 5.0, 6.0, 7.0])
    X = np.stack([np.zeros(10), np.zeros(10), z])
    one = np.stack([np.full(10, K.CC[0] + 3.0), np.full(10, K.CC[1] - 2.0)])
    xy = np.tile(one[None, None], (1, 3, 1, 1))
    return dict(X=X, xy=xy, cam=CAM, offset=None, mask=None, init=K.identity(3), schedule={}, reaches="failed solve")


def far_start():
    """The start poses are a turn and a shift of 0.6 away from the true ones: some trial steps are rejected."""
    w = window(120, 3, 2, 0.0, 906, depth_err=0.1, pose_err=0.6)
    return _case(w, "a rejected step", 2, noiter=60)


def failed_between():
    """The same window from a turn and a shift of 1.0: on the way a point's 3 x 3 loses a pivot, and solves fail between
    accepted steps."""
    w = window(120, 3, 2, 0.0, 906, depth_err=0.1, pose_err=1.0)
    return _case(w, "failed solves between accepted steps", 2, noiter=60)


def no_iterations():
    return _case(window(50, 3, 2, 0.3, 907), "noiter = 0", 2, noiter=0)


def exact_dyadic():
    """Dyadic points, a power-of-two focal length and a dyadic offset seen from identity poses: every projection is exact,
    c = 0."""
    g = np.array([(x, y, z) for z in (2.0, 4.0, 8.0) for y in (-0.5, 0.25, 1.0) for x in (-1.0, -0.25, 0.5, 0.75)]).T
    xy = np.empty((2, 3, 2, g.shape[1]))
    for s in range(2):
        xy[s, :] = np.stack([1024.0 * (g[0] + OFFSET[0] * s) / g[2] + 640.0, 1024.0 * g[1] / g[2] + 360.0])[None]
    return dict(X=g, xy=xy, cam=((1024.0, 1024.0), K.CC), offset=OFFSET, mask=None, init=K.identity(3), schedule={},
                reaches="c = 0 at the start")


def one_side():
    return _case(window(90, 4, 1, 0.3, 909), "S = 1", 1)


def two_frames():
    return _case(window(100, 2, 2, 0.3, 910), "F = 2", 2)


CRAFTED = dict(all_masked=all_masked, two_adjusted=two_adjusted, nan_observation=nan_observation,
               depth_zero_at_start=depth_zero_at_start, on_the_axis=on_the_axis, far_start=far_start, failed_between=failed_between,
               no_iterations=no_iterations, exact_dyadic=exact_dyadic, one_side=one_side, two_frames=two_frames)


def crafted(name):
    return CRAFTED[name]()


def run_host(c, **kw):
    from invcompcamtrack_amd import bundle as B
    sched = dict(c["schedule"])
    sched.update(kw)
    return B.adjust_window_host(c["X"], c["xy"], c["cam"], offset=c["offset"], mask=c["mask"], init=c["init"], detail=True,
                                **sched)
