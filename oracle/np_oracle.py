"""Independent NumPy-float32 restatement of the reference tracker.

TEST INFRASTRUCTURE ONLY (same rules as oracle.py). Written from the reference's formulas without looking at
ictr_oracle.c's structure: vectorised over points and patch pixels, no materialised sd planes. Used to
cross-check the C oracle: element-wise quantities (projections, patches, coefficients) must agree bit for
bit, sums to float tolerance. Restates visibility (points outside the reference or the new view), patch
normalisation and the loop rule for a FIRST frame pair; the stale-patch quirk across frame pairs stays with the C oracle.
track is made of new_state, level_setup and iteration, which tests/iter_judge.py calls on their own to judge a traced
run at its own poses.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32


def exp_se3(p, dtype=np.float32):
    """utilities.h:84-145."""
    p = np.asarray(p, dtype)
    one = dtype(1)
    w = p[3:]
    q = w * w
    sig = np.sqrt(q[0] + q[1] + q[2], dtype=dtype)
    s2, s3 = sig * sig, sig * sig * sig
    if sig > 1e-4:
        sa = np.sin(sig, dtype=dtype) / sig
        sb = (one - np.cos(sig, dtype=dtype)) / s2
        sc = (sig - np.sin(sig, dtype=dtype)) / s3
    else:
        sa = one - s2 / dtype(6) * (one - s2 / dtype(20) * (one - s2 / dtype(42)))
        sb = dtype(0.5) * (one - s2 / dtype(12) * (one - s2 / dtype(30) * (one - s2 / dtype(56))))
        sc = (one - s2 / dtype(20) * (one - s2 / dtype(42) * (one - s2 / dtype(72)))) / dtype(6)
    G = np.zeros(12, dtype)
    G[0] = one - q[1] * sb - q[2] * sb
    G[1] = w[0] * w[1] * sb - w[2] * sa
    G[2] = w[1] * sa + w[0] * w[2] * sb
    G[4] = w[2] * sa + w[0] * w[1] * sb
    G[5] = one - q[0] * sb - q[2] * sb
    G[6] = w[1] * w[2] * sb - w[0] * sa
    G[8] = w[0] * w[2] * sb - w[1] * sa
    G[9] = w[0] * sa + w[1] * w[2] * sb
    G[10] = one - q[0] * sb - q[1] * sb
    t1, t2, t3 = w[2] * sb, w[0] * w[1] * sc, w[1] * sb
    t4, t5, t6 = w[0] * w[2] * sc, w[0] * sb, w[1] * w[2] * sc
    G[3] = (one - (q[1] + q[2]) * sc) * p[0] + (t2 - t1) * p[1] + (t3 + t4) * p[2]
    G[7] = (t1 + t2) * p[0] + (one - (q[0] + q[2]) * sc) * p[1] + (t6 - t5) * p[2]
    G[11] = (t4 - t3) * p[0] + (t5 + t6) * p[1] + (one - (q[0] + q[1]) * sc) * p[2]
    return G


def project(G, X, Y, Z, fx, fy, cx, cy):
    """pose.cpp:384-391, float32, left-to-right sums."""
    tx = ((G[0] * X + G[1] * Y) + G[2] * Z) + G[3]
    ty = ((G[4] * X + G[5] * Y) + G[6] * Z) + G[7]
    tz = ((G[8] * X + G[9] * Y) + G[10] * Z) + G[11]
    return (tx / tz) * fx + cx, (ty / tz) * fy + cy, tx, ty, tz


def patches(plane, mx, my, psz):
    """utilities.cpp:55-113 for K centres at once: returns (K, psz, psz) float32."""
    mx, my = mx.astype(f32), my.astype(f32)
    p0 = np.ceil(mx + f32(.00001)).astype(np.int64)
    p1 = np.ceil(my + f32(.00001)).astype(np.int64)
    r0 = mx - np.floor(mx)
    r1 = my - np.floor(my)
    w = [r0 * r1, (f32(1) - r0) * r1, r0 * (f32(1) - r1), (f32(1) - r0) * (f32(1) - r1)]
    ii = np.arange(psz)
    col = (p0 + psz // 2)[:, None, None] + ii[None, None, :]
    row = (p1 + psz // 2)[:, None, None] + ii[None, :, None]
    a, b, c, d = plane[row, col], plane[row, col - 1], plane[row - 1, col], plane[row - 1, col - 1]
    wv = [x[:, None, None] for x in w]
    return ((wv[0] * a + wv[1] * b) + wv[2] * c) + wv[3] * d


def sd_coefs(X, Y, Z, fx, fy):
    """odometer.cpp:313-326; (K,6) x-coefficients and y-coefficients, the '1.0 +' terms in float64."""
    zsq = Z * Z
    cx = np.zeros((len(X), 6), f32)
    cy = np.zeros((len(X), 6), f32)
    cx[:, 0] = fx / Z
    cy[:, 1] = fy / Z
    cx[:, 2] = -X / zsq * fx
    cy[:, 2] = -Y / zsq * fy
    cx[:, 3] = -X * Y / zsq * fx
    cy[:, 3] = ((-(1.0 + (Y * Y / zsq).astype(np.float64))) * np.float64(fy)).astype(f32)
    cx[:, 4] = ((1.0 + (X * X / zsq).astype(np.float64)) * np.float64(fx)).astype(f32)
    cy[:, 4] = X * Y / zsq * fy
    cx[:, 5] = -Y / Z * fx
    cy[:, 5] = X / Z * fy
    return cx, cy


def in_view(mx, my, swo, sho):
    """odometer.cpp:273-276, 369-377: inclusive bounds; NaN is outside."""
    with np.errstate(invalid="ignore"):
        return (mx >= 0) & (my >= 0) & (mx <= swo) & (my <= sho)


def normdp32(dp):
    """delta_p.lpNorm<1>() in Eigen's redux order for 6 coefficients, f32."""
    d = np.abs(np.asarray(dp, f32))
    with np.errstate(all="ignore"):
        return f32(f32(d[0] + f32(d[1] + d[2])) + f32(d[3] + f32(d[4] + d[5])))


def _patchnorm(pat):
    """utilities.cpp:111-112, 187-188: the patch mean, summed and divided in f32, taken off the intensity patch."""
    n = pat.shape[1] * pat.shape[2]
    mean = pat.reshape(len(pat), -1).sum(1, dtype=f32) / f32(n)
    return pat - mean[:, None, None]


def new_state(pts3d, G0, psz):
    """What Set3Dpoints and SetPose leave: the points (f32), the points rotated by G0, zeroed T/Gx/Gy patches and
    coefficient lines. level_setup updates the buffers in place."""
    X, Y, Z = (np.asarray(pts3d[k]).astype(f32) for k in range(3))
    K = len(X)
    _, _, Xc, Yc, Zc = project(G0, X, Y, Z, f32(1), f32(1), f32(0), f32(0))
    T, Gx, Gy = (np.zeros((K, psz, psz), f32) for _ in range(3))
    return dict(X=X, Y=Y, Z=Z, Xc=Xc, Yc=Yc, Zc=Zc, T=T, Gx=Gx, Gy=Gy, cx=np.zeros((K, 6), f32), cy=np.zeros((K, 6), f32))


def level_setup(st, G0, sl, pyr_ref, cam, psz, *, dopatchnorm=False, clean_invisible=False):
    """The setup of level sl (odometer.cpp:263-335) on the buffers of `st`: fresh T/Gx/Gy and coefficient lines for the
    points in the reference view, the sd planes of all points. Returns dict(fx, fy, cx, cy, swo, sho: the level's camera;
    mx, my, vis_ref; sd (K,6,P,P) f32)."""
    T, Gx, Gy, cxk, cyk = st["T"], st["Gx"], st["Gy"], st["cx"], st["cy"]
    fx, fy, cx_, cy_ = (f32(cam(k, sl)) for k in range(4))
    swo, sho = f32(cam(4, sl)), f32(cam(5, sl))
    mx, my, _, _, _ = project(G0, st["X"], st["Y"], st["Z"], fx, fy, cx_, cy_)
    vr = in_view(mx, my, swo, sho)
    t_new = patches(pyr_ref.img[sl], mx[vr], my[vr], psz)
    T[vr] = _patchnorm(t_new) if dopatchnorm else t_new
    Gx[vr] = patches(pyr_ref.dx[sl], mx[vr], my[vr], psz)
    Gy[vr] = patches(pyr_ref.dy[sl], mx[vr], my[vr], psz)
    cxk[vr], cyk[vr] = sd_coefs(st["Xc"][vr], st["Yc"][vr], st["Zc"][vr], fx, fy)
    if clean_invisible:
        Gx[~vr] = 0
        Gy[~vr] = 0
    sd = Gx[:, None] * cxk[:, :, None, None] + Gy[:, None] * cyk[:, :, None, None]  # (K,6,P,P)
    sd[:, 0] = Gx * cxk[:, 0, None, None]
    sd[:, 1] = Gy * cyk[:, 1, None, None]
    return dict(fx=fx, fy=fy, cx=cx_, cy=cy_, swo=swo, sho=sho, mx=mx, my=my, vis_ref=vr, sd=sd)


def iteration(st, lev, G, sl, pyr_new, psz, *, dopatchnorm=False, huber_k=0.0):
    """One iteration's per-pixel part at the pose G (odometer.cpp:360-404): the points in the new view and their
    residuals r = T - I, weighted where huber_k > 0. Returns dict(nx, ny, vis_new, r (points in view, P, P), over)."""
    nx, ny, _, _, _ = project(G, st["X"], st["Y"], st["Z"], lev["fx"], lev["fy"], lev["cx"], lev["cy"])
    vn = in_view(nx, ny, lev["swo"], lev["sho"])
    I = patches(pyr_new.img[sl], nx[vn], ny[vn], psz)
    if dopatchnorm:
        I = _patchnorm(I)
    r = st["T"][vn] - I
    over = float(np.mean(np.abs(r) > f32(huber_k))) if huber_k > 0 and r.size else 0.0
    if huber_k > 0:
        ar = np.abs(r)
        r = np.where(ar > f32(huber_k), r * (f32(huber_k) / np.where(ar > 0, ar, f32(1))), r).astype(f32)
    return dict(nx=nx, ny=ny, vis_new=vn, r=r, over=over)


def track(pts3d, p_in, pyr_ref, pyr_new, cam, lv_f, lv_l, psz, maxiter, solve, compose=None, huber_k=0.0, *,
          clean_invisible=False, dopatchnorm=False, normdp_ratio=None, exp=None, detail=None):
    """No-normalisation TrackPose (odometer.cpp:257-426) of a FIRST frame pair after Set3Dpoints.
    pyr_*: object with .img/.dx/.dy lists of padded planes; cam(which, level) -> float (0..3 fx fy cx cy, 4 5 the
    unpadded level size swo sho); solve(H,b) -> dp.
    Returns (p float32[6], trace list of dict(level, iter, H, b, dp, p, vis_new, over)).
    Visibility (in_view): points outside the reference view at a level get no fresh T/Gx/Gy/coefficients -- they keep
    what the buffers hold, the zeros of Set3Dpoints or a coarser level's values (odometer.cpp:304) --, points outside the
    new view at an iteration do not enter b; the patches of neither are fetched. The stale state ACROSS frame pairs is
    not restated (the C oracle owns it).
    dopatchnorm: patch mean (f32) taken off T and I. normdp_ratio: None runs maxiter iterations per level; a number
    applies the loop rule of odometer.cpp:341-346 (iteration k + 1 iff k + 1 < maxiter and normdp_k / normdp_0 > ratio).
    exp: p float32[6] -> G float32[12], default exp_se3 (NumPy's sinf; a caller that wants the bits of another build's
    libm passes that build's exp map). detail: a dict that receives, per level, dict(vis_ref, mx, my, T, Gx, Gy, cx, cy).
    Options of the build's robustness extension (not reference behaviour): compose(p, dp) -> p_new replaces the
    additive update (the test passes log(exp(dp) exp(p))); huber_k > 0 weights residuals min(1, k/|r|) in b;
    clean_invisible zeroes Gx, Gy of the points outside the reference view at a level, so that they add nothing to H
    or b there."""
    exp = exp_se3 if exp is None else exp
    p = np.asarray(p_in, np.float64).astype(f32)
    G0 = np.asarray(exp(p), f32)
    trace = []
    st = new_state(pts3d, G0, psz)
    K = len(st["X"])
    for sl in range(lv_f, lv_l - 1, -1):
        lev = level_setup(st, G0, sl, pyr_ref, cam, psz, dopatchnorm=dopatchnorm, clean_invisible=clean_invisible)
        sd = lev["sd"]
        if detail is not None:
            detail[sl] = dict(vis_ref=lev["vis_ref"].copy(), mx=lev["mx"], my=lev["my"], T=st["T"].copy(),
                              Gx=st["Gx"].copy(), Gy=st["Gy"].copy(), cx=st["cx"].copy(), cy=st["cy"].copy())
        sdf = sd.reshape(K, 6, -1).astype(np.float64)
        H = np.einsum("kip,kjp->ij", sdf, sdf).astype(f32)
        it, nd, nd0 = 0, f32(1e-10), f32(1e-10)
        while it < maxiter:
            if normdp_ratio is not None:
                with np.errstate(all="ignore"):
                    if not f32(nd / nd0) > f32(normdp_ratio):
                        break
            cur = iteration(st, lev, np.asarray(exp(p), f32), sl, pyr_new, psz, dopatchnorm=dopatchnorm, huber_k=huber_k)
            vn, r = cur["vis_new"], cur["r"]
            b = (sd[vn] * r[:, None]).reshape(int(vn.sum()), 6, -1).astype(np.float64).sum((0, 2)).astype(f32)
            dp = solve(H, b)
            p = (p + dp) if compose is None else np.asarray(compose(p, dp), f32)
            trace.append(dict(level=sl, iter=it, H=H, b=b, dp=dp, p=p.copy(), vis_new=vn, over=cur["over"]))
            nd = normdp32(dp)
            if it == 0:
                nd0 = nd
            it += 1
    return p, trace
