"""Multi-view point triangulation on the device (ictr_triang_*, csrc/ictr_triang.hip): the reference's
misc_src/triang.c for a whole track set at once, and its Python callers' names (misc_src/func_util_geom.py:538-606,
609-812) on the single-point entry points.

Modes: "dlt" (triangulate_DLT), "gn" (triangulate_full3D), "lm" (triangulate_full3D_LM), "depth"
(triangulate_depthonly). Every mode computes in f32 with the reference's order of operations: the results carry the
bits of the reference binary (tests/golden/triang_golden.npz).

Tracks are a ragged list: point i owns observations offsets[i] .. offsets[i+1]-1 of view[] (camera index) and xy[].
Cameras are a table P [F, 12] (row-major 3x4, f32). What a pose is here: se(3) coefficients p with [R | t] = exp(p),
x_cam = R X + t (the tracker's convention), so P = K [R | t] and the camera centre is -R^T t.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._hostmath import se3_exp_d as _se3_exp
from ._lib import check, dp, f32c, f64c, fp

__all__ = ["Triangulator", "triangulate_tracks", "cameras_from_poses", "rays_from_first_view", "tracks_from_oftrack",
           "func_get_P_from_KRt", "func_pt_triangulate_from_P_linear_sq", "func_pt_triangulate_from_P_nonlin_LM",
           "MODES", "STATUS_NONFINITE", "STATUS_BEHIND"]

MODES = {"dlt": 0, "gn": 1, "lm": 2, "depth": 3}
STATUS_NONFINITE, STATUS_BEHIND = 1, 2
_I32P, _I64P = C.POINTER(C.c_int32), C.POINTER(C.c_int64)


def _fc_cc(cam):
    fc = cam["fc"] if isinstance(cam, dict) else cam.fc
    cc = cam["cc"] if isinstance(cam, dict) else cam.cc
    fc = np.asarray(fc, np.float64).reshape(-1)
    fc = np.array([fc[0], fc[0]]) if fc.size == 1 else fc[:2]
    return fc, np.asarray(cc, np.float64).reshape(-1)[:2]


def _P_from_KG(fc, cc, R, t):
    """K [R | t] in f64, written out entry by entry (K's zeros skipped), so that every caller forms the same bits."""
    G = np.concatenate([np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3, 1)], 1)
    return np.stack([fc[0] * G[0] + cc[0] * G[2], fc[1] * G[1] + cc[1] * G[2], G[2]], 0)


def _rot_vec(R, v, transpose=False):
    R = np.asarray(R, np.float64).reshape(3, 3)
    if transpose:
        R = R.T
    return np.array([(R[i, 0] * v[0] + R[i, 1] * v[1]) + R[i, 2] * v[2] for i in range(3)])


def cameras_from_poses(cam, poses):
    """se(3) coefficients [F, 6] -> camera table [F, 12] f32: K [R | t] formed in f64 and narrowed once (as the
    reference's callers narrow Plin). cam: dict or object with fc, cc."""
    fc, cc = _fc_cc(cam)
    poses = np.asarray(poses, np.float64).reshape(-1, 6)
    out = np.empty((len(poses), 12), np.float32)
    for i, p in enumerate(poses):
        G = _se3_exp(p)
        out[i] = _P_from_KG(fc, cc, G[:, :3], G[:, 3]).reshape(-1)
    return out


def _ray(fc, cc, R, xy):
    """Unit ray through pixel xy of a camera with rotation R, in world coordinates (func_util_geom.py:800-803), f64."""
    d = np.array([(float(xy[0]) - cc[0]) / fc[0], (float(xy[1]) - cc[1]) / fc[1], 1.0])
    d = d / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    return _rot_vec(R, d, transpose=True)


def rays_from_first_view(cam, poses, offsets, view, xy):
    """Per point the centre of its first view's camera and the unit ray through its first observation: f64, narrowed.
    Returns campos [n, 3], ptdir [n, 3] (f32), the depth-only mode's inputs."""
    fc, cc = _fc_cc(cam)
    poses = np.asarray(poses, np.float64).reshape(-1, 6)
    off = np.asarray(offsets, np.int64)
    view = np.asarray(view, np.int64)
    xy = np.asarray(xy).reshape(-1, 2)
    v0 = view[off[:-1]]
    R = np.zeros((len(poses), 3, 3))
    c = np.zeros((len(poses), 3))
    for v in np.unique(v0):
        G = _se3_exp(poses[v])
        R[v], c[v] = G[:, :3], -_rot_vec(G[:, :3], G[:, 3], transpose=True)
    # _ray for all points at once, the same operations in the same order
    x0 = xy[off[:-1]].astype(np.float64)
    d = np.stack([(x0[:, 0] - cc[0]) / fc[0], (x0[:, 1] - cc[1]) / fc[1], np.ones(len(v0))], 1)
    d = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
    Rv = R[v0]
    ptdir = np.stack([(Rv[:, 0, i] * d[:, 0] + Rv[:, 1, i] * d[:, 1]) + Rv[:, 2, i] * d[:, 2] for i in range(3)], 1)
    return c[v0].astype(np.float32), ptdir.astype(np.float32)


def tracks_from_oftrack(oftrack_obj, min_views=2, first_frame=0):
    """The sliding-window tracker's blocks -> the ragged list. Block b of ``oftrack_obj.tracks`` ([K, 2, bsize], opened
    at frame b) holds in column c the position in frame b + c, NaN from the frame on where the track was lost. A track
    contributes its leading finite columns when there are at least min_views of them. first_frame is added to every
    view index. Returns offsets [n + 1] i64, view [M] i32, xy [M, 2] f32 and origin [n, 2] (block, row) of each track."""
    offs, views, xys, origin = [0], [], [], []
    for b, blk in enumerate(oftrack_obj.tracks):
        if blk is None:
            continue
        blk = np.asarray(blk)
        ok = np.isfinite(blk).all(1)                    # [K, bsize]
        nlead = np.where(ok.all(1), ok.shape[1], np.argmin(ok, 1))
        for k in np.nonzero(nlead >= max(2, int(min_views)))[0]:
            L = int(nlead[k])
            views.append(np.arange(b, b + L, dtype=np.int32) + int(first_frame))
            xys.append(blk[k, :, :L].T.astype(np.float32))
            offs.append(offs[-1] + L)
            origin.append((b, int(k)))
    view = np.concatenate(views) if views else np.zeros(0, np.int32)
    xy = np.concatenate(xys) if xys else np.zeros((0, 2), np.float32)
    return np.asarray(offs, np.int64), view.astype(np.int32), xy, np.asarray(origin, np.int64).reshape(-1, 2)


class Triangulator:
    """One ictr_triang object: up to max_points tracks with max_obs observations in all over max_frames cameras."""

    def __init__(self, max_points, max_obs, max_frames):
        self._h = C.c_void_p()
        check(_lib.load().ictr_triang_create(C.byref(self._h), int(max_points), int(max_obs), int(max_frames)))
        self.n = 0

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.load().ictr_triang_destroy(self._h)
            self._h = None

    def set_cameras(self, P):
        P = f32c(P).reshape(-1, 12)
        check(_lib.load().ictr_triang_set_cameras(self._h, fp(P), P.shape[0]))

    def set_tracks(self, offsets, view, xy):
        """xy: [M, 2], or a pair (x, y) of [M] arrays."""
        off = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        view = np.ascontiguousarray(view, np.int32).reshape(-1)
        if isinstance(xy, (tuple, list)) and len(xy) == 2:
            x, y = f32c(xy[0]).reshape(-1), f32c(xy[1]).reshape(-1)
        else:
            xy = np.asarray(xy, np.float32).reshape(-1, 2)
            x, y = f32c(xy[:, 0]), f32c(xy[:, 1])
        if off.size < 2:
            raise ValueError("offsets needs n + 1 >= 2 entries")
        if not (view.size == x.size == y.size) or view.size < int(off[-1]):
            raise ValueError(f"{view.size} views, {x.size} x, {y.size} y for offsets that end at {int(off[-1])}")
        check(_lib.load().ictr_triang_set_tracks(self._h, off.size - 1, off.ctypes.data_as(_I64P),
                                                 view.ctypes.data_as(_I32P), fp(x), fp(y)))
        self.n = off.size - 1

    def run_async(self, mode="dlt", noiter=10, minres=1e-5, damp_init=2.0, damp_fct=10.0, maxdamp=1e10, init=None,
                  campos=None, ptdir=None, stream=None):
        if mode not in MODES:
            raise ValueError(f"mode {mode!r}: one of {sorted(MODES)}")
        prm = _lib.TriangParams(int(noiter), float(minres), float(damp_init), float(damp_fct), float(maxdamp))

        def arr(a, what):
            if a is None:
                return None
            a = f32c(a).reshape(-1, 3)
            if a.shape[0] != self.n:
                raise ValueError(f"{what}: {a.shape[0]} rows for {self.n} points")
            return a

        init, campos, ptdir = arr(init, "init"), arr(campos, "campos"), arr(ptdir, "ptdir")
        ptr = lambda a: fp(a) if a is not None else None  # noqa: E731
        sp = getattr(stream, "cuda_stream", stream)
        check(_lib.load().ictr_triang_run(self._h, MODES[mode], C.byref(prm), ptr(init), ptr(campos), ptr(ptdir),
                                          C.c_void_p(sp or 0)))
        self._mode = mode

    def wait(self):
        n = self.n
        pts, cov = np.zeros((n, 3), np.float32), np.zeros((n, 9), np.float32)
        iters, status = np.zeros(n, np.int32), np.zeros(n, np.int32)
        check(_lib.load().ictr_triang_wait(self._h, fp(pts), fp(cov), iters.ctypes.data_as(_I32P),
                                           status.ctypes.data_as(_I32P)))
        return dict(pts=pts, cov=cov[:, 0].copy() if self._mode == "depth" else cov.reshape(n, 3, 3), iters=iters,
                    status=status)


def triangulate_tracks(P, offsets, view, xy, mode="dlt", noiter=10, minres=1e-5, damp_init=2.0, damp_fct=10.0,
                       maxdamp=1e10, init=None, campos=None, ptdir=None, stream=None):
    """All tracks in one launch. Returns dict: pts [n, 3] f32, cov [n, 3, 3] (depth: [n], the scalar), iters [n],
    status [n] (STATUS_NONFINITE | STATUS_BEHIND). init=None in an iterative mode: a DLT run first, on the same stream.
    The depth-only mode needs campos and ptdir (rays_from_first_view)."""
    P = f32c(P).reshape(-1, 12)
    off = np.asarray(offsets, np.int64).reshape(-1)
    if mode not in MODES:
        raise ValueError(f"mode {mode!r}: one of {sorted(MODES)}")
    t = Triangulator(max(1, off.size - 1), max(2 * (off.size - 1), int(off[-1]) if off.size else 2), P.shape[0])
    t.set_cameras(P)
    t.set_tracks(off, view, xy)
    if mode != "dlt" and init is None:
        t.run_async("dlt", stream=stream)
        init = t.wait()["pts"]
    t.run_async(mode, noiter, minres, damp_init, damp_fct, maxdamp, init, campos, ptdir, stream)
    return t.wait()


# ---------------------------------------------------------------- the reference callers' names (func_util_geom.py)
def func_get_P_from_KRt(fc, cc, R, tw):
    """K [-R | R tw] (f64 3x4): the reference's camera matrix of a camera with rotation R at the world position tw (its
    sign is the reference's; as a projection it equals K [R | -R tw])."""
    fc, cc = np.asarray(fc, np.float64).reshape(-1), np.asarray(cc, np.float64).reshape(-1)
    R = np.asarray(R, np.float64).reshape(3, 3)
    return _P_from_KG(fc, cc, -R, _rot_vec(R, np.asarray(tw, np.float64).reshape(-1)))


def _single_inputs(fc, cc, R_l, tw_l, x_l):
    if not (len(R_l) == len(tw_l) == len(x_l)):
        raise ValueError("R_l, tw_l and x_l must have one entry per view")
    pt2d = np.ascontiguousarray(np.stack([np.asarray(x, np.float64).reshape(-1)[:2] for x in x_l], 1), np.float32)
    Plin = np.stack([func_get_P_from_KRt(fc, cc, R_l[i], tw_l[i]).reshape(-1) for i in range(len(R_l))])
    return pt2d, np.ascontiguousarray(Plin.astype(np.float32).T)


def func_pt_triangulate_from_P_linear_sq(fc, cc, R_l, tw_l, x_l, use_c_interf=True):
    """Linear triangulation of one point (func_util_geom.py:565-606, the C-interface branch) through
    ictr_triangulate_DLT. Returns (pt3d [3], cov [3, 3]) f32. There is no NumPy branch here."""
    if not use_c_interf:
        raise ValueError("only the native path exists here (use_c_interf=True); there is no CPU fallback")
    pt2d, Plin = _single_inputs(fc, cc, R_l, tw_l, x_l)
    pt, cov = np.zeros(3, np.float32), np.zeros((3, 3), np.float32)
    check(_lib.load().ictr_triangulate_DLT(fp(pt), fp(cov), fp(pt2d), fp(Plin), len(x_l)))
    return pt, cov


def func_pt_triangulate_from_P_nonlin_LM(pt3dinit, fc, cc, R_l, tw_l, x_l, noiter=10, mswitch=1, lamb_damp_init=2.0,
                                         lamp_damp_fact=10.0, minres=1e-5, verbose=0, use_c_interf=True):
    """Non-linear refinement of one point (func_util_geom.py:609-812, the C-interface branch): mswitch 0 the full 3-D
    Levenberg-Marquardt (maxdamp 1e10), otherwise the depth along the first view's ray. Returns pt3d [3] f32."""
    if not use_c_interf:
        raise ValueError("only the native path exists here (use_c_interf=True); there is no CPU fallback")
    pt2d, Plin = _single_inputs(fc, cc, R_l, tw_l, x_l)
    pt = np.array(np.asarray(pt3dinit).reshape(-1)[:3], np.float32)
    L = _lib.load()
    if mswitch == 0:
        cov = np.zeros(9, np.float32)
        check(L.ictr_triangulate_full3D_LM(fp(pt), fp(cov), fp(pt2d), fp(Plin), len(x_l), int(noiter),
                                           float(lamb_damp_init), float(lamp_damp_fact), float(minres), 1e10))
    else:
        fcv, ccv = np.asarray(fc, np.float64).reshape(-1), np.asarray(cc, np.float64).reshape(-1)
        ptdir = f32c(_ray(fcv, ccv, R_l[0], np.asarray(x_l[0]).reshape(-1)))
        campos = f32c(np.asarray(tw_l[0], np.float64).reshape(-1)[:3])
        cov = np.zeros(1, np.float32)
        check(L.ictr_triangulate_depthonly(fp(pt), fp(cov), fp(campos), fp(ptdir), fp(pt2d), fp(Plin), len(x_l),
                                           int(noiter), float(minres)))
    return pt
