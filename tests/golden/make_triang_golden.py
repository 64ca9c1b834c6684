"""Generates tests/golden/triang_golden.npz by running the REFERENCE's misc_src/triang.c as a binary.

Run in the build container only (needs /root/reference and gcc): python tests/golden/make_triang_golden.py
The reference source is compiled into a temporary directory outside the repository and called through ctypes, point
by point, with file descriptor 1 redirected to a temporary file: the `Iter` lines it prints per call are counted, which
pins the iteration counts too. The .npz holds data only: seeded inputs and the binary's outputs.

Main group: 24 cameras on a drifting path, points seen in 2..12 consecutive views with 0.5 px noise; 4000 are run (all
must come back finite in every mode), the first 512 are stored. Second group: hand-made degenerate tracks, each with
its own start point and options, for the inf / NaN and early-exit behaviour.
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

REF = "/root/reference/misc_src/triang.c"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "triang_golden.npz")
F32 = np.float32
FP = C.POINTER(C.c_float)
FC, CC = (1000.0, 1200.0), (660.0, 390.0)
NOITER, MINRES, DAMP, FCT, MAXDAMP = 10, 1e-5, 2.0, 10.0, 1e10
N_RUN, N_KEEP = 4000, 512


def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def make_cameras(rng, nf):
    Ps, Rs, cs = [], [], []
    c = np.zeros(3)
    for i in range(nf):
        R = rodrigues(rng.normal(0, 0.03, 3))
        # K [R | -R c], entry by entry in f64 (no BLAS: the same bits wherever it is formed)
        t = -np.array([(R[r, 0] * c[0] + R[r, 1] * c[1]) + R[r, 2] * c[2] for r in range(3)])
        G = np.concatenate([R, t[:, None]], 1)
        Ps.append(np.stack([FC[0] * G[0] + CC[0] * G[2], FC[1] * G[1] + CC[1] * G[2], G[2]], 0).reshape(-1))
        Rs.append(R)
        cs.append(c.copy())
        d = np.array([1.0, 0.15 * np.sin(0.4 * i), 0.1 * np.cos(0.3 * i)])
        c = c + 0.25 * d / np.linalg.norm(d)
    return np.array(Ps), np.array(Rs), np.array(cs)


def make_tracks(rng, P64, n):
    nf = len(P64)
    X = np.stack([rng.uniform(-3, 8, n), rng.uniform(-2, 2, n), rng.uniform(8, 14, n)], 1)
    lens = rng.integers(2, 13, n)
    first = np.array([rng.integers(0, nf - l + 1) for l in lens])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    view = np.concatenate([np.arange(f, f + l) for f, l in zip(first, lens)]).astype(np.int32)
    Xr = np.repeat(X, lens, 0)
    h = np.einsum("mij,mj->mi", P64[view].reshape(-1, 3, 4), np.concatenate([Xr, np.ones((len(Xr), 1))], 1))
    xy = h[:, :2] / h[:, 2:3] + rng.normal(0, 0.5, (len(Xr), 2))
    return X, off, view, xy[:, 0].astype(F32), xy[:, 1].astype(F32)


def first_view_rays(Rs, cs, off, view, x, y):
    v0 = view[off[:-1]]
    d = np.stack([(x[off[:-1]].astype(np.float64) - CC[0]) / FC[0], (y[off[:-1]].astype(np.float64) - CC[1]) / FC[1],
                  np.ones(len(v0))], 1)
    d = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
    R = Rs[v0]
    w = np.stack([(R[:, 0, i] * d[:, 0] + R[:, 1, i] * d[:, 1]) + R[:, 2, i] * d[:, 2] for i in range(3)], 1)  # R^T d
    return cs[v0].astype(F32), w.astype(F32)


class Binary:
    def __init__(self, tmp):
        so = os.path.join(tmp, "libtriang.so")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-std=gnu99", "-shared", "-fPIC", REF, "-o", so, "-lm"])
        self.dll = C.CDLL(so)
        self.libc = C.CDLL(None)
        ll, f = C.c_longlong, C.c_float
        self.dll.triangulate_DLT.argtypes = [FP, FP, FP, FP, ll]
        self.dll.triangulate_full3D.argtypes = [FP, FP, FP, FP, ll, ll, f]
        self.dll.triangulate_full3D_LM.argtypes = [FP, FP, FP, FP, ll, ll, f, f, f, f]
        self.dll.triangulate_depthonly.argtypes = [FP, FP, FP, FP, FP, FP, ll, ll, f]
        for fn in (self.dll.triangulate_DLT, self.dll.triangulate_full3D, self.dll.triangulate_full3D_LM,
                   self.dll.triangulate_depthonly):
            fn.restype = None
        self.log = os.path.join(tmp, "stdout.txt")

    def counted(self, fn, *args):
        """Calls fn with fd 1 redirected to the log; returns the number of `Iter` lines it printed."""
        sys.stdout.flush()
        self.libc.fflush(None)
        keep = os.dup(1)
        fd = os.open(self.log, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o600)
        os.dup2(fd, 1)
        try:
            fn(*args)
            self.libc.fflush(None)
        finally:
            os.dup2(keep, 1)
            os.close(fd)
            os.close(keep)
        with open(self.log) as fh:
            return sum(1 for line in fh if line.startswith("Iter"))

    def point(self, mode, Pl, pt2d, init, campos, ptdir, noiter, minres, damp, fct, maxdamp):
        """One point: Pl [12][nv], pt2d [2][nv] (the binary's layouts). Returns point, cov[9], Iter lines."""
        nv = Pl.shape[1]
        pt = np.zeros(3, F32) if init is None else np.array(init, F32)
        cov = np.zeros(9, F32)
        a = lambda v: v.ctypes.data_as(FP)  # noqa: E731
        if mode == "dlt":
            it = self.counted(self.dll.triangulate_DLT, a(pt), a(cov), a(pt2d), a(Pl), nv)
        elif mode == "gn":
            it = self.counted(self.dll.triangulate_full3D, a(pt), a(cov), a(pt2d), a(Pl), nv, noiter, minres)
        elif mode == "lm":
            it = self.counted(self.dll.triangulate_full3D_LM, a(pt), a(cov), a(pt2d), a(Pl), nv, noiter, damp, fct,
                              minres, maxdamp)
        else:
            cp, pd = np.array(campos, F32), np.array(ptdir, F32)
            it = self.counted(self.dll.triangulate_depthonly, a(pt), a(cov), a(cp), a(pd), a(pt2d), a(Pl), nv, noiter,
                              minres)
        return pt, cov, it


def run_group(B, P32, off, view, x, y, init, campos, ptdir, opts):
    """Every mode on every track. init None: the iterative modes start from the DLT point. opts: per track
    (noiter, minres, damp_init, damp_fct, maxdamp)."""
    n = len(off) - 1
    res = {m: dict(pts=np.zeros((n, 3), F32), cov=np.zeros((n, 9), F32), iters=np.zeros(n, np.int32))
           for m in ("dlt", "gn", "lm", "depth")}
    for i in range(n):
        s = slice(off[i], off[i + 1])
        Pl = np.ascontiguousarray(P32[view[s]].T)
        pt2d = np.ascontiguousarray(np.stack([x[s], y[s]], 0))
        for m in ("dlt", "gn", "lm", "depth"):
            start = None if m == "dlt" else (res["dlt"]["pts"][i] if init is None else init[i])
            pt, cov, it = B.point(m, Pl, pt2d, start, campos[i], ptdir[i], *opts[i])
            res[m]["pts"][i], res[m]["cov"][i], res[m]["iters"][i] = pt, cov, it
    return res


def degenerate_group(P64, Rs, cs):
    """<= 16 hand-made tracks: (views, observations, start point, options)."""
    std = (NOITER, MINRES, DAMP, FCT, MAXDAMP)
    X = np.array([1.5, 0.3, 10.0])

    def obs(views, Xw=X):
        h = P64[views].reshape(-1, 3, 4) @ np.append(Xw, 1.0)
        return h[:, :2] / h[:, 2:3]

    T = []
    T.append(([3, 3], obs([3, 3]), X, std))                                  # two identical cameras
    T.append(([5, 5, 5], obs([5, 5, 5]) + [[0, 0], [0.5, -0.5], [1, 1]], X, std))  # three identical cameras, noisy
    o = obs([0, 1, 2, 3])
    o[0] = CC
    T.append(([0, 1, 2, 3], o, cs[0], std))                                  # start at a camera centre (w = 0)
    T.append(([2, 4, 6], obs([2, 4, 6]) + 0.3, X + 0.2, (0, MINRES, DAMP, FCT, MAXDAMP)))     # noiter 0
    T.append(([2, 4, 6], obs([2, 4, 6]) + 0.3, X + 0.2, (1, MINRES, DAMP, FCT, MAXDAMP)))     # noiter 1
    T.append(([1, 2, 3, 4], obs([1, 2, 3, 4]) - 0.4, X - 0.3, (NOITER, 1e6, DAMP, FCT, MAXDAMP)))   # a huge minres
    T.append(([1, 2, 3, 4], obs([1, 2, 3, 4]), X + 0.5, (NOITER, 1e-30, DAMP, FCT, MAXDAMP)))  # exact data, tiny minres
    T.append(([7, 9], obs([7, 9]) + [[0.2, 0.1], [-0.3, 0.2]], X + 1.0, (NOITER, MINRES, 2.0, FCT, 1.0)))  # damp >= maxdamp
    T.append(([7, 9, 11], obs([7, 9, 11]) + 0.25, X + 1.0, (NOITER, MINRES, 1e-3, 3.0, 50.0)))     # other LM options
    Xb = cs[10] - np.array([0.2, 0.1, 6.0])
    T.append(([10, 12, 14], obs([10, 12, 14], Xb), Xb, std))                 # a point behind the cameras
    T.append(([0, 23], obs([0, 23]) + [[30, -20], [-25, 40]], X * 3.0, std))  # gross outliers, far start
    T.append(([4, 5], obs([4, 5]), np.array([1e20, -1e20, 1e20]), std))      # a start that overflows f32 products
    views, xs, ys, init, opts, off = [], [], [], [], [], [0]
    for v, o, s, op in T:
        views += list(v)
        xs += list(np.asarray(o)[:, 0])
        ys += list(np.asarray(o)[:, 1])
        init.append(s)
        opts.append(op)
        off.append(len(views))
    return (np.array(off, np.int64), np.array(views, np.int32), np.array(xs, F32), np.array(ys, F32),
            np.array(init, F32), opts)


def main():
    rng = np.random.default_rng(5)
    P64, Rs, cs = make_cameras(rng, 24)
    P32 = P64.astype(F32)
    X, off, view, x, y = make_tracks(rng, P64, N_RUN)
    campos, ptdir = first_view_rays(Rs, cs, off, view, x, y)
    out = dict(P=P32, fc=np.array(FC), cc=np.array(CC), cam_R=Rs, cam_c=cs,
               options=np.array([NOITER, MINRES, DAMP, FCT, MAXDAMP]))
    with tempfile.TemporaryDirectory() as tmp:
        B = Binary(tmp)
        res = run_group(B, P32, off, view, x, y, None, campos, ptdir, [(NOITER, MINRES, DAMP, FCT, MAXDAMP)] * N_RUN)
        for m, r in res.items():
            assert np.isfinite(r["pts"]).all() and np.isfinite(r["cov"]).all(), m  # the main group has no excluded case
            err = np.linalg.norm(r["pts"] - X, axis=1)
            print(f"{m}: median error against truth {np.median(err):.4f}, iterations {np.bincount(r['iters'])}")
        k, mk = N_KEEP, int(off[N_KEEP])
        out.update(truth=X[:k], offsets=off[:k + 1], view=view[:mk], x=x[:mk], y=y[:mk], campos=campos[:k],
                   ptdir=ptdir[:k])
        for m, r in res.items():
            out.update({f"{m}_pts": r["pts"][:k], f"{m}_cov": r["cov"][:k], f"{m}_iters": r["iters"][:k]})
        doff, dview, dx, dy, dinit, dopts = degenerate_group(P64, Rs, cs)
        dcam, ddir = first_view_rays(Rs, cs, doff, dview, dx, dy)
        dres = run_group(B, P32, doff, dview, dx, dy, dinit, dcam, ddir, dopts)
        out.update(deg_offsets=doff, deg_view=dview, deg_x=dx, deg_y=dy, deg_init=dinit, deg_campos=dcam,
                   deg_ptdir=ddir, deg_options=np.array(dopts, np.float64))
        for m, r in dres.items():
            out.update({f"deg_{m}_pts": r["pts"], f"deg_{m}_cov": r["cov"], f"deg_{m}_iters": r["iters"]})
            print(f"deg {m}: iterations {r['iters']}, non-finite points {(~np.isfinite(r['pts']).all(1)).sum()}")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    sys.exit(main())
