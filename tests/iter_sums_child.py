"""Runs one problem batch of test_gpu_iter_sums.py on the device and keeps what the judge needs.

Only the single-problem engine records a trace, so a batch's problem 0 is followed through its problem record
(ProbState: p, G, H, b, dp of the last executed iteration): the same batch is tracked at ONE pyramid level with maxiter
= 1, 2, ..., maxiter, each on a fresh engine, and the record after the run of m iterations is iteration m - 1. The runs
are bit-reproducible, which the chain itself proves: the caller holds every record to dp == solve6(H, b) and
p == f32(p of the run one iteration shorter + dp) (parity_util.check_solver_turns' rules), and H must not change.

Imported by the test for the batches that need no environment. The resident form's pairs in flight per launch are
capped with ICTR_RESIDENT_SLOTS, which the library reads once per process, so for that case the test starts this file
as a fresh process:

    ICTR_RESIDENT_SLOTS=<slots> python iter_sums_child.py <slots> <in.npz> <out.npz>

in.npz: img_a, img_b, fc, cc, wh, pts (3, n) f64, poses (B, 6) f64, psz, maxiter. out.npz: see run().
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)


def run(inp):
    """Every problem has the points `pts`; problem k starts from poses[k]. Returns, for problem 0: H, b, dp, p, G per run
    (maxiter, ...), pts3d (3, n) f32 as Set3Dpoints left them,
    pt2d (2, n), T, Gx, Gy (n, psz*psz), coef (n, 16), path (the launch form's name, identical in every run)."""
    import invcompcamtrack_amd as ic
    psz, maxiter = int(inp["psz"]), int(inp["maxiter"])
    pts, poses = np.ascontiguousarray(inp["pts"], np.float64), np.ascontiguousarray(inp["poses"], np.float64)
    B, n = poses.shape[0], pts.shape[1]
    pa, pb = ic.Pyramid(inp["img_a"], 0, psz), ic.Pyramid(inp["img_b"], 0, psz)
    cam = ic.CamClass(1, inp["fc"], inp["cc"], inp["wh"], psz)
    recs, paths, out = [], set(), {}
    for m in range(1, maxiter + 1):
        op = ic.optparam(0, 0, psz, m, 0.0, 0, 0, n)
        e = ic.TrackBatch(cam, op, B)
        for k in range(B):
            e.Set3Dpoints(k, pts.copy())
        e.SetPoseAll(poses, pa, pb)
        e.track_async()
        got = e.poses()
        st = e.read_buffer(0, 8, 116)
        assert int(e.iterations()[0]) == m and np.array_equal(got[0], st[:6].astype(np.float64))
        recs.append(dict(p=st[:6].copy(), G=st[6:18].copy(), H=st[18:54].reshape(6, 6).copy(), b=st[104:110].copy(),
                         dp=st[110:116].copy()))
        paths.add(e.path_name())
        if m == maxiter:
            M = op.maxpttrack
            out["pts3d"] = e.read_buffer(0, 4, 3 * M).reshape(3, M)[:, :n].copy()
            out["pt2d"] = e.read_buffer(0, 100, 2 * M).reshape(2, M)[:, :n].copy()
            for w, q in ((0, "T"), (1, "Gx"), (2, "Gy")):
                out[q] = e.read_buffer(0, w, psz * psz * n).reshape(n, -1)
            out["coef"] = e.read_buffer(0, 7, 16 * n).reshape(n, 16)
    assert len(paths) == 1, paths
    for k in ("p", "G", "H", "b", "dp"):
        out[k] = np.stack([r[k] for r in recs])
    out["path"] = np.array(paths.pop())
    return out


def main(argv):
    slots, src, dst = int(argv[1]), argv[2], argv[3]
    if os.environ.get("ICTR_RESIDENT_SLOTS") != str(slots):
        raise SystemExit(f"ICTR_RESIDENT_SLOTS must be {slots}")
    np.savez(dst, **run(dict(np.load(src))))


if __name__ == "__main__":
    main(sys.argv)
