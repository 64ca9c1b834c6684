"""The two resident-form cases of tests/test_gpu_resident_windows.py, shared with tools/record_resident_windows.py
(which records tests/golden/resident_windows_parent.npz from the commit to compare against).

batch: 96 problems of 515 points on 640 x 480 with two pairs in flight (ICTR_RESIDENT_SLOTS=2, a fresh child process):
    thirty-two patches per wave, 48 rounds per slot. A worker holds 128 points, so the fifth worker's waves hold 3, 0, 0
    and 0 points: fewer patches than windows in flight. Points lie up to 6 px outside the frame (margin -6), so some sit
    on the margin of the view at every level and some leave it during the iterations. The child follows problem 0
    through runs of 1 .. MAXITER iterations at one level (tests/iter_sums_child.py) and then tracks the batch once more
    over a three-level pyramid.
one: one problem of 8200 + 5 points, all pairs in flight: sixteen patches per wave; the last worker holds 13, 0, 0, 0.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):  # (started as the child: nothing has set the path up)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import iter_judge as J  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "resident_windows_parent.npz")
BATCH_SCENE = (640, 480, 515, 39, -6.0)   # w, h, points, seed, margin
BATCH_B, BATCH_SLOTS, BATCH_MAXITER, BATCH_LV_F = 96, 2, 4, 2
ONE_SCENE = (256, 224, 8205, 12, 12.0)
ONE_MAXITER, ONE_LV_F = 5, 2
PSZ = 8
KEPT = 4  # problems whose b is kept in the golden file (the poses of all are)


def batch_input():
    sc = J.make_scene(*BATCH_SCENE)
    poses = sc["p_a"][None, :] + np.random.default_rng(4).normal(0, 1e-3, (BATCH_B, 6))
    poses[0] = sc["p_a"]
    return sc, dict(img_a=sc["img_a"], img_b=sc["img_b"], fc=sc["fc"], cc=sc["cc"], wh=sc["wh"], pts=sc["pts3d"],
                    poses=poses, psz=np.int32(PSZ), maxiter=np.int32(BATCH_MAXITER))


def run_batch_child(inp):
    """What this file writes when started as the child: iter_sums_child.run's record of problem 0 per run, plus, of a
    one-level run and of one three-level tracking of the same batch, the poses of all problems and b of the first KEPT."""
    import invcompcamtrack_amd as ic
    import iter_sums_child as child
    out = child.run(inp)
    psz, maxiter = int(inp["psz"]), int(inp["maxiter"])
    pts, poses = np.ascontiguousarray(inp["pts"], np.float64), np.ascontiguousarray(inp["poses"], np.float64)
    B, n = poses.shape[0], pts.shape[1]
    for tag, lv_f in (("lv0", 0), ("lv2", BATCH_LV_F)):
        pa, pb = ic.Pyramid(inp["img_a"], lv_f, psz), ic.Pyramid(inp["img_b"], lv_f, psz)
        cam = ic.CamClass(lv_f + 1, inp["fc"], inp["cc"], inp["wh"], psz)
        e = ic.TrackBatch(cam, ic.optparam(lv_f, 0, psz, maxiter, 0.0, 0, 0, n), B)
        for k in range(B):
            e.Set3Dpoints(k, pts.copy())
        e.SetPoseAll(poses, pa, pb)
        e.track_async()
        out[f"poses_{tag}"] = np.asarray(e.poses(), np.float64).copy()
        out[f"b_{tag}"] = np.stack([e.read_buffer(k, 8, 116)[104:110].copy() for k in range(KEPT)])
        out[f"path_{tag}"] = np.array(e.path_name())
    return out


def golden_of_batch(got):
    """The entries of the golden file that the batch case is held to."""
    return {"batch_b": got["b"], "batch_p": got["p"], "batch_poses_lv0": got["poses_lv0"], "batch_b_lv0": got["b_lv0"],
            "batch_poses_lv2": got["poses_lv2"], "batch_b_lv2": got["b_lv2"]}


def start_batch_child(inp, workdir, timeout):
    """The batch case in a fresh process (the library reads ICTR_RESIDENT_SLOTS once). Returns (what the child wrote or
    None, its output, why it died or None): a child that ends on a signal or at its time limit may have faulted or hung
    the device, and the caller starts nothing on it afterwards."""
    import subprocess
    src, dst = os.path.join(workdir, "in.npz"), os.path.join(workdir, "out.npz")
    np.savez(src, **inp)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), src, dst],
                           env=dict(os.environ, ICTR_RESIDENT_SLOTS=str(BATCH_SLOTS)), stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        return None, "", f"ran into its time limit of {timeout} s"
    if r.returncode < 0:
        return None, r.stdout, f"ended on signal {-r.returncode}:\n{r.stdout[-3000:]}"
    return (dict(np.load(dst)) if r.returncode == 0 else None), r.stdout, None


def run_one(oracle):
    """The one-problem case on the single-problem engine through test_gpu_iter_sums._track (solver turns, launch form,
    the judge's preconditions, every record's H and b held to that file's bar). Returns (the judge's results,
    dict(b = every record's b, pose = what TrackPose returned))."""
    import test_gpu_iter_sums as T
    sc = J.make_scene(*ONE_SCENE)
    kept, real = {}, T.check_solver_turns

    def keeping(odo, p_start, op, p_final=None, **kw):
        tr = real(odo, p_start, op, p_final=p_final, **kw)
        kept["b"] = np.stack([np.asarray(r["b"], np.float32) for r in tr])
        kept["pose"] = np.asarray(p_final, np.float64).copy()
        return tr
    T.check_solver_turns = keeping
    try:
        res = T._track(oracle, "8205", sc, "8205", PSZ, lv_f=ONE_LV_F, maxiter=ONE_MAXITER, variant=0,
                       path=("k_level_resident", None))
    finally:
        T.check_solver_turns = real
    return res, kept


def golden_of_one(kept):
    return {"one_b": kept["b"], "one_pose": kept["pose"]}


def main(argv):
    src, dst = argv[1], argv[2]
    if os.environ.get("ICTR_RESIDENT_SLOTS") != str(BATCH_SLOTS):
        raise SystemExit(f"ICTR_RESIDENT_SLOTS must be {BATCH_SLOTS}")
    np.savez(dst, **run_batch_child(dict(np.load(src))))


if __name__ == "__main__":
    main(sys.argv)
