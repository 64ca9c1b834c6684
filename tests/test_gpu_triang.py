"""Multi-view triangulation on the device (ictr_triang.hip): bit for bit against the reference binary's recorded outputs
(tests/golden/triang_golden.npz) and against the NumPy restatement (tests/triang_np.py) on large ragged batches; the
single-point entry points, the reference-named wrappers, the CLI, the C++ facade and the plumbing into the tracker."""
import os
import subprocess
import sys

import numpy as np
import pytest

import invcompcamtrack_amd as ic
import triang_np as TN
from invcompcamtrack_amd import run_triangulate as RT
from invcompcamtrack_amd import triang as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FC, CC = np.array([1000.0, 1200.0]), np.array([660.0, 390.0])


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "triang_golden.npz"))


def _cov9(res):
    c = np.asarray(res["cov"], np.float32)
    if c.ndim == 1:  # depth: the scalar; the checker keeps it in column 0 of 9
        c = np.concatenate([c[:, None], np.zeros((len(c), 8), np.float32)], 1)
    return c.reshape(len(c), 9)


def _assert_bits(got, want, what):
    ok = TN.same_bits(got, want)
    print(f"{what}: {int((~ok).sum())} of {ok.size} words differ")
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} words differ, first at {np.argwhere(~ok)[0]}"


@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode", TN.MODES)
def test_device_equals_the_reference_binary_main_group(golden, mode):
    g = golden
    no, mr, di, fct, md = g["options"]
    xy = np.stack([g["x"], g["y"]], 1)
    r = T.triangulate_tracks(g["P"], g["offsets"], g["view"], xy, mode, int(no), mr, di, fct, md, init=g["dlt_pts"],
                             campos=g["campos"], ptdir=g["ptdir"])
    assert np.isfinite(g[mode + "_pts"]).all() and len(r["pts"]) == 512  # no excluded case
    _assert_bits(r["pts"], g[mode + "_pts"], mode + " points")
    _assert_bits(_cov9(r), g[mode + "_cov"], mode + " covariances")
    assert np.array_equal(r["iters"], g[mode + "_iters"])
    assert np.array_equal(r["status"], TN.status_bits(g["P"], g["offsets"], g["view"], r["pts"], _cov9(r), mode))
    if mode != "dlt":  # init=None: the DLT run first gives the same start points
        r2 = T.triangulate_tracks(g["P"], g["offsets"], g["view"], xy, mode, int(no), mr, di, fct, md,
                                  campos=g["campos"], ptdir=g["ptdir"])
        _assert_bits(r2["pts"], g[mode + "_pts"], mode + " points from the device's DLT start")


@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode", TN.MODES)
def test_device_equals_the_reference_binary_degenerate_group(golden, mode):
    g = golden
    off, opts = g["deg_offsets"], g["deg_options"]
    bad = []
    for i in range(len(off) - 1):
        s = slice(off[i], off[i + 1])
        o = opts[i]
        r = T.triangulate_tracks(g["P"], [0, off[i + 1] - off[i]], g["deg_view"][s],
                                 np.stack([g["deg_x"][s], g["deg_y"][s]], 1), mode, int(o[0]), o[1], o[2], o[3], o[4],
                                 init=g["deg_init"][i:i + 1], campos=g["deg_campos"][i:i + 1],
                                 ptdir=g["deg_ptdir"][i:i + 1])
        ok = (TN.same_bits(r["pts"], g[f"deg_{mode}_pts"][i:i + 1]).all()
              and TN.same_bits(_cov9(r), g[f"deg_{mode}_cov"][i:i + 1]).all()
              and r["iters"][0] == g[f"deg_{mode}_iters"][i])
        nonfinite = not (np.isfinite(r["pts"]).all() and np.isfinite(_cov9(r)).all())
        ok = ok and bool(r["status"][0] & 1) == nonfinite
        if not ok:
            bad.append((i, r["pts"], g[f"deg_{mode}_pts"][i], int(r["iters"][0]), int(g[f"deg_{mode}_iters"][i])))
    assert not bad, bad


def _big_scene(n, nf=64, lmin=2, lmax=32, seed=17):
    """n ragged tracks over nf cameras on a drifting path, 0.5 px noise; a few points start behind their cameras."""
    rng = np.random.default_rng(seed)
    poses = np.zeros((nf, 6))
    poses[:, 0] = -0.2 * np.arange(nf) + rng.normal(0, 0.01, nf)
    poses[:, 1:3] = rng.normal(0, 0.02, (nf, 2))
    poses[:, 3:] = rng.normal(0, 0.02, (nf, 3))
    cam = dict(fc=FC, cc=CC)
    P = T.cameras_from_poses(cam, poses)
    lens = rng.integers(lmin, lmax + 1, n)
    first = (rng.uniform(0, 1, n) * (nf - lens + 1)).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.arange(off[-1]) - np.repeat(off[:-1], lens)
    view = (np.repeat(first, lens) + idx).astype(np.int32)
    X = np.stack([rng.uniform(-3, 14, n), rng.uniform(-2, 2, n), rng.uniform(8, 14, n)], 1)
    Xr = np.repeat(X, lens, 0)
    Pv = P[view].astype(np.float64).reshape(-1, 3, 4)
    h = np.einsum("mij,mj->mi", Pv[:, :, :3], Xr) + Pv[:, :, 3]
    xy = (h[:, :2] / h[:, 2:3] + rng.normal(0, 0.5, (len(Xr), 2))).astype(np.float32)
    campos, ptdir = T.rays_from_first_view(cam, poses, off, view, xy)
    return dict(P=P, off=off, view=view, xy=xy, X=X, campos=campos, ptdir=ptdir, poses=poses, cam=cam)


@pytest.fixture(scope="module")
def big():
    sc = _big_scene(100000)
    assert len(set(np.diff(sc["off"]).tolist())) == 31  # every length 2 .. 32 occurs: every wave is ragged
    return sc


@pytest.fixture(scope="module")
def big_dlt(big):
    return T.triangulate_tracks(big["P"], big["off"], big["view"], big["xy"], "dlt")


@pytest.mark.timeout(600)
@pytest.mark.parametrize("mode", TN.MODES)
def test_device_equals_numpy_on_100000_ragged_tracks(big, big_dlt, mode):
    import torch
    sc = big
    init = big_dlt["pts"].copy()
    init[::1000] = -init[::1000]  # some starts behind the cameras: the iterations wander, the status bit is exercised
    kw = dict(noiter=10, minres=1e-5, damp_init=2.0, damp_fct=10.0, maxdamp=1e10, init=init, campos=sc["campos"],
              ptdir=sc["ptdir"])
    want = TN.triangulate(sc["P"], sc["off"], sc["view"], sc["xy"][:, 0], sc["xy"][:, 1], mode, **kw)
    t = T.Triangulator(100000, int(sc["off"][-1]), 64)
    t.set_cameras(sc["P"])
    t.set_tracks(sc["off"], sc["view"], sc["xy"])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    runs = []
    for st in (None, s1, s2, s1):
        t.run_async(mode, stream=st, **kw)
        runs.append(t.wait())
    r = runs[0]
    _assert_bits(r["pts"], want["pts"], mode + " points")
    _assert_bits(_cov9(r), want["cov"], mode + " covariances")
    assert np.array_equal(r["iters"], want["iters"])
    assert np.array_equal(r["status"], want["status"])
    assert np.array_equal(r["status"], TN.status_bits(sc["P"], sc["off"], sc["view"], r["pts"], _cov9(r), mode))
    if mode != "dlt":
        assert len(set(r["iters"].tolist())) > 1  # the stop tests fire at different iterations inside a wave
    for q in runs[1:]:  # two runs, two streams: the same bits
        for k in ("pts", "cov", "iters", "status"):
            assert q[k].tobytes() == r[k].tobytes(), k
    if mode == "dlt":
        err = np.linalg.norm(r["pts"] - sc["X"], axis=1)
        assert np.median(err) < 0.1


def test_destroy_with_a_run_pending():
    """A triangulator dropped with its run in flight ends that run before its buffers go; a fresh one then gives the
    NumPy restatement's bits. 65 two-view tracks: one full wave and one of a single track."""
    sc = _big_scene(65, nf=4, lmin=2, lmax=2, seed=65)
    t = T.Triangulator(65, 130, 4)
    t.set_cameras(sc["P"])
    t.set_tracks(sc["off"], sc["view"], sc["xy"])
    t.run_async("dlt")
    del t
    want = TN.triangulate(sc["P"], sc["off"], sc["view"], sc["xy"][:, 0], sc["xy"][:, 1], "dlt")
    r = T.triangulate_tracks(sc["P"], sc["off"], sc["view"], sc["xy"], "dlt")
    _assert_bits(r["pts"], want["pts"], "dlt points")
    _assert_bits(_cov9(r), want["cov"], "dlt covariances")
    assert np.array_equal(r["iters"], want["iters"]) and np.array_equal(r["status"], want["status"])


@pytest.mark.timeout(300)
def test_single_point_entry_points_and_reference_named_wrappers(golden):
    g = golden
    L = ic._lib.load()
    no, mr, di, fct, md = g["options"]
    fp = ic._lib.fp
    Rs, cs = g["cam_R"], g["cam_c"]
    for i in range(32):
        s = slice(g["offsets"][i], g["offsets"][i + 1])
        v = g["view"][s]
        nv = len(v)
        Pl = np.ascontiguousarray(g["P"][v].T)
        pt2d = np.ascontiguousarray(np.stack([g["x"][s], g["y"][s]], 0))
        pt, cov = np.zeros(3, np.float32), np.zeros(9, np.float32)
        assert L.ictr_triangulate_DLT(fp(pt), fp(cov), fp(pt2d), fp(Pl), nv) == 0
        assert TN.same_bits(pt, g["dlt_pts"][i]).all() and TN.same_bits(cov, g["dlt_cov"][i]).all(), i
        pt, cov = g["dlt_pts"][i].copy(), np.zeros(9, np.float32)
        assert L.ictr_triangulate_full3D(fp(pt), fp(cov), fp(pt2d), fp(Pl), nv, int(no), mr) == 0
        assert TN.same_bits(pt, g["gn_pts"][i]).all() and TN.same_bits(cov, g["gn_cov"][i]).all(), i
        pt, cov = g["dlt_pts"][i].copy(), np.zeros(9, np.float32)
        assert L.ictr_triangulate_full3D_LM(fp(pt), fp(cov), fp(pt2d), fp(Pl), nv, int(no), di, fct, mr, md) == 0
        assert TN.same_bits(pt, g["lm_pts"][i]).all() and TN.same_bits(cov, g["lm_cov"][i]).all(), i
        pt, cov = g["dlt_pts"][i].copy(), np.zeros(1, np.float32)
        cp, pd = g["campos"][i].copy(), g["ptdir"][i].copy()
        assert L.ictr_triangulate_depthonly(fp(pt), fp(cov), fp(cp), fp(pd), fp(pt2d), fp(Pl), nv, int(no), mr) == 0
        assert TN.same_bits(pt, g["depth_pts"][i]).all() and TN.same_bits(cov, g["depth_cov"][i, :1]).all(), i
        # the reference callers' names: cameras as (R, position), observations per view
        R_l, tw_l = [Rs[k] for k in v], [cs[k] for k in v]
        x_l = [np.array([g["x"][j], g["y"][j]]) for j in range(s.start, s.stop)]
        p1, c1 = T.func_pt_triangulate_from_P_linear_sq(g["fc"], g["cc"], R_l, tw_l, x_l, use_c_interf=True)
        assert TN.same_bits(p1, g["dlt_pts"][i]).all() and TN.same_bits(c1.reshape(-1), g["dlt_cov"][i]).all(), i
        p2 = T.func_pt_triangulate_from_P_nonlin_LM(p1, g["fc"], g["cc"], R_l, tw_l, x_l, noiter=int(no), mswitch=0,
                                                    lamb_damp_init=di, lamp_damp_fact=fct, minres=mr, use_c_interf=True)
        assert TN.same_bits(p2, g["lm_pts"][i]).all(), i
        p3 = T.func_pt_triangulate_from_P_nonlin_LM(p1, g["fc"], g["cc"], R_l, tw_l, x_l, noiter=int(no), mswitch=1,
                                                    minres=mr, use_c_interf=True)
        assert TN.same_bits(p3, g["depth_pts"][i]).all(), i
    # a loop that never runs leaves the caller's covariance alone, as the reference does
    pt, cov = g["dlt_pts"][0].copy(), np.full(9, 7.0, np.float32)
    assert L.ictr_triangulate_full3D(fp(pt), fp(cov), fp(pt2d), fp(Pl), nv, 0, mr) == 0
    assert np.all(cov == 7.0) and TN.same_bits(pt, g["dlt_pts"][0]).all()


@pytest.mark.timeout(300)
def test_cli_and_cxx_facade_write_the_same_files(tmp_path, golden):
    g = golden
    k = 200
    m = int(g["offsets"][k])
    xy = np.stack([g["x"][:m], g["y"][:m]], 1)
    fin, fno = str(tmp_path / "in.txt"), str(tmp_path / "in_noinit.txt")
    RT.write_triang_input(fin, g["P"], g["offsets"][:k + 1], g["view"][:m], xy, init=g["dlt_pts"][:k],
                          campos=g["campos"][:k], ptdir=g["ptdir"][:k])
    RT.write_triang_input(fno, g["P"], g["offsets"][:k + 1], g["view"][:m], xy)
    exe = str(tmp_path / "triang_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "triang_driver.cpp"),
                           "-L" + os.path.join(ROOT, "invcompcamtrack_amd"), "-l:libictr_hip.so",
                           "-Wl,-rpath," + os.path.join(ROOT, "invcompcamtrack_amd")], timeout=300)
    for mode in TN.MODES:
        for src in (fin, fno):
            if mode == "depth" and src == fno:
                continue
            a, b = str(tmp_path / f"py_{mode}.txt"), str(tmp_path / f"cx_{mode}.txt")
            assert RT.main([src, a, "--mode", mode]) == 0
            r = subprocess.run([exe, src, b, mode], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stdout + r.stderr
            assert open(a, "rb").read() == open(b, "rb").read(), (mode, src)
            rows = np.loadtxt(a)
            assert rows.shape == (k, 6 if mode == "depth" else 14)
            assert np.array_equal(rows[:, :3].astype(np.float32), g[mode + "_pts"][:k])
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = str(tmp_path / "mod.txt")
    subprocess.check_call([sys.executable, "-m", "invcompcamtrack_amd.run_triangulate", fin, out, "--mode", "lm"],
                          cwd=ROOT, env=env, timeout=120)
    assert open(out, "rb").read() == open(str(tmp_path / "py_lm.txt"), "rb").read()


@pytest.mark.timeout(600)
def test_end_to_end_points_feed_the_tracker():
    """Poses from track_sequence -> cameras; observations = true projections + 0.5 px noise -> triangulate_tracks ->
    Set3Dpoints / TrackPose on a later pair. The device's points are the NumPy checker's bits, so both trackings agree
    within the tracker's 1e-4 pose bar: this checks the plumbing, not accuracy."""
    from invcompcamtrack_amd import sequence as sq
    from invcompcamtrack_amd import synth
    from seq_scene import make_pan
    W, H, NF, NW = 640, 480, 10, 2000
    sc = make_pan(W, H, NF, NW, step=-0.5, seed=8, tilt=0.5)
    args = (4, 0, 8, 10, 0.01, 1, 1)
    op = ic.optparam(*args, 128)
    cam = ic.CamClass(args[0] + 1, sc["cam"]["fc"], sc["cam"]["cc"], sc["cam"]["wh"], args[2])
    dev = sq.track_sequence(cam, op, sc["pts3d"], sc["frames"], sc["poses"][0], 10)
    poses = dev["poses"]
    assert np.all(np.isfinite(poses))
    # tracks: the world points that frames 0 .. 5 all see (true poses), observed with 0.5 px noise
    rng = np.random.default_rng(4)
    fc, cc = sc["cam"]["fc"].astype(np.float64), sc["cam"]["cc"].astype(np.float64)
    X = sc["pts3d"]
    uv = []
    for k in range(6):
        G = synth.se3_exp(sc["poses"][k]).reshape(3, 4)
        Xc = G[:, :3] @ X + G[:, 3:4]
        uv.append(np.stack([fc[0] * Xc[0] / Xc[2] + cc[0], fc[1] * Xc[1] / Xc[2] + cc[1]], 1))
    uv = np.stack(uv, 1)  # [Nw, 6, 2]
    seen = np.all((uv[:, :, 0] >= 1) & (uv[:, :, 0] <= W) & (uv[:, :, 1] >= 1) & (uv[:, :, 1] <= H), 1)
    ids = np.nonzero(seen)[0][:120]
    assert len(ids) >= 60
    n = len(ids)
    off = 6 * np.arange(n + 1, dtype=np.int64)
    view = np.tile(np.arange(6, dtype=np.int32), n)
    xy = (uv[ids] + rng.normal(0, 0.5, (n, 6, 2))).reshape(-1, 2).astype(np.float32)
    camd = dict(fc=fc, cc=cc)
    P = T.cameras_from_poses(camd, poses[:6])
    got = T.triangulate_tracks(P, off, view, xy, "lm")
    dlt = TN.triangulate(P, off, view, xy[:, 0], xy[:, 1], "dlt")
    want = TN.triangulate(P, off, view, xy[:, 0], xy[:, 1], "lm", init=dlt["pts"])
    _assert_bits(got["pts"], want["pts"], "points")
    assert np.array_equal(got["status"], want["status"]) and (got["status"] == 0).mean() > 0.9
    assert np.median(np.linalg.norm(got["pts"] - X[:, ids].T, axis=1)) < 1.0

    def track(pts, status):
        p3 = np.ascontiguousarray(pts[status == 0].T.astype(np.float64))
        op2 = ic.optparam(*args, p3.shape[1])
        pose = ic.PoseClass(cam, op2)
        odo = ic.OdometerClass(pose, op2)
        pa, pb = ic.Pyramid(sc["frames"][6], args[0], args[2]), ic.Pyramid(sc["frames"][7], args[0], args[2])
        odo.Set3Dpoints(p3)
        odo.SetPose(poses[6], pa, pb)
        return odo.TrackPose()

    p_dev, p_np = track(got["pts"], got["status"]), track(want["pts"], want["status"])
    print("pose from the device's points", p_dev, "\npose from the checker's points", p_np)
    assert np.abs(p_dev - p_np).max() <= 1e-4
    assert np.all(np.isfinite(p_dev))


@pytest.mark.timeout(120)
def test_refusals_and_caps(golden):
    g = golden
    k = 64
    m = int(g["offsets"][k])
    xy = np.stack([g["x"][:m], g["y"][:m]], 1)
    off, view = g["offsets"][:k + 1], g["view"][:m]
    with pytest.raises(ic.IctrError):
        T.Triangulator(0, 10, 4)
    t = T.Triangulator(k, m, 24)
    with pytest.raises(ic.IctrError):  # tracks before cameras
        t.set_tracks(off, view, xy)
    with pytest.raises(ic.IctrError):  # more frames than the cap
        t.set_cameras(np.zeros((25, 12), np.float32))
    t.set_cameras(g["P"])
    with pytest.raises(ic.IctrError):  # run before tracks
        t.run_async("dlt")
    with pytest.raises(ic.IctrError):  # more points than the cap
        t.set_tracks(g["offsets"][:k + 2], g["view"][:int(g["offsets"][k + 1])], np.zeros((int(g["offsets"][k + 1]), 2)))
    small = T.Triangulator(k, m - 1, 24)
    small.set_cameras(g["P"])
    with pytest.raises(ic.IctrError):  # more observations than the cap
        small.set_tracks(off, view, xy)
    bad_view = view.copy()
    bad_view[5] = 24
    with pytest.raises(ic.IctrError, match="view index"):
        t.set_tracks(off, bad_view, xy)
    bad_view[5] = -1
    with pytest.raises(ic.IctrError, match="view index"):
        t.set_tracks(off, bad_view, xy)
    short = off.copy()
    short[1] = 1  # the first track has one view (the second one more)
    with pytest.raises(ic.IctrError, match="fewer than 2"):
        t.set_tracks(short, view, xy)
    with pytest.raises(ic.IctrError):  # a refused set_tracks leaves no tracks behind
        t.run_async("dlt")
    t.set_tracks(off, view, xy)
    for mode in ("gn", "lm", "depth"):
        with pytest.raises(ic.IctrError, match="initial points"):
            t.run_async(mode)
    with pytest.raises(ic.IctrError, match="centres and rays"):
        t.run_async("depth", init=g["dlt_pts"][:k])
    with pytest.raises(ic.IctrError):
        t.run_async("gn", noiter=-1, init=g["dlt_pts"][:k])
    with pytest.raises(ic.IctrError):  # nothing in flight after the refused calls
        t.wait()
    t.run_async("lm", init=g["dlt_pts"][:k])
    with pytest.raises(ic.IctrError, match="in flight"):
        t.set_cameras(g["P"])
    with pytest.raises(ic.IctrError, match="in flight"):
        t.set_tracks(off, view, xy)
    with pytest.raises(ic.IctrError, match="in flight"):
        t.run_async("dlt")
    r = t.wait()
    _assert_bits(r["pts"], g["lm_pts"][:k], "points after the refused calls")
    with pytest.raises(ic.IctrError):
        t.wait()
    t.set_cameras(g["P"][:12])  # fewer frames than the tracks were checked against: they have to be set again
    with pytest.raises(ic.IctrError):
        t.run_async("dlt")
    with pytest.raises(ic.IctrError, match="view index"):
        t.set_tracks(off, view, xy)
