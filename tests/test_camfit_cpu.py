"""The camera fit on the host: csrc/ictr_camfit_hd.h as plain C++ against the restatement of camfit.py (bit for bit), the
restatement against an independent judge (scipy's MINPACK Levenberg-Marquardt over rotation vector + translation), the
default schedule, the crafted inputs reaching their branches, the chain split -> depth -> fit, the helpers and the CLI."""
import os
import subprocess

import numpy as np
import pytest

import camfit_cases as K
from invcompcamtrack_amd import camfit as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5  # px, host against judge: the next power of ten above the measured worst (2.8e-6, DESIGN.md §4 "Camera fit")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _fit(c, **kw):
    return F.fit_cameras_host(c["X"], c["xy"], c["cam"], mask=c["mask"], init=c["init"], detail=True, **c["schedule"], **kw)


# ---------------------------------------------------------------- 1. header == restatement
@pytest.fixture(scope="module")
def hd_host():
    exe = os.path.join(ROOT, "tests", "cxx", "camfit_hd_host")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        "-I" + os.path.join(ROOT, "invcompcamtrack_amd", "csrc"), "-o", exe, exe + ".cpp"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _header_equals_restatement(exe, tmp_path, X, xy, cam, mask, init, schedule, what):
    prm = F._params(schedule)
    camt = F._as_cam(cam)
    words = F._words_of(mask, X.shape[1])
    G0 = F._as_poses(init, xy.shape[0])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([X.shape[1], xy.shape[0], words is not None, prm["noiter"]], np.int64).tobytes())
        f.write(np.array(camt + (prm["damp_init"], prm["damp_fct"], prm["minres"], prm["maxdamp"])).tobytes())
        f.write(np.ascontiguousarray(X, np.float64).tobytes() + np.ascontiguousarray(xy, np.float64).tobytes())
        f.write(G0.tobytes() + (b"" if words is None else words.tobytes()))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    got = np.fromfile(fout).reshape(-1, 68)
    assert len(got) == xy.shape[0]
    ps = F.pass_host(X, xy, cam, G0, mask=mask)
    fit = F.fit_cameras_host(X, xy, cam, mask=mask, init=G0, **schedule)
    solved = 0
    for f, g in enumerate(got):
        want = np.concatenate([ps["H"][f], ps["b"][f], [ps["s"][f], float(ps["n"][f])]])
        assert np.array_equal(_bits(g[:29]), _bits(want)), (what, f, "pass")
        assert not g[29:32].any()
        ok, x = F._solve([float(v) for v in ps["H"][f]], [float(v) for v in ps["b"][f]], prm["damp_init"])
        assert g[32] == float(ok), (what, f, "solve status")
        if ok:
            solved += 1
            assert np.array_equal(_bits(g[33:39]), _bits(x)), (what, f, "solve")
            assert np.array_equal(_bits(g[39:51]), _bits(F._update([float(v) for v in G0[f]], x))), (what, f, "update")
        want = np.concatenate([fit["G"][f].reshape(12), [fit["cost"][f], fit["damp"][f], fit["iters"][f], fit["status"][f],
                                                         fit["n"][f]]])
        assert np.array_equal(_bits(g[51:]), _bits(want)), (what, f, "fit")
    return solved


def test_shared_header_on_the_host_equals_the_restatement(hd_host, tmp_path):
    """csrc/ictr_camfit_hd.h compiled as plain C++ (tests/cxx/camfit_hd_host.cpp, -ffp-contract=off, address and
    undefined-behaviour sanitizers): the pass sums, the solve, the update and whole fits carry the bits of camfit.py on the
    crafted cases and on one seeded window at N = C - 1, C, C + 1 and 2 C + 1; the sanitizers stay silent."""
    solved = 0
    for name in K.CRAFTED:
        c = K.crafted(name)
        solved += _header_equals_restatement(hd_host, tmp_path, c["X"], c["xy"], c["cam"], c["mask"], c["init"],
                                             c["schedule"], name)
    C = F.CHUNK
    X, xy, _ = K.window(2 * C + 1, 3, 0.3, seed=810)
    for n in (C - 1, C, C + 1, 2 * C + 1):
        mask = np.ones(n, bool)
        mask[::7] = False
        for m in (None, mask):
            solved += _header_equals_restatement(hd_host, tmp_path, X[:, :n].copy(), xy[:, :, :n].copy(), K.CAM, m, None, {},
                                                 "N = %d" % n)
    assert solved >= 24 + 5


# ---------------------------------------------------------------- 2. the judge
def _judge(X, xy, G):
    """scipy.optimize.least_squares(method="lm") over rotation vector + translation from the true pose; shares no code
    with the restatement (projection and Rodrigues' formula are the test cases' own)."""
    opt = pytest.importorskip("scipy.optimize")
    from scipy.spatial.transform import Rotation

    def res(p):
        return (K.project(X, K.rot(p[:3]), p[3:]) - xy).reshape(-1)
    x0 = np.concatenate([Rotation.from_matrix(G[:, :3]).as_rotvec(), G[:, 3]])
    r = opt.least_squares(res, x0, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    return K.rot(r.x[:3]), r.x[3:]


def test_restatement_against_the_judge():
    """Measured: the largest distance between the reprojections under the host's pose (from the identity, minres 0,
    noiter 50) and under the judge's, over all points of the 8 scenes: 2.8e-6 px (motion 0.02, 0.3 px noise, N = 200);
    noise-free 4.6e-13 px. The gap on the noisy scenes is the judge's: its finite-difference Jacobian stops it where the
    gradient J^T r is still 5e-2 (the host's: 1.4e-9) and its cost is above the host's by 9e-12 relative. Bar: 1e-5 px.
    The host's sum of squares is never above the judge's (up to 1e-12 relative)."""
    worst = 0.0
    scenes = K.judged_scenes()
    assert len(scenes) == 8
    for motion, noise, X, xy, G in scenes:
        assert 200 <= X.shape[1] <= 500 and 4.0 <= X[2].min() and X[2].max() <= 12.0
        h = F.fit_cameras_host(X, xy, K.CAM, minres=0.0, noiter=50)
        Rj, tj = _judge(X, xy[0], G)
        ph, pj = K.project(X, h["G"][0][:, :3], h["G"][0][:, 3]), K.project(X, Rj, tj)
        d = float(np.hypot(*(ph - pj)).max())
        print("motion %.2f noise %.1f N %d: %.3e px, %d iterations, status %d"
              % (motion, noise, X.shape[1], d, h["iters"][0], h["status"][0]))
        worst = max(worst, d)
        sh, sj = ((ph - xy[0]) ** 2).sum(), ((pj - xy[0]) ** 2).sum()
        assert sh <= sj * (1.0 + 1e-12) + 1e-20, (motion, noise, sh, sj)
    print("worst %.3e px" % worst)
    assert worst <= BAR


# ---------------------------------------------------------------- 3. the default schedule
def test_default_schedule_converges():
    """Noise-free: CONVERGED with c <= minres within 10 iterations from the identity, the true pose to 4e-5. Noisy:
    CONVERGED by the improvement rule (the cost stays at the noise floor, the damping far below maxdamp)."""
    for motion, noise, X, xy, G in K.judged_scenes():
        h = F.fit_cameras_host(X, xy, K.CAM, detail=True)
        assert h["status"][0] == F.CONVERGED and h["iters"][0] <= 10, (motion, noise)
        if noise == 0.0:
            assert h["cost"][0] <= F.DEFAULTS["minres"] and np.abs(h["G"][0] - G).max() <= 4e-5
        else:
            assert h["cost"][0] > F.DEFAULTS["minres"] and h["damp"][0] < 1.0 and h["trace"][0][-1] == "accept"
            assert 0.5 * noise ** 2 < h["cost"][0] / 2.0 < 1.5 * noise ** 2  # two residuals of variance noise^2 each
        assert np.array_equal(h["p"][0], __import__("invcompcamtrack_amd").util_SE3_group_to_coeff(h["G"][0]))


# ---------------------------------------------------------------- 4. crafted inputs reach their branches
def test_fewer_than_three_counted_observations():
    for name, n in (("few_by_mask", 2), ("few_by_nan", 2), ("all_masked", 0)):
        c = K.crafted(name)
        h = _fit(c)
        assert h["status"][0] == F.FEW_OBS and h["n"][0] == n and h["iters"][0] == 0, name
        assert np.array_equal(h["G"][0], c["init"][0]) and h["trace"][0] == []
    assert _bits(h["cost"])[0] == 0x7ff8000000000000  # nothing counted: the canonical NaN


def test_depth_zero_at_the_start_is_a_cost_that_is_not_finite():
    c = K.crafted("depth_zero_at_start")
    h = _fit(c)
    assert h["status"][0] == F.START_NOT_FINITE and h["n"][0] == 80 and not np.isfinite(h["cost"][0])
    assert np.array_equal(h["G"][0], c["init"][0]) and h["iters"][0] == 0


def test_far_start_has_rejected_steps():
    h = _fit(K.crafted("far_start"))
    tr = h["trace"][0]
    assert tr[0] == "start" and "reject" in tr and "accept" in tr
    i = tr.index("reject")
    assert tr[i + 1] in ("reject", "accept") and h["iters"][0] == len(tr) - 1


def test_points_on_one_line_fail_the_solve_up_to_maxdamp():
    h = _fit(K.crafted("on_one_line"))
    assert h["trace"][0] == ["start"] + ["failed-solve"] * 10
    assert h["status"][0] == F.MAXDAMP and h["iters"][0] == 10 and h["damp"][0] == 2e10 and h["cost"][0] == 13.0
    h = _fit(K.crafted("on_one_line"), noiter=4)
    assert h["status"][0] == F.NOITER and h["iters"][0] == 4 and h["damp"][0] == 2e4


def test_nan_observations_masked_or_not_do_not_count():
    c = K.crafted("nan_masked_and_not")
    h = _fit(c)
    assert h["n"][0] == 297 and h["status"][0] == F.CONVERGED and np.isfinite(h["G"]).all() and np.isfinite(h["cost"][0])
    keep = c["mask"] & np.isfinite(c["xy"][0]).all(axis=0)
    again = F.fit_cameras_host(c["X"][:, keep], c["xy"][:, :, keep], c["cam"])
    assert np.abs(again["G"] - h["G"]).max() < 1e-9  # the same fit, summed in another order


def test_no_iterations_and_exact_start():
    c = K.crafted("no_iterations")
    h = _fit(c)
    assert h["status"][0] == F.NOITER and h["iters"][0] == 0 and h["cost"][0] > 1.0 and h["trace"][0] == ["start"]
    assert np.array_equal(h["G"][0], c["init"][0])
    c = K.crafted("exact_dyadic")
    h = _fit(c)
    assert h["status"][0] == F.CONVERGED and h["iters"][0] == 0 and h["cost"][0] == 0.0 and h["n"][0] == 36


def test_arguments():
    X, xy, _ = K.scene(20, 0.1, 0.0, 1)
    for bad in (dict(noiter=-1), dict(damp_fct=1.0), dict(damp_init=0.0), dict(minres=float("nan")), dict(maxdamp=0.0)):
        with pytest.raises(ValueError):
            F.fit_cameras_host(X, xy, K.CAM, **bad)
    with pytest.raises(TypeError):
        F.fit_cameras_host(X, xy, K.CAM, tol=1.0)
    with pytest.raises(ValueError):
        F.fit_cameras_host(X.T, xy, K.CAM)
    with pytest.raises(ValueError):
        F.fit_cameras_host(X, xy, K.CAM, mask=np.ones(19, bool))
    words = F._words_of(np.arange(20) % 3 == 0, 20)
    assert words.dtype == np.uint64 and words.shape == (1,) and int(words[0]) == sum(1 << i for i in range(0, 20, 3))
    a = F.fit_cameras_host(X, xy, K.CAM, mask=words)
    b = F.fit_cameras_host(X, xy, K.CAM, mask=np.arange(20) % 3 == 0)
    assert a["G"].tobytes() == b["G"].tobytes() and a["n"][0] == 7


# ---------------------------------------------------------------- 5. the chain
def test_chain_split_depth_fit_on_the_host():
    """The seeded stereo window (600 points, 8 frames, 30 % moving by 30 px, 0.3 px noise): no moving point is an inlier,
    and per frame the mean reprojection error in both cameras stays below 3 x the one of the true poses on the same
    inliers (a cap against a wrong fit, not a measurement)."""
    xy_t, moving, G = K.stereo_window()
    assert xy_t.shape == (600, 4, 8) and moving.sum() == 180
    split, X, left, right, fit = K.chain_host(xy_t)
    assert not split["mask"][moving].any() and split["best_count"] >= 100  # 180: what 100 rounds find at this noise
    off = [K.BASELINE, 0.0, 0.0]
    for obs, offset in ((left, None), (right, off)):
        got, n = F.reprojection_errors_host(X, obs, K.CAM, fit["G"], mask=split["words"], offset=offset)
        true, _ = F.reprojection_errors_host(X, obs, K.CAM, G, mask=split["words"], offset=offset)
        print("fit  %s\ntrue %s" % (np.round(got, 3), np.round(true, 3)))
        assert (n == split["best_count"]).all()
        # frame 0 defines the points: in the left camera the true error is rounding alone and the identity start stays
        assert (got[1:] < 3.0 * true[1:]).all() and got[0] <= 3.0 * true[0]
    assert (fit["status"] == F.CONVERGED).all()
    # the same numbers from the script's own expressions (lines 407-411)
    inl = split["inliers"]
    for f in (0, 5):
        R, t = fit["G"][f][:, :3], fit["G"][f][:, 3]
        want = np.mean(np.linalg.norm(left[f][:, inl].T - K.project(X[:, inl], R, t).T, axis=1))
        got, _ = F.reprojection_errors_host(X, left, K.CAM, fit["G"], mask=split["words"])
        assert abs(got[f] - want) < 1e-9


def test_script_steps_around_the_fit():
    """depth_from_disparity and points_from_first_view are lines 361-371 of the script; observations_from_stereo_tracks
    splits its block."""
    rng = np.random.default_rng(3)
    xy_t = rng.uniform(0, 500, (30, 4, 5))
    fx, base = 900.0, -0.4
    b = xy_t[:, 2, 0] - xy_t[:, 0, 0]
    depth = base * fx / b
    assert np.array_equal(F.depth_from_disparity(xy_t, fx, base), depth)
    cam = ((fx, 950.0), (320.0, 240.0))
    ptnorm = (xy_t[:, 0:2, 0] - np.array([320.0, 240.0])[None, :]) / np.array([fx, 950.0])[None, :]
    ptnorm = np.concatenate((ptnorm, np.ones((30, 1))), axis=1)
    ptnorm *= depth[:, None]
    assert np.array_equal(F.points_from_first_view(xy_t, cam, depth), ptnorm.T)
    left, right = F.observations_from_stereo_tracks(xy_t)
    assert left.shape == right.shape == (5, 2, 30)
    for f in range(5):
        assert np.array_equal(left[f], xy_t[:, 0:2, f].T) and np.array_equal(right[f], xy_t[:, 2:4, f].T)


# ---------------------------------------------------------------- the CLI and the native caller
def test_cli_round_trips_on_the_host(tmp_path, capsys):
    from invcompcamtrack_amd import run_fit_cameras
    X, xy, _ = K.window(300, 3, 0.3, seed=820)
    mask = np.arange(300) % 5 != 0
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, X=X, xy=xy, fc=K.FC, cc=K.CC, mask=mask)
    assert run_fit_cameras.main([fin, fout, "--host"]) == 0
    want = F.fit_cameras_host(X, xy, K.CAM, mask=mask)
    err, _ = F.reprojection_errors_host(X, xy, K.CAM, want["G"], mask=mask)
    with np.load(fout) as z:
        for k in ("G", "p", "cost", "damp", "iters", "status", "n"):
            assert z[k].tobytes() == want[k].tobytes(), k
        assert z["reproj"].tobytes() == err.tobytes()
    assert capsys.readouterr().out.splitlines() == run_fit_cameras.frame_lines(want, err)
    xy_t, moving, _ = K.stereo_window()
    np.savez(fin, xy_t=xy_t, fc=K.FC, cc=K.CC, baseline=K.BASELINE)
    assert run_fit_cameras.main([fin, fout, "--host", "--stereo"]) == 0
    split, Xs, left, right, fit = K.chain_host(xy_t)
    lines = capsys.readouterr().out.splitlines()
    with np.load(fout) as z:
        assert z["G"].tobytes() == fit["G"].tobytes() and np.array_equal(z["inliers"], split["inliers"])
        assert lines == ["[%.17g, %.17g]" % (a, b) for a, b in zip(z["reproj"], z["reproj_right"])] and len(lines) == 8


def test_native_caller_compiles_against_the_facade():
    """tests/cxx/camfit_driver.cpp (CTR::CamFitClass of include/ctr_shim.hpp) builds with plain g++ -std=c++11 and links
    against libictr_hip.so; without a device the object fails loudly."""
    import __graft_entry__ as g
    import invcompcamtrack_amd as ic
    g.build()
    exe = os.path.join(ROOT, "tests", "cxx", "camfit_driver")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        exe + ".cpp", "-L" + os.path.join(ROOT, "invcompcamtrack_amd"), "-l:libictr_hip.so",
                        "-Wl,-rpath,$ORIGIN/../../invcompcamtrack_amd"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if ic.device_count() < 1:
        with pytest.raises(ic.IctrError, match="no usable HIP device"):
            F.CameraFitter(100, 2)
        for n, nframes in ((0, 1), ((1 << 22) + 1, 1), (10, 0), (10, 4097)):
            with pytest.raises(ic.IctrError):
                F.CameraFitter(n, nframes)
