"""The window bundle adjustment on the host: csrc/ictr_ba_hd.h as plain C++ against the restatement of bundle.py (bit for
bit), the restatement against an independent judge (scipy's trust-region least squares over rotation vectors,
translations and points), descent and usefulness on the chain's stereo window, the crafted inputs reaching their
branches, the golden windows, the arguments and the new C entries without a device."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import bundle_cases as BC
import camfit_cases as K
from invcompcamtrack_amd import bundle as B
from invcompcamtrack_amd import camfit as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# px, host against judge: one decade above the measured worst (DESIGN.md §4 "Window bundle adjustment")
BAR_NOISY, BAR_EXACT = 1e-3, 1e-11


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---------------------------------------------------------------- 1. header == restatement
@pytest.fixture(scope="module")
def hd_host():
    exe = os.path.join(ROOT, "tests", "cxx", "bundle_hd_host")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        "-I" + os.path.join(ROOT, "invcompcamtrack_amd", "csrc"), "-o", exe, exe + ".cpp"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _header_equals_restatement(exe, tmp_path, X, xy, cam, offset, mask, init, schedule, what):
    X = F._as_points(X)
    n = X.shape[1]
    xy = B._as_obs(xy, n)
    S, Fr = xy.shape[:2]
    prm, words, G0 = F._params(schedule), F._words_of(mask, n), F._as_poses(init, xy.shape[1])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([n, Fr, S, words is not None, prm["noiter"]], np.int64).tobytes())
        f.write(np.array(F._as_cam(cam) + (prm["damp_init"], prm["damp_fct"], prm["minres"], prm["maxdamp"])
                         + tuple(B._as_offset(offset))).tobytes())
        f.write(X.tobytes() + xy.tobytes() + G0.tobytes() + (b"" if words is None else words.tobytes()))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    got = np.fromfile(fout)
    dim = 6 * (Fr - 1)
    sy = B.system_host(X, xy, cam, G0, prm["damp_init"], offset=offset, mask=mask)
    want = np.concatenate([[sy["n"], sy["cost"], sy["nfail"]], sy["A"], sy["rhs"], sy["V"].ravel(), sy["gp"].ravel()])
    at = len(want)
    assert np.array_equal(_bits(got[:at]), _bits(want)), (what, "system")
    # the reduced solve, the pose update and the points' back-substitution of the first step
    P = B._Problem(X, xy, cam, offset, mask)
    ok, dc = (False, None) if sy["nfail"] else B._reduced_solve(sy["A"], sy["rhs"], dim)
    assert got[at] == float(ok), (what, "solve status")
    solved = 0
    if ok:
        solved = 1
        Gt = G0.copy()
        for f in range(1, Fr):
            Gt[f] = F._update([float(v) for v in G0[f]], dc[6 * (f - 1):6 * f])
        with np.errstate(all="ignore"):
            Xt = P.back_pass(G0, P.X0, sy["V"], sy["gp"], prm["damp_init"], dc)
        want = np.concatenate([dc, Gt.ravel(), Xt.ravel()])
        assert np.array_equal(_bits(got[at + 1:at + 1 + len(want)]), _bits(want)), (what, "first step")
    run = B.adjust_window_host(X, xy, cam, offset=offset, mask=mask, init=G0, **schedule)
    want = np.concatenate([run["G"].ravel(), run["X"].ravel(), [run["cost"], run["damp"], run["iters"], run["status"],
                                                               run["n"]]])
    assert np.array_equal(_bits(got[-len(want):]), _bits(want)), (what, "run")
    assert len(got) == at + 1 + dim + 12 * Fr + 3 * n + len(want)
    return solved


def test_shared_header_on_the_host_equals_the_restatement(hd_host, tmp_path):
    """csrc/ictr_ba_hd.h compiled as plain C++ (tests/cxx/bundle_hd_host.cpp, -ffp-contract=off, address and
    undefined-behaviour sanitizers): the per-point blocks, the reduced system, both solves, the update and whole runs
    carry the bits of bundle.py on the crafted cases and on one seeded window at N = C - 1, C, C + 1 and 2 C + 1 with
    F = 3, one and two sides, with and without a mask; the sanitizers stay silent."""
    solved = 0
    for name in BC.CRAFTED:
        c = BC.crafted(name)
        solved += _header_equals_restatement(hd_host, tmp_path, c["X"], c["xy"], c["cam"], c["offset"], c["mask"],
                                             c["init"], c["schedule"], name)
    Cn = F.CHUNK
    w = BC.window(2 * Cn + 1, 3, 2, 0.3, seed=920, pose_err=0.02)
    for n in (Cn - 1, Cn, Cn + 1, 2 * Cn + 1):
        for S in (1, 2):
            for m in (None, BC.spotted_mask(n, n)):
                solved += _header_equals_restatement(hd_host, tmp_path, w["X0"][:, :n].copy(), w["xy"][:S, :, :, :n].copy(),
                                                     BC.CAM, BC.OFFSET if S == 2 else None, m, w["G0"], dict(noiter=3),
                                                     "N = %d, S = %d" % (n, S))
    assert solved >= 16 + 7


# ---------------------------------------------------------------- 2. the judge
def _judge(w, offset):
    """scipy.optimize.least_squares over rotation vectors, translations and points with frame 0 fixed, started at the
    true poses and points; shares no code with the restatement (projection and Rodrigues' formula are the test cases'
    own)."""
    opt = pytest.importorskip("scipy.optimize")
    from scipy.sparse import lil_matrix
    from scipy.spatial.transform import Rotation
    xy, G = w["xy"], w["G"]
    S, Fr, _, n = xy.shape
    off = [np.zeros(3), np.asarray(offset, np.float64)]

    def unpack(p):
        poses = [(G[0][:, :3], G[0][:, 3])] + [(K.rot(p[6 * f:6 * f + 3]), p[6 * f + 3:6 * f + 6]) for f in range(Fr - 1)]
        return poses, p[6 * (Fr - 1):].reshape(3, n)

    def res(p):
        poses, X = unpack(p)
        return np.concatenate([(K.project(X, R, t + off[s]) - xy[s, f]).reshape(-1)
                               for s in range(S) for f, (R, t) in enumerate(poses)])

    sp = lil_matrix((2 * S * Fr * n, 6 * (Fr - 1) + 3 * n), dtype=int)
    for s in range(S):
        for f in range(Fr):
            r0 = (s * Fr + f) * 2 * n
            if f:
                sp[r0:r0 + 2 * n, 6 * (f - 1):6 * f] = 1
            for k in range(3):
                for c in range(2):
                    sp[r0 + c * n + np.arange(n), 6 * (Fr - 1) + k * n + np.arange(n)] = 1
    x0 = np.concatenate([np.concatenate([Rotation.from_matrix(G[f][:, :3]).as_rotvec(), G[f][:, 3]]) for f in range(1, Fr)]
                        + [w["X"].reshape(-1)])
    r = opt.least_squares(res, x0, method="trf", jac_sparsity=sp, x_scale="jac", xtol=1e-15, ftol=1e-15, gtol=1e-15,
                          max_nfev=200)
    return unpack(r.x)


@functools.lru_cache(maxsize=None)
def judged_scenes():
    """8 scenes: N = 40 .. 80, F = 3 .. 5, two sides, noise 0 and 0.3 px, the points started with 3 % of depth error."""
    out = []
    for i, (noise, (n, nframes)) in enumerate((s, nf) for s in K.NOISES for nf in ((40, 3), (55, 4), (70, 5), (80, 3))):
        out.append((noise, BC.window(n, nframes, 2, noise, seed=960 + i, depth_err=0.03)))
    return out


def test_restatement_against_the_judge():
    """Measured: the largest distance between the reprojections under the host's poses and points (from the true poses
    and 3 % depth error, minres 0, noiter 100) and under the judge's, over every observation: 8.8e-5 px on the 4 noisy
    scenes, 3.2e-13 px on the 4 noise-free ones. The gap on the noisy scenes is the judge's: it stops where its sum of
    squares is still above the host's by 1e-9 relative. Bars, one decade above: 1e-3 and 1e-11 px. The host's sum of
    squares is never above the judge's (up to 1e-12 relative)."""
    worst = {0.0: 0.0, 0.3: 0.0}
    scenes = judged_scenes()
    assert len(scenes) == 8
    for noise, w in scenes:
        xy = w["xy"]
        S, Fr, _, n = xy.shape
        assert S == 2 and 40 <= n <= 80 and 3 <= Fr <= 5
        h = B.adjust_window_host(w["X0"], xy, BC.CAM, offset=BC.OFFSET, init=w["G"], minres=0.0, noiter=100)
        poses, Xj = _judge(w, BC.OFFSET)
        d = sh = sj = 0.0
        for s in range(S):
            for f in range(Fr):
                o = np.asarray(BC.OFFSET) * s
                ph = K.project(h["X"], h["G"][f][:, :3], h["G"][f][:, 3] + o)
                pj = K.project(Xj, poses[f][0], poses[f][1] + o)
                d = max(d, float(np.hypot(*(ph - pj)).max()))
                sh += ((ph - xy[s, f]) ** 2).sum()
                sj += ((pj - xy[s, f]) ** 2).sum()
        print("noise %.1f N %d F %d: %.3e px, %d iterations, status %d, ssq host %.17g judge %.17g"
              % (noise, n, Fr, d, h["iters"], h["status"], sh, sj))
        worst[noise] = max(worst[noise], d)
        assert sh <= sj * (1.0 + 1e-12) + 1e-20, (noise, n, Fr, sh, sj)
    print("worst: noisy %.3e px, noise-free %.3e px" % (worst[0.3], worst[0.0]))
    assert worst[0.3] <= BAR_NOISY and worst[0.0] <= BAR_EXACT


# ---------------------------------------------------------------- 3. descent and usefulness
def test_descent_and_usefulness_on_the_chains_stereo_window():
    """camfit_cases.stereo_window() after chain_host: the default schedule converges, every accepted cost is below the
    one before, the final cost is below the cost at the true poses and points, and both per-frame reprojection means are
    no larger than chain_host's (frame 0 in the left camera: at most equal)."""
    xy_t, moving, G = K.stereo_window()
    split, X, left, right, fit = K.chain_host(xy_t)
    xy = np.stack([left, right])
    h = B.adjust_window_host(X, xy, K.CAM, offset=BC.OFFSET, mask=split["words"], init=fit["G"], detail=True)
    assert h["status"] == B.CONVERGED and h["n"] == split["best_count"]
    assert len(h["costs"]) >= 3 and (np.diff(h["costs"]) < 0).all() and h["costs"][-1] == h["cost"]
    # the cost at the truth: the true points are the first view's, X_true = depth-exact points; take them from the
    # noise-free geometry of the same seed
    rng = np.random.default_rng(700)
    Xtrue = K.points(600, rng)
    true = B.system_host(Xtrue, xy, K.CAM, G, 2.0, offset=BC.OFFSET, mask=split["words"])
    start = B.system_host(X, xy, K.CAM, fit["G"], 2.0, offset=BC.OFFSET, mask=split["words"])
    print("cost: start %.4f, adjusted %.4f, at the truth %.4f, %d iterations" % (start["cost"], h["cost"], true["cost"],
                                                                                 h["iters"]))
    assert start["cost"] == h["costs"][0] and h["cost"] < true["cost"] < start["cost"]
    for obs, offset in ((left, None), (right, list(BC.OFFSET))):
        before, _ = F.reprojection_errors_host(X, obs, K.CAM, fit["G"], mask=split["words"], offset=offset)
        after, _ = F.reprojection_errors_host(h["X"], obs, K.CAM, h["G"], mask=split["words"], offset=offset)
        print("before %s\nafter  %s" % (np.round(before, 3), np.round(after, 3)))
        assert (after[1:] <= before[1:]).all()
        if offset is None:
            assert after[0] <= before[0] or np.array_equal(h["G"][0], fit["G"][0])
    assert np.array_equal(_bits(h["G"][0]), _bits(fit["G"][0]))  # the gauge: frame 0 keeps its start pose
    assert not np.array_equal(h["X"][:, split["mask"]], X[:, split["mask"]])
    assert np.array_equal(_bits(h["X"][:, ~split["mask"]]), _bits(X[:, ~split["mask"]]))


# ---------------------------------------------------------------- 4. crafted inputs reach their branches
def test_fewer_than_three_adjusted_points():
    for name, n in (("all_masked", 0), ("two_adjusted", 2)):
        c = BC.crafted(name)
        h = BC.run_host(c)
        assert h["status"] == B.FEW_OBS and h["n"] == n and h["iters"] == 0 and h["trace"] == [], name
        assert np.array_equal(_bits(h["G"]), _bits(c["init"])) and np.array_equal(_bits(h["X"]), _bits(c["X"]))
    assert _bits(BC.run_host(BC.crafted("all_masked"))["cost"])[0] == 0x7ff8000000000000  # the canonical NaN


def test_a_nan_observation_takes_its_point_out_of_every_frame():
    c = BC.crafted("nan_observation")
    h = BC.run_host(c)
    assert h["n"] == 129 and h["status"] == B.CONVERGED
    assert np.array_equal(_bits(h["X"][:, 64]), _bits(c["X"][:, 64])) and np.isfinite(h["X"]).all()
    assert (h["X"][:, :64] != c["X"][:, :64]).any(axis=0).all()


def test_depth_zero_at_the_start_is_a_cost_that_is_not_finite():
    c = BC.crafted("depth_zero_at_start")
    h = BC.run_host(c)
    assert h["status"] == B.START_NOT_FINITE and h["n"] == 80 and not np.isfinite(h["cost"]) and h["iters"] == 0
    assert np.array_equal(_bits(h["G"]), _bits(c["init"])) and np.array_equal(_bits(h["X"]), _bits(c["X"]))


def test_points_on_the_axis_fail_the_solve_up_to_maxdamp_or_noiter():
    h = BC.run_host(BC.crafted("on_the_axis"))
    assert h["trace"] == ["start"] + ["failed-solve"] * 10
    assert h["status"] == B.MAXDAMP and h["iters"] == 10 and h["damp"] == 2e10 and h["cost"] == 13.0
    h = BC.run_host(BC.crafted("on_the_axis"), noiter=4)
    assert h["status"] == B.NOITER and h["iters"] == 4 and h["damp"] == 2e4
    s = B.system_host(**{k: BC.crafted("on_the_axis")[k] for k in ("X", "xy", "cam")}, G=K.identity(3), damp=2.0)
    assert s["nfail"] == 10


def test_far_starts_have_rejected_steps_and_failed_solves():
    h = BC.run_host(BC.crafted("far_start"))
    tr = h["trace"]
    assert tr[0] == "start" and "reject" in tr and "accept" in tr and h["iters"] == len(tr) - 1
    assert h["status"] == B.CONVERGED and h["cost"] < 1e-5
    h = BC.run_host(BC.crafted("failed_between"))
    tr = h["trace"]
    i = tr.index("failed-solve")
    assert "accept" in tr[:i] and "accept" in tr[i:] and h["iters"] == len(tr) - 1


def test_no_iterations_and_exact_start():
    c = BC.crafted("no_iterations")
    h = BC.run_host(c)
    assert h["status"] == B.NOITER and h["iters"] == 0 and h["cost"] > 0.1 and h["trace"] == ["start"]
    assert np.array_equal(_bits(h["G"]), _bits(c["init"])) and np.array_equal(_bits(h["X"]), _bits(c["X"]))
    h = BC.run_host(BC.crafted("exact_dyadic"))
    assert h["status"] == B.CONVERGED and h["iters"] == 0 and h["cost"] == 0.0 and h["n"] == 36


def test_one_side_and_two_frames():
    """One side: the scale is free and only the damping keeps the system definite, so the test is descent, not
    recovery. Two frames: one moving camera."""
    for name in ("one_side", "two_frames"):
        h = BC.run_host(BC.crafted(name))
        assert h["status"] == B.CONVERGED and h["iters"] >= 3 and (np.diff(h["costs"]) < 0).all(), name
        assert np.isfinite(h["X"]).all() and np.isfinite(h["G"]).all()


def test_arguments():
    w = BC.window(20, 3, 2, 0.0, 1)
    args = (w["X0"], w["xy"], BC.CAM)
    for bad in (dict(noiter=-1), dict(damp_fct=1.0), dict(damp_init=0.0), dict(minres=float("nan")), dict(maxdamp=0.0)):
        with pytest.raises(ValueError):
            B.adjust_window_host(*args, offset=BC.OFFSET, **bad)
    with pytest.raises(TypeError):
        B.adjust_window_host(*args, tol=1.0)
    for X, xy in ((w["X0"].T, w["xy"]), (w["X0"], w["xy"][:, :1]), (w["X0"], np.zeros((3, 3, 2, 20))),
                  (w["X0"][:, :7], w["xy"][..., :7]), (w["X0"], np.zeros((1, 33, 2, 20)))):
        with pytest.raises(ValueError):
            B.adjust_window_host(X, xy, BC.CAM)
    with pytest.raises(ValueError):
        B.adjust_window_host(*args, mask=np.ones(19, bool))
    with pytest.raises(ValueError):
        B.adjust_window_host(*args, offset=[0.0, np.nan, 0.0])
    bad = w["G0"].copy()
    bad[1, 0, 0] = np.inf
    with pytest.raises(ValueError):
        B.adjust_window_host(*args, init=bad)
    a = B.adjust_window_host(*args, offset=BC.OFFSET, mask=F._words_of(np.arange(20) % 3 != 0, 20))
    b = B.adjust_window_host(*args, offset=BC.OFFSET, mask=np.arange(20) % 3 != 0)
    assert a["G"].tobytes() == b["G"].tobytes() and a["X"].tobytes() == b["X"].tobytes() and a["n"] == 13
    one = B.adjust_window_host(w["X0"], w["xy"][0], BC.CAM, noiter=2)  # (F, 2, N) is one side
    assert one["G"].shape == (3, 3, 4) and one["X"].shape == (3, 20)


# ---------------------------------------------------------------- 5. the golden windows
@pytest.mark.parametrize("thresh", [0.03, 2.0])
def test_window_bundle_host_on_the_golden_windows(thresh):
    import windowcams_cases as WC
    from invcompcamtrack_amd import windowcams as W
    from test_stereotrack_cpu import fields, golden
    for name in WC.WINDOWS:
        r = W.window_bundle_host(*fields(golden()[name]), K.CAM, K.BASELINE, thresh=thresh)
        WC.same(r, WC.host(name, thresh), name)  # the existing result is untouched
        assert "xy_t" not in r
        xy_t = WC.host(name, thresh)["xy_t"]
        X = F.points_from_first_view(xy_t, K.CAM, F.depth_from_disparity(xy_t, K.FC[0], K.BASELINE))
        start = B.system_host(X, np.stack(F.observations_from_stereo_tracks(xy_t)), K.CAM, r["G"], 2.0, offset=BC.OFFSET,
                              mask=r["words"])
        ba = r["ba"]
        print(name, "status", ba["status"], "iters", ba["iters"], "cost", start["cost"], "->", ba["cost"])
        assert ba["status"] in (B.CONVERGED, B.NOITER, B.MAXDAMP) and ba["cost"] <= start["cost"]
        assert ba["n"] == r["best_count"] and r["err_left_ba"].shape == r["err_right_ba"].shape == r["err_left"].shape
    with pytest.raises(ValueError, match="bsize"):
        W._check_bundle(33, None)


# ---------------------------------------------------------------- 6. the C entries without a device
def test_new_entry_points_fail_loudly_on_null_and_without_a_device():
    import __graft_entry__ as g
    import invcompcamtrack_amd as ic
    from invcompcamtrack_amd import _lib
    g.build()
    L = _lib.load()
    d, none = np.zeros(64), None
    i64, i32, dbl = C.c_int64(), C.c_int32(), C.c_double()
    assert L.ictr_ba_create(None, 100, 3, 1) != 0
    for call in (lambda: L.ictr_ba_set_points(none, _lib.dp(d)), lambda: L.ictr_ba_set_observations(none, _lib.dp(d)),
                 lambda: L.ictr_ba_set_mask(none, None), lambda: L.ictr_ba_set_camera(none, _lib.dp(d), _lib.dp(d)),
                 lambda: L.ictr_ba_set_offset(none, _lib.dp(d)), lambda: L.ictr_ba_set_timing(none, 1),
                 lambda: L.ictr_ba_run(none, _lib.dp(d), 1, 2.0, 10.0, 1e-5, 1e10, None),
                 lambda: L.ictr_ba_wait(none, None, None, None, None, None, None, None),
                 lambda: L.ictr_ba_get_kernel_times(none, None),
                 lambda: L.ictr_debug_ba_system(none, _lib.dp(d), None, 2.0, C.byref(i64), C.byref(dbl), _lib.dp(d),
                                                _lib.dp(d), _lib.dp(d), _lib.dp(d), C.byref(i64)),
                 lambda: L.ictr_ba_set_points_from_window(none, none, 1.0),
                 lambda: L.ictr_ba_set_observations_from_window(none, none),
                 lambda: L.ictr_ba_set_mask_from_fsplit(none, none, None),
                 lambda: L.ictr_debug_ba_inputs(none, None, None, None)):
        assert call() != 0 and L.ictr_last_error()
    L.ictr_ba_destroy(None)
    for args in ((7, 3, 1), ((1 << 22) + 1, 3, 1), (100, 1, 1), (100, 33, 1), (100, 3, 0), (100, 3, 3)):
        with pytest.raises(ic.IctrError):
            B.BundleAdjuster(*args)
    if ic.device_count() < 1:
        with pytest.raises(ic.IctrError, match="no usable HIP device"):
            B.BundleAdjuster(100, 3, 2)
        w = BC.window(20, 3, 2, 0.0, 1)
        with pytest.raises(ic.IctrError):
            B.adjust_window(w["X0"], w["xy"], BC.CAM, offset=BC.OFFSET)


# ---------------------------------------------------------------- 7. the CLI and the native caller
def test_cli_round_trips_on_the_host(tmp_path, capsys):
    from invcompcamtrack_amd import run_bundle
    w = BC.window(60, 3, 2, 0.3, seed=970, pose_err=0.02)
    mask = np.arange(60) % 5 != 0
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, X=w["X0"], xy=w["xy"], fc=K.FC, cc=K.CC, offset=BC.OFFSET, mask=mask, init=w["G0"])
    assert run_bundle.main([fin, fout, "--host"]) == 0
    want = B.adjust_window_host(w["X0"], w["xy"], BC.CAM, offset=BC.OFFSET, mask=mask, init=w["G0"])
    with np.load(fout) as z:
        for k in run_bundle.KEYS:
            assert z[k].tobytes() == np.asarray(want[k]).tobytes(), k
    lines = capsys.readouterr().out.splitlines()
    assert lines == run_bundle.result_lines(want) and len(lines) == 1 + 3 + 60
    assert float.fromhex(lines[0].split()[7]) == want["cost"] and lines[1].startswith("G 0: 0x1p+0 0x0p+0 ")
    assert [run_bundle.hexf(v) for v in (1.0, 0.0, -2.5, 0.1, float("inf"), float("nan"), 5e-324)] == [
        "0x1p+0", "0x0p+0", "-0x1.4p+1", "0x1.999999999999ap-4", "inf", "nan", "0x0.0000000000001p-1022"]
    xy_t, moving, _ = K.stereo_window()
    np.savez(fin, xy_t=xy_t, fc=K.FC, cc=K.CC, baseline=K.BASELINE)
    assert run_bundle.main([fin, fout, "--host", "--stereo", "--noiter", "5"]) == 0
    capsys.readouterr()
    split, X, left, right, fit = K.chain_host(xy_t)
    want = B.adjust_window_host(X, np.stack([left, right]), K.CAM, offset=BC.OFFSET, mask=split["words"], init=fit["G"],
                                noiter=5)
    with np.load(fout) as z:
        assert z["G"].tobytes() == want["G"].tobytes() and z["X"].tobytes() == want["X"].tobytes()
        assert z["fit_G"].tobytes() == fit["G"].tobytes() and np.array_equal(z["inliers"], split["inliers"])


def test_native_caller_compiles_against_the_facade():
    """tests/cxx/bundle_driver.cpp (CTR::BundleClass of include/ctr_shim.hpp) builds with plain g++ -std=c++11 and links
    against libictr_hip.so."""
    import __graft_entry__ as g
    g.build()
    exe = os.path.join(ROOT, "tests", "cxx", "bundle_driver")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        exe + ".cpp", "-L" + os.path.join(ROOT, "invcompcamtrack_amd"), "-l:libictr_hip.so",
                        "-Wl,-rpath,$ORIGIN/../../invcompcamtrack_amd"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
