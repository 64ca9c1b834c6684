"""The window camera RANSAC on the host: csrc/ictr_camransac_hd.h and csrc/ictr_p3p_hd.h as plain C++ against the
restatement of camransac.py and ransac.py (bit for bit), the restatement's score against an independent statement in matrix
form, the usefulness of the step on the seeded stereo windows, the crafted inputs reaching their branches, the pipeline on
the golden windows and the CLI."""
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import camfit_cases as K
import camransac_cases as CR
import ransac_cases as RC
from invcompcamtrack_amd import camfit as F
from invcompcamtrack_amd import camransac as R
from invcompcamtrack_amd import ransac as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-8     # px, restatement against the judge: fsplit's bar
MARGIN = 1e-6  # px, the judged trials keep every distance this far from thresh


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---------------------------------------------------------------- 1. header == restatement
@pytest.fixture(scope="module")
def hd_host():
    exe = os.path.join(ROOT, "tests", "cxx", "camransac_hd_host")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        "-I" + os.path.join(ROOT, "invcompcamtrack_amd", "csrc"), "-o", exe, exe + ".cpp"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run_hd(exe, tmp_path, c):
    X, xy = c["X"], c["xy"]
    n, (S, Fr) = X.shape[1], xy.shape[:2]
    W = (n + 63) // 64
    words = F._words_of(c["mask"], n)
    off = np.zeros(3) if c["offset"] is None else np.asarray(c["offset"], np.float64)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([n, Fr, S, words is not None, c["ntrials"], c["seed"]], np.int64).tobytes())
        f.write(np.array(F._as_cam(c["cam"]) + tuple(off) + (c["thresh"],)).tobytes())
        f.write(X.tobytes() + xy.tobytes() + (b"" if words is None else words.tobytes()))
    r = subprocess.run([exe, "run", fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    raw = np.fromfile(fout, np.uint64)
    rec = 6 + 12 * Fr + n + W
    assert raw.size == rec * c["ntrials"] + 2
    t = raw[:-2].reshape(c["ntrials"], rec)
    return dict(status=t[:, 0].astype(np.int64), draws=t[:, 1:5].view(np.int64), cnt=t[:, 5].astype(np.int64),
                G=t[:, 6:6 + 12 * Fr], dd=t[:, 6 + 12 * Fr:6 + 12 * Fr + n], words=t[:, 6 + 12 * Fr + n:],
                best=raw[-2:].view(np.int64))


def _same_as_host(got, h, thr, what):
    T = len(h["status"])
    assert np.array_equal(got["status"], h["status"]), what
    assert np.array_equal(got["draws"], h["all_draws"]), what
    assert np.array_equal(got["G"], _bits(h["all_G"]).reshape(T, -1)), what
    assert np.array_equal(got["dd"], _bits(h["all_dd"])), what
    with np.errstate(invalid="ignore"):
        thr_words = np.array([R._pack_words(h["counts"] & (d < thr)) for d in h["all_dd"]])
    assert np.array_equal(got["cnt"], h["cnt"]) and np.array_equal(got["words"], thr_words), what
    assert got["best"][0] == h["best_trial"] and got["best"][1] == h["best_count"], what


def test_shared_header_on_the_host_equals_the_restatement(hd_host, tmp_path):
    """csrc/ictr_camransac_hd.h compiled as plain C++ (tests/cxx/camransac_hd_host.cpp, -ffp-contract=off, address and
    undefined-behaviour sanitizers) carries camransac.py's bits for status, draws, every frame's G, counts, words and dd
    over 64 trials of the seeded windows and of every crafted case -- with the running maximum kept on rx^2 + ry^2 and one
    root per point, where the restatement takes a root per distance; the sanitizers stay silent."""
    for key in CR.seeded_cases():
        _same_as_host(_run_hd(hd_host, tmp_path, CR.seeded(*key)), CR.host_seeded(*key), CR.seeded(*key)["thresh"], key)
    for name in CR.CRAFTED:
        _same_as_host(_run_hd(hd_host, tmp_path, CR.crafted(name)), CR.host(name), CR.crafted(name)["thresh"], name)


def test_solver_text_on_the_host_equals_the_restatement(hd_host, tmp_path):
    """p3p_lambda_twist of csrc/ictr_p3p_hd.h as host C++ gives ransac.p3p's solutions bit for bit, in its order, on every
    ordered triple of the first four matches of the crafted sets of ransac_cases.py, the LAMBDA_TWIST_LIMIT ones included."""
    cases, want = [], []
    for fn in RC.CRAFTED:
        c = fn()
        assert c["kc"] == 0.0
        (fx, fy), (cx, cy) = c["fc"], c["cc"]
        for tri in itertools.permutations(range(4), 3):
            y = []
            for q in tri:
                bx, by = (c["x"][0, q] - cx) / fx, (c["x"][1, q] - cy) / fy
                s = 1.0 / math.sqrt(bx * bx + by * by + 1.0)
                y.append([bx * s, by * s, s])
            x = [[float(c["X"][k, q]) for k in range(3)] for q in tri]
            cases.append(np.array(y + x).reshape(18))
            want.append((c["name"], tri, RS.p3p(y, x)))
    assert RC.LAMBDA_TWIST_LIMIT <= {fn().get("name") for fn in RC.CRAFTED}
    fin, fout = str(tmp_path / "p_in.bin"), str(tmp_path / "p_out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([len(cases)], np.int64).tobytes() + np.array(cases).tobytes())
    r = subprocess.run([hd_host, "p3p", fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    got = np.fromfile(fout, np.uint64).reshape(len(cases), 49)
    nsol = 0
    for g, (name, tri, sols) in zip(got, want):
        assert int(g[0]) == len(sols) <= 4, (name, tri)
        for k, (Rm, T) in enumerate(sols):
            assert np.array_equal(g[1 + 12 * k:13 + 12 * k], _bits(list(Rm) + list(T))), (name, tri, k)
        nsol += len(sols)
    assert nsol > 50


# ---------------------------------------------------------------- 2. an independent statement of the score
def _judge_dd(G, X, xy, cam, off):
    """The largest reprojection distance of every point, in matrix form."""
    (fx, fy), (cx, cy) = cam
    Kc = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    d = []
    for f in range(xy.shape[1]):
        for s in range(xy.shape[0]):
            h = Kc @ (G[f, :, :3] @ X + (G[f, :, 3] + s * off)[:, None])
            d.append(np.hypot(h[0] / h[2] - xy[s, f, 0], h[1] / h[2] - xy[s, f, 1]))
    return np.max(d, axis=0)


@pytest.fixture(scope="module")
def scenes():
    """The two wrong-depth scenes with 100 trials of the restatement, computed once."""
    out = {}
    for seed in (700, 701):
        xy_t, moving, moved, G = CR.wrong_depth_window(seed)
        X, xy = CR.stereo_inputs(xy_t)
        out[seed] = dict(xy_t=xy_t, moving=moving, moved=moved, G=G, X=X, xy=xy,
                         host=R.window_ransac_host(X, xy, CR.CAM, CR.OFFSET, ntrials=100, thresh=2.0, seed=0, detail=True))
    return out


def test_restatement_against_an_independent_score(scenes):
    """Measured: the worst |d_host - d_judge| over every point of the 198 successful trials of both scenes (118 800
    distances, all finite, the largest 7.7e6 px) is 1.4e-9 px (bar 1e-8, fsplit's), 2.3e-13 relative to the distance; no
    trial has a distance within 1e-6 px of thresh (the cap is 1 %, 2 trials)."""
    worst, close, judged = 0.0, 0, 0
    for sc in scenes.values():
        h = sc["host"]
        for g in range(100):
            if not h["status"][g]:
                continue
            G = h["all_G"][g].reshape(-1, 3, 4)
            dj = _judge_dd(G, sc["X"], sc["xy"], CR.CAM, CR.OFFSET)
            if np.min(np.abs(dj[h["counts"]] - 2.0)) < MARGIN:
                close += 1
                continue
            judged += 1
            assert np.array_equal(np.nonzero(h["counts"] & (dj < 2.0))[0],
                                  np.nonzero(h["counts"] & (h["all_dd"][g] < 2.0))[0]), g
            assert np.isfinite(dj).all() and np.isfinite(h["all_dd"][g]).all()
            worst = max(worst, float(np.max(np.abs(dj - h["all_dd"][g]))))
    print(f"worst |d_host - d_judge| = {worst:.3e} px over {judged} trials, {close} left out")
    assert close <= 2 and judged >= 150
    assert worst <= BAR


# ---------------------------------------------------------------- 3. usefulness
def _pose_err(G, Gt):
    return float(np.max(np.abs(np.asarray(G) - Gt)))


def test_usefulness_on_the_stereo_window():
    """stereo_window() with the defaults (100 trials, 2 px, seed 0). Measured: 352 static inliers, no moving one; the fit
    from the RANSAC poses on the RANSAC inliers converges in at most 6 iterations; its max |G - G_true| is 0.0026 against
    chain_host's 0.0028."""
    xy_t, moving, Gt = K.stereo_window()
    X, xy = CR.stereo_inputs(xy_t)
    r = R.window_ransac_host(X, xy, CR.CAM, CR.OFFSET)
    print("inliers", r["best_count"], "moving among them", int(r["mask"][moving].sum()))
    assert not r["mask"][moving].any() and int(r["mask"][~moving].sum()) >= 300
    fit = F.fit_cameras_host(X, xy[0], CR.CAM, mask=r["words"], init=r["G"])
    _, _, _, _, chain = K.chain_host(xy_t)
    print("iters", fit["iters"], "err", _pose_err(fit["G"], Gt), "chain", _pose_err(chain["G"], Gt))
    assert (fit["status"] == F.CONVERGED).all() and (fit["iters"] <= 10).all()
    assert _pose_err(fit["G"], Gt) <= _pose_err(chain["G"], Gt)


def test_usefulness_on_wrong_depths(scenes):
    """A fifth of the static points with a wrong depth (right x of frame 0 moved by 5 px). Measured, scene seeds 700 / 701:
    chain_host keeps 40 / 30 of them, the RANSAC none and no moving point, 280 / 302 others; pose error after the fit
    0.0024 / 0.0017 against 0.0091 / 0.0030; worst right-camera mean 0.50 / 0.51 px against 1.44 / 1.15 px."""
    for seed, sc in scenes.items():
        r, moving, moved = sc["host"], sc["moving"], sc["moved"]
        assert not r["mask"][moving].any() and not r["mask"][moved].any()
        assert int(r["mask"][~moving & ~moved].sum()) >= 250
        split, Xc, left, right, chain = K.chain_host(sc["xy_t"])
        assert int(split["mask"][moved].sum()) >= 20
        fit = F.fit_cameras_host(sc["X"], sc["xy"][0], CR.CAM, mask=r["words"], init=r["G"])
        e_r, _ = F.reprojection_errors_host(sc["X"], sc["xy"][1], CR.CAM, fit["G"], mask=r["words"], offset=CR.OFFSET)
        e_c, _ = F.reprojection_errors_host(Xc, right, CR.CAM, chain["G"], mask=split["words"], offset=CR.OFFSET)
        print(seed, "kept by chain", int(split["mask"][moved].sum()), "others", int(r["mask"][~moving & ~moved].sum()),
              "err", _pose_err(fit["G"], sc["G"]), _pose_err(chain["G"], sc["G"]), "right", e_r.max(), e_c.max())
        assert _pose_err(fit["G"], sc["G"]) < _pose_err(chain["G"], sc["G"])
        assert e_r.max() < e_c.max()


# ---------------------------------------------------------------- 4. crafted cases reach their branches
def _failed_with_all_draws(h):
    return [g for g in range(len(h["status"])) if not h["status"][g] and (h["all_draws"][g] >= 0).all()]


def test_drawn_points_that_do_not_count_fail_the_trial():
    for name, bad in (("drawn_masked", 2), ("drawn_nan", 3)):
        h = CR.host(name)
        assert not h["counts"][bad] and h["counts"].sum() == 5
        hit = [g for g in _failed_with_all_draws(h) if bad in h["all_draws"][g]]
        assert hit and all(np.isnan(h["all_G"][g]).all() and h["cnt"][g] == 0 for g in hit)
        assert all(bad not in h["all_draws"][g] for g in np.nonzero(h["status"])[0]) and h["status"].any()
        assert not h["mask"][bad] and h["best_trial"] >= 0


def test_nan_on_the_right_side_of_one_frame():
    h = CR.host("nan_right_one_frame")
    assert not h["counts"][7] and h["counts"].sum() == 39 and not h["mask"][7]
    assert np.isnan(h["dd"][7]) and _bits(h["dd"][7:8])[0] == 0x7FF8000000000000
    assert h["best_count"] >= 20


def test_one_degenerate_frame_fails_the_trial():
    h = CR.host("degenerate_frame")
    c = CR.crafted("degenerate_frame")
    hit = [g for g in _failed_with_all_draws(h) if {0, 1, 2} <= set(h["all_draws"][g])]
    assert hit
    for g in hit:
        G = h["all_G"][g]
        assert np.isnan(G[1]).all() and np.isfinite(G[0]).all() and np.isfinite(G[2]).all() and h["cnt"][g] == 0
        x2 = [[c["xy"][0, 1, 0, i], c["xy"][0, 1, 1, i], 1.0] for i in h["all_draws"][g]]
        P = [[float(c["X"][k, i]) for k in range(3)] for i in h["all_draws"][g]]
        assert RS.is_degenerate(P, x2)
    assert h["status"].any()


def test_every_trial_failing_gives_the_empty_result():
    h = CR.host("all_fail")
    assert not h["status"].any() and h["best_trial"] == -1 and h["best_count"] == 0
    assert np.isnan(h["G"]).all() and np.isnan(h["p"]).all() and np.isnan(h["dd"]).all()
    assert not h["words"].any() and not h["mask"].any() and h["inliers"].size == 0 and (h["draws"] == -1).all()


def test_lowest_trial_wins_a_tie():
    h = CR.host("exact_all_inliers")
    ok = np.nonzero(h["status"])[0]
    n = CR.crafted("exact_all_inliers")["X"].shape[1]
    assert ok.size >= 2 and (h["cnt"][ok] == n).all()
    assert h["best_trial"] == ok[0] and h["best_count"] == n and h["mask"].all()


def test_one_side_and_one_frame():
    for name in ("one_side", "one_frame"):
        h, c = CR.host(name), CR.crafted(name)
        assert h["G"].shape == (c["xy"].shape[1], 3, 4) and h["best_count"] >= 40
        assert not h["mask"][-14:].any() or name == "one_frame"  # one frame: the first, where no point is displaced
    with pytest.raises(ValueError):
        c = CR.crafted("one_frame")
        R.window_ransac_host(c["X"], c["xy"], c["cam"], None)   # two sides need the offset


def test_depth_zero_in_one_frame():
    h = CR.host("depth_zero")
    assert h["counts"][9] and not h["mask"][9] and not (h["dd"][9] < 1e3)
    for g in np.nonzero(h["status"])[0]:
        assert not (h["all_dd"][g][9] < 1e3)
    assert h["best_count"] >= 25


def test_arguments():
    c = CR.crafted("one_side")
    for kw in (dict(ntrials=0), dict(ntrials=(1 << 20) + 1), dict(thresh=float("nan"))):
        with pytest.raises(ValueError):
            R.window_ransac_host(c["X"], c["xy"], c["cam"], **kw)
    with pytest.raises(ValueError):
        R.window_ransac_host(c["X"][:, :3], c["xy"][..., :3], c["cam"])
    with pytest.raises(ValueError):
        R.window_ransac_host(c["X"], np.zeros((3, 2, 2, 70)), c["cam"], CR.OFFSET)


# ---------------------------------------------------------------- 5. pipeline and CLI on the host
PIPE_TIGHT = 0.05  # px: on the golden windows the winner keeps a real share of the points


@pytest.mark.parametrize("name", ["small_disp", "large_disp", "odd_long", "two_frames"])
def test_pipeline_on_the_golden_windows(name):
    """window_ransac_cameras_host: shapes, dtypes and the consistency of its parts (the golden windows' geometry is not
    rigid, so no counts are asserted): the RANSAC's keys are window_ransac_host's on the window's points, the fit is
    fit_cameras_host from the RANSAC poses on the RANSAC words."""
    from invcompcamtrack_amd import windowcams as W
    from test_stereotrack_cpu import fields, golden
    c = golden()[name]
    for thresh in (2.0, PIPE_TIGHT):
        r = W.window_ransac_cameras_host(*fields(c), K.CAM, K.BASELINE, thresh=thresh, bundle=True, tracks=True)
        m, b = len(c["rows"]), c["xy_t"].shape[2]
        assert r["m"] == m and r["xy_t"].tobytes() == c["xy_t"].tobytes()
        X, xy = CR.stereo_inputs(c["xy_t"])
        ran = R.window_ransac_host(X, xy, K.CAM, CR.OFFSET, ntrials=100, thresh=thresh)
        for k in W._RANSAC_KEYS:
            assert np.asarray(r[k]).tobytes() == np.asarray(ran[k]).tobytes(), k
        assert r["G_ransac"].tobytes() == ran["G"].tobytes() and r["p_ransac"].tobytes() == ran["p"].tobytes()
        assert r["G"].shape == (b, 3, 4) and r["p"].shape == (b, 6) and r["dd"].shape == (m,) and r["mask"].dtype == bool
        assert r["status"].dtype == np.int32 and r["n"].dtype == np.int64 and r["err_left"].shape == r["err_right"].shape == (b,)
        print(name, thresh, "keeps", r["best_count"], "of", m, "trial", r["best_trial"], "status", r["status"])
        if r["best_trial"] < 0:
            assert (r["status"] == F.FEW_OBS).all() and np.isnan(r["err_left"]).all() and np.isnan(r["G"]).all()
            assert r["ba"] is None and np.isnan(r["err_right_ba"]).all()
        else:
            fit = F.fit_cameras_host(X, xy[0], K.CAM, mask=ran["words"], init=ran["G"])
            assert r["G"].tobytes() == fit["G"].tobytes() and np.array_equal(r["n"], np.full(b, r["best_count"]))
            assert r["ba"]["G"].shape == (b, 3, 4) and r["err_left_ba"].shape == (b,)


def test_pipeline_refusals_and_the_path_without_a_successful_trial(monkeypatch):
    from invcompcamtrack_amd import windowcams as W
    from test_stereotrack_cpu import fields, golden
    with pytest.raises(ValueError, match="bsize"):
        W.window_ransac_cameras_host(*fields(golden()["one_frame"]), K.CAM, K.BASELINE)
    c = golden()["two_frames"]
    with pytest.raises(TypeError):
        W.window_ransac_cameras_host(*fields(c), K.CAM, K.BASELINE, no_such_parameter=1)
    # every trial failing, as all_fail makes it: nothing is fitted
    empty = CR.host("all_fail")
    monkeypatch.setattr(R, "window_ransac_host", lambda *a, **k: empty)
    monkeypatch.setattr(F, "fit_cameras_host", lambda *a, **k: pytest.fail("a fit was started"))
    r = W.window_ransac_cameras_host(*fields(c), K.CAM, K.BASELINE, bundle=True)
    assert r["best_trial"] == -1 and (r["status"] == F.FEW_OBS).all() and r["status"].shape == (2,)
    assert np.isnan(r["err_left"]).all() and np.isnan(r["err_right"]).all() and np.isnan(r["G"]).all()
    assert r["ba"] is None and not r["iters"].any() and not r["n"].any()


def test_cli_on_the_host(tmp_path, capsys):
    from invcompcamtrack_amd import run_window_ransac
    from invcompcamtrack_amd import windowcams as W
    from test_stereotrack_cpu import fields, golden
    g = golden()["two_frames"]
    zin, zout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(zin, fc=K.FC, cc=K.CC, baseline=K.BASELINE, **{k: g[k] for k in ("disp_lr", "disp_rl", "flow_l", "flow_r")})
    assert run_window_ransac.main([zin, zout, "--host", "--thresh", str(PIPE_TIGHT), "--ntrials", "40", "--seed", "3"]) == 0
    want = W.window_ransac_cameras_host(*fields(g), K.CAM, K.BASELINE, thresh=PIPE_TIGHT, ntrials=40, seed=3)
    with np.load(zout) as z:
        assert sorted(z.files) == sorted(want)
        for k in want:
            assert z[k].tobytes() == np.asarray(want[k]).tobytes(), k
    assert "inliers of trial %d" % want["best_trial"] in capsys.readouterr().out
    assert run_window_ransac.main([zin, zout, "--host", "--th_abs", "0.0"]) == 2
