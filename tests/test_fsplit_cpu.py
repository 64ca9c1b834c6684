"""The static split on the host: fit_f8 / epiline_dist against an independent 50-digit judge (tests/fsplit_mp.py), the
crafted inputs reaching their branches, whole host runs, the track-window helpers and the CLI."""
import numpy as np
import pytest

import fsplit_cases as K
import fsplit_mp as J
from invcompcamtrack_amd import fsplit as S

N_JUDGE, TRIALS_PER_SCENE, THRESH = 200, 50, 2.0  # 6 scenes x 50 trials = 300 judged fits
BAR = 1e-8         # px, host against judge (the bar of the RANSAC judge for R and T)
MARGIN = 1e-6      # px: no judge distance this near to the threshold
ILL = 1e-6         # sigma_8 / sigma_1 of the design matrix below this: the trial may be left out ...
ILL_SHARE = 0.01   # ... for at most this share of the trials


@pytest.fixture(scope="module")
def judged():
    """Per trial: (scene, trial, host distances, judge distances as f64, judge distances' margin to THRESH, ratio)."""
    rows = []
    for si, (static, noise) in enumerate(K.SCENES):
        pairs, _ = K.scene(N_JUDGE, 1, static, noise, seed=100 + si)
        for t in range(TRIALS_PER_SCENE):
            idx = S.draw_indices_n(7, t, N_JUDGE, 8)
            xa, xb = pairs[0, 0:2, idx].reshape(8, 2), pairs[0, 2:4, idx].reshape(8, 2)
            Fj, ratio = J.fit(xa[:, 0], xa[:, 1], xb[:, 0], xb[:, 1])
            dj = J.dist(Fj, *pairs[0])
            F = S.fit_f8(xa, xb)
            assert F is not None
            dh = S.epiline_dist(F, pairs[0, 0:2].T, pairs[0, 2:4].T)
            with J.mp.workdps(J.DPS):
                err = max(abs(J.mp.mpf(float(a)) - b) for a, b in zip(dh, dj))
                margin = min(abs(b - THRESH) for b in dj)
            rows.append(dict(scene=si, trial=t, dh=dh, dj=np.array([float(b) for b in dj]), err=float(err),
                             margin=float(margin), ratio=float(ratio)))
    return rows


def _compared(judged):
    keep = [r for r in judged if r["ratio"] >= ILL]
    assert len(judged) >= 300 and len(judged) - len(keep) <= ILL_SHARE * len(judged)
    return keep


def test_fit_and_distance_against_the_judge(judged):
    """Measured: worst |d_host - d_judge| 1.9e-9 px over 300 trials (0 left out, smallest sigma_8 / sigma_1 8.1e-5);
    with 3 sweeps instead of 5 it is 3.2e-4 px, with 4 it is already 1.9e-9 (DESIGN.md §4 "Static split")."""
    keep = _compared(judged)
    worst = max(keep, key=lambda r: r["err"])
    print("\nworst |d_host - d_judge| %.3e px (scene %d trial %d), %d of %d compared, smallest ratio %.3e"
          % (worst["err"], worst["scene"], worst["trial"], len(keep), len(judged), min(r["ratio"] for r in judged)))
    assert worst["err"] <= BAR


def test_sweep_count_is_the_smallest_that_holds_plus_one(judged):
    """SWEEPS - 1 sweeps hold the bar on the judged trials, SWEEPS - 2 do not."""
    def worst(sweeps):
        w = 0.0
        for si, (static, noise) in enumerate(K.SCENES):
            pairs, _ = K.scene(N_JUDGE, 1, static, noise, seed=100 + si)
            for r in (r for r in _compared(judged) if r["scene"] == si):
                idx = S.draw_indices_n(7, r["trial"], N_JUDGE, 8)
                F = S.fit_f8(pairs[0, 0:2, idx].reshape(8, 2), pairs[0, 2:4, idx].reshape(8, 2), sweeps=sweeps)
                w = max(w, np.abs(S.epiline_dist(F, pairs[0, 0:2].T, pairs[0, 2:4].T) - r["dj"]).max())
        return w
    assert worst(S.SWEEPS - 1) <= BAR < worst(S.SWEEPS - 2)


def test_inlier_sets_against_the_judge(judged):
    keep = _compared(judged)
    near = [r for r in keep if r["margin"] <= MARGIN]
    assert not near, "a judge distance within 1e-6 px of the threshold: pick another seed"
    for r in keep:
        assert np.array_equal(r["dh"] < THRESH, r["dj"] < THRESH), (r["scene"], r["trial"])


# ---------------------------------------------------------------- crafted inputs reach their branches
def test_coincident_points_fail_on_the_mean_distance():
    pairs, _ = K.coincident()
    idx = S.draw_indices_n(0, 0, 8, 8)
    assert S._normalise(pairs[0, 0, idx].tolist(), pairs[0, 1, idx].tolist()) is None
    res = S.split_static_host(pairs, 5, 2.0, 0, detail=True)
    assert not res["status"].any() and res["best_count"] == 0 and res["best_trial"] == 0
    assert np.isnan(res["F"]).all() and np.isnan(res["dd"]).all() and not res["mask"].any()


def test_duplicate_point_fails_on_an_exactly_zero_pivot():
    pairs, _ = K.duplicate()
    idx = S.draw_indices_n(0, 0, 8, 8)
    xa, ya, xb, yb = (pairs[0, c, idx].tolist() for c in range(4))
    na, nb = S._normalise(xa, ya), S._normalise(xb, yb)
    assert na is not None and nb is not None
    A = [[nb[0][r] * na[0][r], nb[0][r] * na[1][r], nb[0][r], nb[1][r] * na[0][r], nb[1][r] * na[1][r], nb[1][r],
          na[0][r], na[1][r], 1.0] for r in range(8)]
    assert S._null_vector(A) is None
    assert not S.split_static_host(pairs, 5, 2.0, 0, detail=True)["status"].any()


def test_nan_drawn_fails_and_nan_not_drawn_is_never_an_inlier():
    pairs, _ = K.nan_drawn()
    assert not S.split_static_host(pairs, 5, 2.0, 0, detail=True)["status"].any()
    pairs, (i_nan, i_inf) = K.nan_not_drawn(3, 0)
    res = S.split_static_host(pairs, 1, 50.0, 3, detail=True)
    assert res["status"][0] == 1 and res["best_count"] == 198
    assert not res["mask"][i_nan] and not res["mask"][i_inf] and np.isnan(res["dd"][i_nan])
    assert res["dd"][i_inf] == np.inf or np.isnan(res["dd"][i_inf])


def test_fronto_parallel_dyadic_set_is_rank_deficient():
    """Every entry of the elimination is exact here, so the deficiency shows as pivots that are exactly 0: trials fail,
    and a trial that does not fail (a sample whose pivots stay non-zero) holds all points to its lines."""
    pairs, _ = K.fronto_parallel()
    res = S.split_static_host(pairs, 40, 1e-6, 0, detail=True)
    assert (res["status"] == 0).sum() >= 1
    ok = res["status"] == 1
    assert (res["cnt"][ok] == pairs.shape[2]).all()


def test_tie_goes_to_the_lowest_trial():
    pairs, thresh = K.tie()
    res = S.split_static_host(pairs, 12, thresh, 0, detail=True)
    full = np.nonzero(res["cnt"] == pairs.shape[2])[0]
    assert full.size >= 2 and res["best_trial"] == full[0] and res["best_count"] == pairs.shape[2]


# ---------------------------------------------------------------- whole runs
def test_best_trial_recovers_the_static_points():
    pairs, moving = K.scene(300, 3, 0.7, 0.0, seed=41)
    res = S.split_static_host(pairs, 100, 2.0, 0)
    assert np.array_equal(res["mask"], ~moving)
    assert res["best_count"] == int((~moving).sum()) == res["inliers"].size
    again = S.split_static_host(pairs, 100, 2.0, 0)
    for k in ("dd", "F", "words", "draws"):
        assert res[k].tobytes() == again[k].tobytes(), k
    assert again["best_trial"] == res["best_trial"]
    other = S.split_static_host(pairs, 100, 2.0, 1)
    assert not np.array_equal(other["draws"], res["draws"])


def test_draw_indices_n_extends_the_pose_sampler_rule():
    from invcompcamtrack_amd import ransac
    for seed, t, n in ((0, 0, 50), (5, 17, 9), (1 << 40, 3, 1000)):
        eight = S.draw_indices_n(seed, t, n, 8)
        assert len(set(eight)) == 8 and eight[:4] == ransac.draw_indices(seed, t, n)
    assert len(S.draw_indices_n(0, 0, 7, 8)) == 7  # 7 points never give 8


@pytest.mark.parametrize("bsize", [10, 7, 2, 3])
def test_pairs_from_tracks_follow_the_script_indexing(bsize):
    rng = np.random.default_rng(bsize)
    tr = rng.uniform(0, 500, (30, 2, bsize)).astype(np.float32)
    tr[4, 1, bsize - 1] = np.nan
    tr[11, 0, 0] = np.nan
    pairs, rows = S.pairs_from_tracks(tr)
    keep = [i for i in range(30) if i not in (4, 11)]
    assert rows.tolist() == keep and pairs.shape == (bsize // 2, 4, 28) and pairs.dtype == np.float64
    for fr in range(bsize // 2):
        fr_f = fr + int(np.ceil(bsize / 2.0))  # run_test_OF_track.py:323
        assert np.array_equal(pairs[fr], np.stack([tr[keep, 0, fr], tr[keep, 1, fr], tr[keep, 0, fr_f],
                                                   tr[keep, 1, fr_f]]).astype(np.float64))
    xy = rng.uniform(0, 500, (20, 4, bsize))
    xy[7, 3, 0] = np.nan
    sp, srows = S.pairs_from_stereo_tracks(xy)
    keep = [i for i in range(20) if i != 7]
    assert srows.tolist() == keep and sp.shape == (2 * (bsize // 2), 4, 19)
    for fr in range(bsize // 2):
        fr_f = fr + int(np.ceil(bsize / 2.0))
        assert np.array_equal(sp[2 * fr, 0:2], xy[keep, 0:2, fr].T) and np.array_equal(sp[2 * fr, 2:4], xy[keep, 2:4, fr_f].T)
        assert np.array_equal(sp[2 * fr + 1, 0:2], xy[keep, 2:4, fr].T)
        assert np.array_equal(sp[2 * fr + 1, 2:4], xy[keep, 0:2, fr_f].T)


def test_cli_round_trips_on_the_host(tmp_path):
    from invcompcamtrack_amd import run_static_split
    pairs, moving = K.scene(150, 2, 0.7, 0.0, seed=43)
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(fin, pairs=pairs)
    assert run_static_split.main([fin, fout, "--host", "--ntrials", "60", "--seed", "2"]) == 0
    want = S.split_static_host(pairs, 60, 2.0, 2)
    with np.load(fout) as z:
        assert np.array_equal(z["inliers"], want["inliers"]) and z["dd"].tobytes() == want["dd"].tobytes()
        assert z["F"].tobytes() == want["F"].tobytes() and int(z["best_trial"]) == want["best_trial"]
        assert np.array_equal(z["draws"], want["draws"])
    assert np.array_equal(want["mask"], ~moving)
    # a track window with a lost row: the inlier indices are those of the input rows
    tr = np.stack([pairs[0, 0:2].T, pairs[1, 2:4].T], axis=2)  # (N, 2, 2): one pair (frame 0, frame 1)
    tr[5, 0, 1] = np.nan
    np.savez(fin, tracks=tr)
    assert run_static_split.main([fin, fout, "--host", "--ntrials", "60"]) == 0
    with np.load(fout) as z:
        assert 5 not in z["inliers"] and z["rows"].size == 149 and set(z["inliers"]) <= set(z["rows"].tolist())


def test_native_caller_compiles_against_the_facade():
    """tests/cxx/fsplit_driver.cpp (CTR::StaticSplitClass of include/ctr_shim.hpp) builds with plain g++ -std=c++11 and
    links against libictr_hip.so; without a device it fails loudly."""
    import os
    import subprocess
    import __graft_entry__ as g
    import invcompcamtrack_amd as ic
    g.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "cxx", "fsplit_driver")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(root, "include"), "-o", exe,
                        exe + ".cpp", "-L" + os.path.join(root, "invcompcamtrack_amd"), "-l:libictr_hip.so",
                        "-Wl,-rpath,$ORIGIN/../../invcompcamtrack_amd"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    if ic.device_count() < 1:
        with pytest.raises(ic.IctrError, match="no usable HIP device"):
            S.StaticSplitter(100, 2)


def test_shared_header_on_the_host_equals_the_restatement(tmp_path):
    """csrc/ictr_fsplit_hd.h compiled as plain C++ (tests/cxx/fsplit_hd_host.cpp, -ffp-contract=off, address and
    undefined-behaviour sanitizers): F, the status and a distance of 1200 scene samples and of the crafted sets carry the
    bits of fit_f8 / epiline_dist, and the sanitizers stay silent."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "cxx", "fsplit_hd_host")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        "-I" + os.path.join(root, "invcompcamtrack_amd", "csrc"), "-o", exe, exe + ".cpp"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    samples = []
    for si, (static, noise) in enumerate(K.SCENES):
        pairs, _ = K.scene(200, 2, static, noise, seed=100 + si)
        for t in range(100):
            idx = S.draw_indices_n(3, t, 200, 8)
            samples += [pairs[p][:, idx].reshape(-1) for p in range(2)]
    for maker in (K.coincident, K.duplicate, K.nan_drawn, K.fronto_parallel):
        pairs, _ = maker()
        for t in range(20):
            samples.append(pairs[0][:, S.draw_indices_n(3, t, pairs.shape[2], 8)].reshape(-1))
    smp = np.array(samples)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    smp.tofile(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    got = np.fromfile(fout).reshape(-1, 11)
    assert len(got) == len(smp)
    failed = 0
    for s8, g in zip(smp, got):
        F = S._fit_f8_list(*s8.reshape(4, 8).tolist())
        ok = float(F[0] == F[0])
        failed += ok == 0.0
        d = S._dist(F, s8[0:1], s8[8:9], s8[16:17], s8[24:25])[0]
        assert np.array_equal(np.array(F + [ok, d]).view(np.uint64), g.view(np.uint64))
    assert 60 <= failed < len(smp) // 10


def test_shared_draw_header_on_the_host_equals_draw_indices_n(tmp_path):
    """csrc/ictr_draw_hd.h compiled as plain C++ (tests/cxx/draw_hd_host.cpp, address and undefined-behaviour
    sanitizers): ran_seed and the indices of ran_draw<4> / ran_draw<8> are those of draw_indices_n, exactly, at the
    smallest and largest n, at trial indices around 2^31, 2^32 and 2^40 and at the seeds' corners; where n < K the
    draw ends with n indices and -1 in the rest. (That it ends after kRanMaxDraws draws and not another number is not
    seen from outside: every index of so small an n is drawn long before.) The sanitizers stay silent."""
    import os
    import subprocess
    from invcompcamtrack_amd import _hostmath as H
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "cxx", "draw_hd_host")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                        "-Werror", "-Wno-unknown-pragmas", "-I" + os.path.join(root, "invcompcamtrack_amd", "csrc"),
                        "-o", exe, exe + ".cpp"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    recs = [(seed, t, n, k) for k in (4, 8) for n in (4, 7, 8, 9, 64, 1 << 22, 1 << 24)
            for t in (0, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 40) - 1)
            for seed in (0, 1, 1 << 63, (1 << 64) - 1)]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.array(recs, np.uint64).tofile(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    got = np.fromfile(fout, np.int64).reshape(-1, 10)
    assert len(got) == len(recs) == 336
    for (seed, t, n, k), g in zip(recs, got):
        idx = S.draw_indices_n(seed, t, n, k)
        assert len(idx) == min(n, k) and len(set(idx)) == len(idx)  # 1024 draws reach every index of a small n
        assert int(g[0]) & H.M64 == H.mix(seed)
        assert g[1] == len(idx) and g[2:].tolist() == idx + [-1] * (8 - len(idx)), (seed, t, n, k)
    assert S.draw_indices_n(0, 0, 7, 8, max_draws=1 << 16) == S.draw_indices_n(0, 0, 7, 8)  # seven, however long
