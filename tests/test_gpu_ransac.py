"""RANSAC pose sampling on the device (ictr_ransac.hip) against the NumPy restatement, and the whole
func_ransac_fitcameras_odom.m through fit_cameras_odom, the CLI and the C++ facade."""
import os
import subprocess

import numpy as np
import pytest

import invcompcamtrack_amd as ic
from invcompcamtrack_amd import io_formats as iof
from invcompcamtrack_amd import ransac as R
from invcompcamtrack_amd import run_ransac, run_track_nposes, synth
from ransac_cases import matches as _matches

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FC, CC, WH = [800.0, 780.0], [320.0, 240.0], (640, 480)


def _check_margins(host, thr):
    for m_thr, e0, e1 in host["margins"]:
        assert m_thr > 1e-6, "a match lies within 1e-6 px of inlthresh: pick another seed"
        assert e1 - e0 > 1e-6 * (1.0 + e0), "two P3P roots reproject the 4th match alike: pick another seed"


def _same(dev, host):
    assert dev["accepted"] == host["accepted"] and dev["trials_used"] == host["trials_used"]
    assert np.array_equal(dev["trials"], host["trials"]) and np.array_equal(dev["draws"], host["draws"])
    assert len(dev["p"]) == len(host["p"])
    if len(dev["p"]):
        assert np.abs(dev["p"] - host["p"]).max() <= 1e-8
        assert np.abs(dev["R"] - host["R"]).max() <= 1e-8
        assert np.abs(dev["t"] - host["t"]).max() <= 1e-8
    assert all(np.array_equal(a, b) for a, b in zip(dev["inl"], host["inl"]))
    assert np.array_equal(dev["inl_cnt"], host["inl_cnt"])


CASES = [(n, r, kc) for n in (7, 64, 65, 1000, 5000) for r in (1.0, 0.6, 0.3) for kc in (0.0, -0.05)]


@pytest.mark.parametrize("n,ratio,kc", CASES)
def test_device_equals_host(n, ratio, kc):
    x, X = _matches(n, ratio, kc, seed=1000 + n)
    thr, ns = 2.0, 24
    host = R.sample_poses_host(x, X, FC, CC, ns, 3000, thr, kc, seed=5, detail=True)
    _check_margins(host, thr)
    dev = R.sample_poses(x, X, FC, CC, ns, 3000, thr, kc, seed=5)
    _same(dev, host)
    if ratio == 1.0 and n >= 64:
        assert host["accepted"] == ns


def test_device_equals_host_when_maxtrials_binds():
    x, X = _matches(1000, 0.3, 0.0, seed=77)
    host = R.sample_poses_host(x, X, FC, CC, 200, 2500, 2.0, 0.0, seed=9, detail=True)
    assert 0 < host["accepted"] < 200 and host["trials_used"] == 2500
    _check_margins(host, 2.0)
    _same(R.sample_poses(x, X, FC, CC, 200, 2500, 2.0, 0.0, seed=9), host)


def test_bit_identical_across_runs_and_chunk_sizes(monkeypatch):
    x, X = _matches(2000, 0.35, -0.05, seed=3)
    runs = []
    for chunk in (None, None, "1024", "3000"):
        if chunk is None:
            monkeypatch.delenv("ICTR_RANSAC_CHUNK", raising=False)
        else:
            monkeypatch.setenv("ICTR_RANSAC_CHUNK", chunk)
        s = R.RansacSampler(2000, 300)
        if chunk is not None:
            assert s.chunk == int(chunk)
        s.set_points(x, X)
        s.run_async(FC, CC, 300, 40000, 2.0, -0.05, seed=11)
        runs.append(s.wait())
    assert runs[0]["accepted"] > 0
    for r in runs[1:]:
        for k in ("p", "R", "t", "inl_cnt", "trials", "draws", "words"):
            assert np.array_equal(r[k], runs[0][k]) and r[k].tobytes() == runs[0][k].tobytes(), k
        assert r["trials_used"] == runs[0]["trials_used"] and r["accepted"] == runs[0]["accepted"]


def test_refusals():
    x, X = _matches(100, 0.6, 0.0, seed=4)
    with pytest.raises(ic.IctrError):
        R.RansacSampler(3, 10)
    with pytest.raises(ic.IctrError):
        R.RansacSampler(1 << 25, 10)
    s = R.RansacSampler(100, 10)
    with pytest.raises(ic.IctrError):  # before set_points
        s.run_async(FC, CC, 10, 100, 2.0)
    s.set_points(x, X)
    for ns, mt, thr in ((0, 100, 2.0), (11, 100, 2.0), (10, 0, 2.0), (10, 100, float("nan")), (10, 100, float("inf"))):
        with pytest.raises(ic.IctrError):
            s.run_async(FC, CC, ns, mt, thr)
    s.run_async(FC, CC, 10, 100000, 2.0)
    with pytest.raises(ic.IctrError):  # setters and a second run are refused while the run is in flight
        s.set_points(x, X)
    with pytest.raises(ic.IctrError):
        s.run_async(FC, CC, 10, 100, 2.0)
    s.wait()
    with pytest.raises(ic.IctrError):  # nothing in flight any more
        s.wait()
    s.set_points(x, X)


def test_destroy_with_a_run_pending(monkeypatch):
    """A sampler dropped with its run in flight ends that run before its buffers go; a fresh one then gives the host's
    result. 67 matches (one full and one ragged 64-block) in chunks of 16 trials."""
    monkeypatch.setenv("ICTR_RANSAC_CHUNK", "16")
    x, X = _matches(67, 0.6, 0.0, seed=67)
    s = R.RansacSampler(67, 5)
    assert s.chunk == 16
    s.set_points(x, X)
    s.run_async(FC, CC, 5, 300, 2.0, seed=2)
    del s
    host = R.sample_poses_host(x, X, FC, CC, 5, 300, 2.0, 0.0, seed=2, detail=True)
    _check_margins(host, 2.0)
    assert host["accepted"] > 0
    _same(R.sample_poses(x, X, FC, CC, 5, 300, 2.0, 0.0, seed=2), host)


def _e2e_scene():
    w, h = 320, 240
    pref = np.array([0.02, -0.03, 0.05, 0.01, -0.02, 0.015])
    step = np.array([0.04, 0.015, 0.0, 0.004, -0.003, 0.0])
    poses = [pref + (k - 2) * step for k in range(5)]
    sq = synth.make_sequence(w, h, poses, 2, 200, seed=21, quantize=False)
    rng = np.random.default_rng(22)
    pt2d = np.concatenate([sq["px_ref"], np.stack([rng.uniform(0, w, 200), rng.uniform(0, h, 200)], 1)], 0)
    pt3d = np.concatenate([sq["pts3d"], sq["pts3d"][rng.permutation(200)] + rng.normal(0, 0.5, (200, 3))], 0)
    op = dict(lv_f=3, lv_l=0, psz=8, maxiter=10, normdp_ratio=0.01, donorm=1, dopatchnorm=0, maxpttrack=0, verbosity=0)
    cam = dict(fc=sq["fc"], cc=sq["cc"], wh=sq["wh"])
    return sq, poses, pt2d, pt3d, op, cam


def test_fit_cameras_odom_end_to_end(tmp_path):
    sq, poses, pt2d, pt3d, op, cam = _e2e_scene()
    thr = float(np.hypot(*sq["wh"])) / 100.0
    fin = str(tmp_path / "odometrycheck.txt")
    res = R.fit_cameras_odom(pt2d, pt3d, cam, 40, 4000, thr, op, (2, 2), sq["frames"], seed=3, write_input=fin)
    b, means = res["best"], res["res_corravg"]
    assert b is not None and len(res["samples"]["p"]) > 0
    assert means[b] == np.nanmax(means) and not np.any(means[:b] == means[b])  # the script's rule (:152-153)
    # Samples whose first three draws are true matches carry the true pose; samples fitted through two true matches
    # and an outlier carry a wrong pose with a handful of inliers, and tracking so few points can correlate better
    # than the true samples' 200 (the script's rule then picks one of them). So the poses are checked on the
    # samples that start at the ground truth: their tracked end-frame poses must be right.
    good = [s for s, p in enumerate(res["samples"]["p"]) if np.abs(p - poses[2]).max() <= 1e-2]
    assert len(good) >= 5
    for s in good:
        assert np.abs(res["res_pose"][s][0] - poses[0]).max() <= 2e-2
        assert np.abs(res["res_pose"][s][4] - poses[4]).max() <= 2e-2
        assert means[s] > 0.99
    G = synth.se3_exp(res["p_best"][2])
    assert np.array_equal(res["p_best"], res["res_pose"][b])
    assert np.allclose(res["R_best"][2], G[:, :3]) and np.allclose(res["c_best"][2], -G[:, :3].T @ G[:, 3])
    # the verification equals run_track_nposes on the file the reference would have written
    want = str(tmp_path / "want.txt")
    assert run_track_nposes.main([fin, want]) == 0
    got = str(tmp_path / "got.txt")
    iof.write_nposes_result(got, res["res_corr"], res["res_pose"])
    assert open(got).read() == open(want).read()
    # the CLI on the same input gives the same samples and the same result file
    fin2, fres = str(tmp_path / "in2.txt"), str(tmp_path / "res_cli.txt")
    argv = [fin, fin2, "--track", fres, "--nsamples", "40", "--maxtrials", "4000", "--inlthresh", repr(thr), "--seed", "3"]
    assert run_ransac.main(argv) == 0
    assert open(fin2).read() == open(fin).read()
    assert open(fres, "rb").read() == open(want, "rb").read()
    # the C++ facade writes the same sample file
    exe = tmp_path / "ransac_driver"
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "cxx", "ransac_driver.cpp"),
                           "-L" + os.path.join(ROOT, "invcompcamtrack_amd"), "-l:libictr_hip.so",
                           "-Wl,-rpath," + os.path.join(ROOT, "invcompcamtrack_amd")])
    fin3 = str(tmp_path / "in3.txt")
    r = subprocess.run([str(exe), fin, fin3, "40", "4000", repr(thr), "0", "3"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(fin3).read() == open(fin).read()
