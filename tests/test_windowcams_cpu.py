"""The window hand-over on the host: windowcams.window_cameras_host (the definition) against the chain of
tests/camfit_cases.py byte for byte, the conditions that keep the GPU test from being about an all-ones mask,
csrc/ictr_handover_hd.h as a sanitized stand-alone program against depth_from_disparity and points_from_first_view in the
bits, and the new entry points' errors on NULL arguments and without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import camfit_cases as K
import windowcams_cases as WC
from invcompcamtrack_amd import camfit as F
from invcompcamtrack_amd import fsplit as S
from invcompcamtrack_amd import windowcams as W
from test_stereotrack_cpu import fields, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEPT = dict(small_disp=(357, 462), large_disp=(143, 242), odd_long=(240, 777), two_frames=(439, 532))


@pytest.mark.parametrize("name", WC.WINDOWS)
def test_host_definition_equals_the_chain_of_the_camera_fit_tests(name):
    c = golden()[name]
    got = WC.host(name)
    split, X, left, right, fit = K.chain_host(c["xy_t"])
    err_l, _ = F.reprojection_errors_host(X, left, K.CAM, fit["G"], mask=split["words"])
    err_r, _ = F.reprojection_errors_host(X, right, K.CAM, fit["G"], mask=split["words"], offset=[K.BASELINE, 0.0, 0.0])
    want = dict(split)
    want.update(fit)
    want.update(m=len(c["rows"]), err_left=err_l, err_right=err_r)
    WC.same(got, want, name)
    assert got["xy_t"].tobytes() == c["xy_t"].tobytes() and np.array_equal(got["rows"], c["rows"])
    # a survivor never holds a NaN: the pairs keep every row, so the device needs no second compaction
    pairs, rows = S.pairs_from_stereo_tracks(c["xy_t"])
    assert np.array_equal(rows, np.arange(len(c["rows"]))) and pairs.shape == (2 * (c["xy_t"].shape[2] // 2), 4, len(rows))
    assert got["best_count"] == got["m"] and got["mask"].all()  # the default threshold keeps every survivor


@pytest.mark.parametrize("name", WC.WINDOWS)
def test_the_tight_threshold_splits_the_golden_windows(name):
    """thresh = 0.03: a real share of the points is kept, trial 0 does not win, every fit converges and the last frame's
    means are small. The GPU test on these inputs is not about an all-ones mask."""
    r = WC.host(name, WC.TIGHT)
    m = r["m"]
    print(name, "keeps", r["best_count"], "of", m, "trial", r["best_trial"], "err", r["err_left"][-1], r["err_right"][-1])
    assert (r["best_count"], m) == KEPT[name]
    assert 0.2 * m < r["best_count"] < 0.9 * m and r["best_trial"] > 0
    assert (r["status"] == F.CONVERGED).all()
    assert r["err_left"][-1] < 0.13 and r["err_right"][-1] < 0.13
    assert int(r["mask"].sum()) == r["best_count"] == len(r["inliers"]) and not r["mask"].all()


def test_too_small_windows_are_refused_on_the_host():
    with pytest.raises(ValueError, match="bsize"):
        W.window_cameras_host(*fields(golden()["one_frame"]), K.CAM, K.BASELINE)
    c = golden()["two_frames"]
    xy0 = np.stack([np.arange(7) + 5.0, np.full(7, 6.0)], 1)
    with pytest.raises(ValueError, match="points"):
        W.window_cameras_host(*fields(c), K.CAM, K.BASELINE, xy0=xy0)


# ---------------------------------------------------------------- the shared header on the host
@pytest.fixture(scope="module")
def hd_host():
    exe = os.path.join(ROOT, "tests", "cxx", "handover_hd_host")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        "-I" + os.path.join(ROOT, "invcompcamtrack_amd", "csrc"), "-o", exe, exe + ".cpp"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run_header(exe, tmp_path, xy_t, cam, baseline):
    m, _, b = xy_t.shape
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([m, b], np.int64).tobytes())
        f.write(np.array([cam[0][0], cam[0][1], cam[1][0], cam[1][1], baseline], np.float64).tobytes())
        f.write(np.ascontiguousarray(xy_t, np.float64).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    raw = np.fromfile(fout, np.uint8)
    return tuple(int(v) for v in raw[:16].view(np.int64)), raw[16:].view(np.float64).reshape(3, m)


def test_shared_header_on_the_host_equals_the_numpy_lines(hd_host, tmp_path):
    """csrc/ictr_handover_hd.h as plain C++ (-ffp-contract=off, address and undefined-behaviour sanitizers) gives the bits
    of depth_from_disparity and points_from_first_view, a zero disparity and a NaN coordinate included."""
    cams = (K.CAM, ((718.856, 721.3), (607.1928, 185.2157)))
    for name in WC.WINDOWS:
        xy_t = np.array(golden()[name]["xy_t"])
        xy_t[3, 2, 0] = xy_t[3, 0, 0]       # zero disparity: +-inf and NaN
        xy_t[5, 2, 0] = xy_t[5, 0, 0]
        xy_t[5, 0, 0] = xy_t[5, 2, 0] = K.CC[0]  # ... and 0 * inf
        xy_t[7, 1, 0] = np.nan              # a NaN coordinate
        xy_t[9, 0, 0] = np.nan
        for cam, baseline in zip(cams, (K.BASELINE, 0.537)):
            half, X = _run_header(hd_host, tmp_path, xy_t, cam, baseline)
            want = F.points_from_first_view(xy_t, cam, F.depth_from_disparity(xy_t, cam[0][0], baseline))
            assert X.tobytes() == np.ascontiguousarray(want).tobytes(), name
            assert np.isinf(want[2, 3]) and not np.isfinite(want[:, 5]).any() and np.isnan(want[0, 5]) == (cam is K.CAM)
            assert np.isnan(want[1, 7]) and np.isnan(want[:, 9]).all()
            assert half == S._half(xy_t.shape[2])
    for b in range(1, 9):
        half, _ = _run_header(hd_host, tmp_path, np.zeros((0, 4, b)), K.CAM, 1.0)
        assert half == S._half(b)


# ---------------------------------------------------------------- the entry points without their arguments or a device
def test_new_entry_points_fail_loudly_on_null_and_without_a_device():
    import __graft_entry__ as g
    g.build()
    import invcompcamtrack_amd as ic
    from invcompcamtrack_amd import _lib
    L = _lib.load()
    calls = [(L.ictr_fsplit_set_pairs_from_window, (None, None)),
             (L.ictr_camfit_set_points_from_window, (None, None, 1.0)),
             (L.ictr_camfit_set_observations_from_window, (None, None, 0)),
             (L.ictr_camfit_set_mask_from_fsplit, (None, None, None)),
             (L.ictr_debug_fsplit_pairs, (None, None)),
             (L.ictr_debug_camfit_inputs, (None, None, None, None))]
    for fn, args in calls:
        assert fn(*args) != 0, fn.__name__
        assert b"NULL" in L.ictr_last_error(), fn.__name__
        with pytest.raises(_lib.IctrError, match="NULL"):
            _lib.check(fn(*args))
    if ic.device_count() == 0:  # the pipeline has no host fall-back: its first device object says so
        with pytest.raises(_lib.IctrError, match="no usable HIP device"):
            W.window_cameras(*fields(golden()["two_frames"]), K.CAM, K.BASELINE)
        with pytest.raises(_lib.IctrError, match="no usable HIP device"):
            W.cameras_from_tracks(golden()["two_frames"]["xy_t"], K.CAM, K.BASELINE)
    assert C.sizeof(C.c_void_p) == 8
