"""The stereo track window on the host: the restatement of stereotrack.py against the reference's own lines (the golden
file of tests/golden/make_stereotrack_golden.py), the cases' reach through `reasons`, the edges against the plain-loop
restatement of tests/stereotrack_np.py, and csrc/ictr_stereotrack_hd.h as a sanitized stand-alone program, bit for bit."""
import functools
import os
import subprocess

import numpy as np
import pytest

import stereotrack_np as NP
from invcompcamtrack_amd import stereotrack as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stereotrack_golden.npz")


@functools.lru_cache(maxsize=None)
def golden():
    out = {}
    with np.load(GOLDEN) as z:
        for name in z["cases"]:
            name = str(name)
            c = {k: z[name + "_" + k] for k in ("disp_lr", "disp_rl", "flow_l", "flow_r", "xy_t", "rows")}
            for a in c.values():
                a.setflags(write=False)
            out[name] = c
    return out


def fields(c):
    return c["disp_lr"], c["disp_rl"], c["flow_l"], c["flow_r"]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_the_golden_file_has_the_cases_of_the_issue():
    g = golden()
    shapes = sorted(c["disp_lr"].shape for c in g.values())
    assert shapes == sorted([(4, 24, 40), (4, 24, 40), (6, 33, 47), (1, 8, 8), (2, 24, 40)])
    assert os.path.getsize(GOLDEN) < (1 << 20)
    for c in g.values():
        assert not np.isnan(c["xy_t"]).any()


@pytest.mark.parametrize("name", ["small_disp", "large_disp", "odd_long", "one_frame", "two_frames"])
def test_restatement_equals_the_reference_lines(name):
    c = golden()[name]
    xy_t, rows = S.stereo_track_window_host(*fields(c))
    assert xy_t.dtype == np.float64 and rows.dtype == np.int64
    assert np.array_equal(rows, c["rows"])
    assert xy_t.shape == c["xy_t"].shape and np.array_equal(xy_t, c["xy_t"])
    again, rows2, why = S.stereo_track_window_host(*fields(c), reasons=True)
    assert np.array_equal(_bits(again), _bits(xy_t)) and np.array_equal(rows2, rows)
    kept = why["frame"] < 0
    assert np.array_equal(np.nonzero(kept)[0], rows)
    assert (why["mask"][kept] == 0).all() and (why["mask"][~kept] != 0).all()


def test_the_golden_cases_are_not_vacuous():
    """Each case keeps between 10 % and 90 % of its points, and over the case set every one of bits 0-8 is the only
    failed test of at least one point."""
    alone = set()
    for name, c in golden().items():
        _, rows, why = S.stereo_track_window_host(*fields(c), reasons=True)
        n = c["disp_lr"].shape[1] * c["disp_lr"].shape[2]
        print(name, "keeps", len(rows), "of", n)
        assert 0.1 * n <= len(rows) <= 0.9 * n, name
        m = why["mask"].astype(np.int64)
        single = m[(m > 0) & (m & (m - 1) == 0)]
        alone |= {int(v).bit_length() - 1 for v in single}
        if c["disp_lr"].shape[0] > 1:
            assert (why["frame"] > 0).any(), name  # a later frame drops points too
    assert alone == set(range(9)), alone


# ---------------------------------------------------------------- edges against the plain loops
def _constant(h, w, bsize, disp=3.0, move=(1.0, 0.5)):
    lr = np.full((bsize, h, w), disp, np.float32)
    rl = np.full((bsize, h, w), disp, np.float32)
    f = np.zeros((bsize, 2, h, w, 2), np.float32)
    f[:, 0] = move
    f[:, 1] = (-move[0], -move[1])
    return lr, rl, f, f.copy()


def _both(args, xy0=None, **kw):
    got = S.stereo_track_window_host(*args, xy0=xy0, **kw)
    want = NP.window(*args, xy0=xy0, **kw)
    assert got[0].shape == want[0].shape
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1])
    return got


def test_edges_one_frame_and_a_golden_case_by_plain_loops():
    c = golden()["one_frame"]
    xy_t, rows = _both(fields(c))
    assert xy_t.shape == (len(c["rows"]), 4, 1)
    c = golden()["two_frames"]
    _both(fields(c))
    _both(fields(c), th_ratio=0.05, th_abs=0.3)


def test_edges_all_dropped_and_all_kept():
    h, w, b = 9, 12, 3
    zero = _constant(h, w, b, disp=0.0)  # zero disparity: 0 / 0 compares false
    xy_t, rows = _both(zero)
    assert xy_t.shape == (0, 4, b) and rows.shape == (0,)
    still = _constant(h, w, b, move=(0.0, 0.0))  # zero motion: dropped at frame 1, kept by a window of one frame
    assert _both(still)[0].shape == (0, 4, b)
    assert _both(tuple(a[:1] for a in still))[0].shape[0] > 0
    xy0 = np.array([[x + 0.25, y + 0.5] for y in range(1, 4) for x in range(4, 8)])
    xy_t, rows = _both(_constant(h, w, b), xy0=xy0)
    assert np.array_equal(rows, np.arange(len(xy0))) and xy_t.shape == (len(xy0), 4, b)
    assert np.array_equal(xy_t[:, 0, 2], xy0[:, 0] + 2.0) and np.array_equal(xy_t[:, 2, 0], xy0[:, 0] - 3.0)


def test_edges_nan_and_border_starts_and_a_custom_start_set():
    c = golden()["small_disp"]
    h, w = c["disp_lr"].shape[1:]
    rng = np.random.default_rng(5)
    xy0 = np.concatenate([
        [[np.nan, 3.0], [4.0, np.nan], [np.nan, np.nan], [np.inf, 2.0], [-0.5, 2.0], [3.0, -1e-9]],
        [[w - 1.0, 5.0], [w - 2 + 0.999, 5.0], [w - 2.0, 5.0], [20.0, h - 1.0], [20.0, h - 2 + 0.999], [20.0, h - 2.0]],
        rng.uniform([0, 0], [w - 1, h - 1], (150, 2))])
    xy_t, rows = _both(fields(c), xy0=xy0)
    assert 10 < len(rows) < len(xy0)
    assert not np.isin(rows, [0, 1, 2, 3, 4, 5, 6, 9]).any()  # NaN, outside, x = W-1 and y = H-1 fail the range test
    got = S.stereo_track_window_host(*fields(c), xy0=xy0, reasons=True)[2]
    assert (got["frame"][[0, 1, 2, 3, 4, 5, 6, 9]] == 0).all() and (got["mask"][[0, 1, 2, 3, 4, 5, 6, 9]] == 1).all()
    # the default start set is the script's meshgrid
    every = np.array([[x, y] for y in range(h) for x in range(w)], np.float64)
    a, b = S.stereo_track_window_host(*fields(c)), S.stereo_track_window_host(*fields(c), xy0=every)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1])


def test_bad_arguments_are_refused():
    lr, rl, fl, fr = _constant(6, 7, 3)
    with pytest.raises(ValueError):
        S.stereo_track_window_host(lr, rl[:2], fl, fr)
    with pytest.raises(ValueError):
        S.stereo_track_window_host(lr, rl, fl[:1], fr)
    with pytest.raises(ValueError):
        S._exact_f32(np.array([[0.1]]))  # a float64 value that float32 cannot hold is refused, not rounded
    assert S._exact_f32(np.array([[0.5, np.nan]])).dtype == np.float32


# ---------------------------------------------------------------- the shared header on the host
@pytest.fixture(scope="module")
def hd_host():
    exe = os.path.join(ROOT, "tests", "cxx", "stereotrack_hd_host")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        "-I" + os.path.join(ROOT, "invcompcamtrack_amd", "csrc"), "-o", exe, exe + ".cpp"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run_header(exe, tmp_path, args, xy0, th=(0.2, 1.0)):
    lr, rl, fl, fr = (np.ascontiguousarray(a, np.float32) for a in args)
    b, h, w = lr.shape
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([h, w, b, 0 if xy0 is None else len(xy0)], np.int64).tobytes())
        f.write(np.array(th, np.float64).tobytes())
        f.write(lr.tobytes() + rl.tobytes() + fl.tobytes() + fr.tobytes())
        if xy0 is not None:
            f.write(np.ascontiguousarray(xy0, np.float64).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    raw = np.fromfile(fout, np.uint8)
    m = int(raw[:8].view(np.int64)[0])
    rows = raw[8:8 + 8 * m].view(np.int64)
    xy_t = raw[8 + 8 * m:].view(np.float64).reshape(m, 4, b)
    return xy_t, rows


def test_shared_header_on_the_host_equals_the_reference_lines(hd_host, tmp_path):
    """csrc/ictr_stereotrack_hd.h compiled as plain C++ (tests/cxx/stereotrack_hd_host.cpp, -ffp-contract=off, address and
    undefined-behaviour sanitizers) reproduces every golden xy_t in the bits, NaN and border starts included, and the
    sanitizers stay silent."""
    for name, c in golden().items():
        xy_t, rows = _run_header(hd_host, tmp_path, fields(c), None)
        assert np.array_equal(rows, c["rows"]), name
        assert np.array_equal(_bits(xy_t), _bits(c["xy_t"])), name
    c = golden()["odd_long"]
    h, w = c["disp_lr"].shape[1:]
    xy0 = np.concatenate([[[np.nan, 1.0], [w - 1.0, 2.0], [w - 2 + 0.999, 2.0], [-3.0, 1e300], [1e300, 2.0]],
                          np.random.default_rng(9).uniform([-2, -2], [w + 1, h + 1], (300, 2))])
    xy_t, rows = _run_header(hd_host, tmp_path, fields(c), xy0, th=(0.15, 0.7))
    want = S.stereo_track_window_host(*fields(c), xy0=xy0, th_ratio=0.15, th_abs=0.7)
    assert len(rows) > 20 and np.array_equal(rows, want[1]) and np.array_equal(_bits(xy_t), _bits(want[0]))
