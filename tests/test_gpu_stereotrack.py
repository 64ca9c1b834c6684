"""The stereo track window on the device against stereotrack.stereo_track_window_host (itself pinned to the reference's
lines in test_stereotrack_cpu.py), with np.array_equal on every output: the golden cases from host and from device
pointers, scan-block edges, a compaction that crosses many workgroups, the edges of the window, the sign and the
flow-grid kind of a field descriptor, frames in (StereoPointTracker), the chain down to the camera fit, the native caller
and the CLI."""
import functools
import os
import subprocess

import numpy as np
import pytest

import camfit_cases as K
from invcompcamtrack_amd import patchflow as pf
from invcompcamtrack_amd import stereotrack as S
from invcompcamtrack_amd import synth
from test_stereotrack_cpu import _constant, fields, golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["small_disp", "large_disp", "odd_long", "one_frame", "two_frames"]


@functools.lru_cache(maxsize=None)
def host(name):
    out = S.stereo_track_window_host(*fields(golden()[name]))
    for a in out:
        a.setflags(write=False)
    return out


def _same(got, want, what=""):
    assert got[0].dtype == np.float64 and got[1].dtype == np.int64, what
    assert got[0].shape == want[0].shape and np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[0], want[0]) and got[0].tobytes() == want[0].tobytes(), what


@pytest.mark.parametrize("name", CASES)
def test_golden_cases_from_host_pointers(name):
    c = golden()[name]
    _same(S.stereo_track_window(*fields(c)), host(name), name)
    _same(S.stereo_track_window(*fields(c)), (c["xy_t"], c["rows"]), name)


def test_golden_cases_from_device_pointers():
    import torch
    for name in CASES:
        dev = [torch.from_numpy(np.array(a)).cuda() for a in fields(golden()[name])]
        torch.cuda.synchronize()
        _same(S.stereo_track_window(*dev), host(name), name)


@functools.lru_cache(maxsize=None)
def _big():
    """97 x 131, every pixel, 3 frames: smooth consistent fields with sparse defects, about half the points kept."""
    h, w, b = 97, 131, 3
    rng = np.random.default_rng(31)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    d = 3.0 + 0.3 * np.sin(xx / 40.0) * np.cos(yy / 30.0)
    lr = np.stack([d] * b)
    rl = np.stack([3.0 + 0.3 * np.sin((xx + d) / 40.0) * np.cos(yy / 30.0)] * b)
    f = np.zeros((b, 2, h, w, 2))
    f[:, 0] = (1.25, -0.75)
    f[:, 1] = (-1.25, 0.75)
    fl, fr = f.copy(), f.copy()
    for a in (lr, rl, fl[..., 0], fr[..., 1]):
        a += np.where(rng.uniform(size=a.shape) < 0.03, rng.choice([0.7, -2.0], size=a.shape), 0.0)
    args = tuple(a.astype(np.float32) for a in (lr, rl, fl, fr))
    want = S.stereo_track_window_host(*args)
    assert 0.2 * h * w < len(want[1]) < 0.8 * h * w
    return args, want


def test_every_pixel_across_many_workgroups_and_two_runs():
    args, want = _big()
    win = S.StereoTrackWindow(131, 97, 3)
    a = S.stereo_track_window(*args, window=win)
    _same(a, want)
    assert len(np.unique((want[1] // 256))) > 40  # survivors in many workgroups, so the order crosses the scan
    b = S.stereo_track_window(*args, window=win)
    c = S.stereo_track_window(*args)
    assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes() and a[1].tobytes() == b[1].tobytes() == c[1].tobytes()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_scan_block_edges(n):
    args, _ = _big()
    xy0 = np.random.default_rng(n).uniform([0, 0], [130, 96], (n, 2))
    xy0[-1] = (20.5, 30.25) if n > 1 else xy0[-1]
    want = S.stereo_track_window_host(*args, xy0=xy0)
    _same(S.stereo_track_window(*args, xy0=xy0), want, n)
    keep = want[1]
    if n > 1:
        assert 0 < len(keep) < n
        only = xy0[keep]  # all kept, then with one NaN start in front
        _same(S.stereo_track_window(*args, xy0=only), (want[0], np.arange(len(keep))), n)
        _same(S.stereo_track_window(*args, xy0=np.concatenate([[[np.nan, 1.0]], only])),
              (want[0], np.arange(1, len(keep) + 1)), n)


def test_window_edges_one_frame_none_kept_all_kept_thresholds():
    h, w, b = 9, 12, 3
    zero = _constant(h, w, b, disp=0.0)
    got = S.stereo_track_window(*zero)
    assert got[0].shape == (0, 4, b) and got[1].shape == (0,)
    _same(got, S.stereo_track_window_host(*zero))
    one = tuple(a[:1] for a in _constant(h, w, b))
    _same(S.stereo_track_window(*one), S.stereo_track_window_host(*one))
    assert S.stereo_track_window(*one)[0].shape[2] == 1
    xy0 = np.array([[x + 0.25, y + 0.5] for y in range(1, 4) for x in range(4, 8)])
    got = S.stereo_track_window(*_constant(h, w, b), xy0=xy0)
    _same(got, S.stereo_track_window_host(*_constant(h, w, b), xy0=xy0))
    assert np.array_equal(got[1], np.arange(len(xy0)))
    c = golden()["odd_long"]
    hh, ww = c["disp_lr"].shape[1:]
    xy0 = np.concatenate([[[np.nan, 3.0], [ww - 1.0, 5.0], [ww - 2 + 0.999, 5.0], [1e300, 2.0], [-0.5, 2.0]],
                          np.random.default_rng(3).uniform([-2, -2], [ww + 1, hh + 1], (400, 2))])
    for th in ((0.2, 1.0), (0.05, 0.3), (np.inf, np.inf)):
        _same(S.stereo_track_window(*fields(c), xy0=xy0, th_ratio=th[0], th_abs=th[1]),
              S.stereo_track_window_host(*fields(c), xy0=xy0, th_ratio=th[0], th_abs=th[1]), th)


def test_call_order_and_bad_fields_are_refused():
    from invcompcamtrack_amd import IctrError
    lr, rl, fl, fr = _constant(9, 12, 2)
    win = S.StereoTrackWindow(12, 9, 2)
    with pytest.raises(IctrError, match="open comes first"):
        win.advance(fl[0, 0], fl[0, 1], fr[0, 0], fr[0, 1], lr[1], rl[1])
    win.open(S.field(lr[0], -1), rl[0])
    with pytest.raises(IctrError, match="advances come first"):
        win.count()
    with pytest.raises(IctrError, match="two components"):
        win.advance(lr[0], fl[0, 1], fr[0, 0], fr[0, 1], lr[1], rl[1])
    win.advance(fl[0, 0], fl[0, 1], fr[0, 0], fr[0, 1], S.field(lr[1], -1), rl[1])
    with pytest.raises(IctrError, match="is full"):
        win.advance(fl[0, 0], fl[0, 1], fr[0, 0], fr[0, 1], lr[1], rl[1])
    assert win.count() == len(win.read()[1])
    with pytest.raises(ValueError):
        S.stereo_track_window(lr.astype(np.float64) + 0.1, rl, fl, fr)  # float64 values are never rounded
    _same(S.stereo_track_window(lr.astype(np.float64), rl, fl, fr), S.stereo_track_window_host(lr, rl, fl, fr))
    with pytest.raises(IctrError):
        S.StereoTrackWindow(12, 9, 0)
    with pytest.raises(ValueError):
        S.StereoTrackWindow(12, 9, 2).open(lr[0][:, :5], rl[0])


def test_the_sign_of_a_descriptor():
    """The same field negated with sign -1 is the same window: in every slot of every step."""
    c = golden()["small_disp"]
    lr, rl, fl, fr = fields(c)
    b = lr.shape[0]
    win = S.StereoTrackWindow(lr.shape[2], lr.shape[1], b)
    neg = lambda a: S.field(-np.ascontiguousarray(a), -1)  # noqa: E731
    win.open(lr[0].copy() * -1.0, neg(rl[0]))  # sign +1 on the negated disparity = the script's -imgs_d
    for k in range(1, b):
        win.advance(neg(fl[k - 1, 0]), fl[k - 1, 1], fr[k - 1, 0], neg(fr[k - 1, 1]), S.field(lr[k], -1), neg(rl[k]))
    _same(win.read(), host("small_disp"))


def _grid_with(w, h, step, rng, amp, base):
    g = pf.FlowGrid(w, h, step)
    d = (np.asarray(base, np.float32) + rng.normal(0, amp, (g.ny, g.nx, 2))).astype(np.float32)
    lost = rng.uniform(size=(g.ny, g.nx)) < 0.05
    return g.set_nodes(d, lost)


def test_the_flow_grid_kind_equals_the_plane_kind_on_its_dense_field():
    w, h, step, b = 75, 50, 4, 3
    rng = np.random.default_rng(12)
    names = ("lr", "rl", "l_fwd", "l_bwd", "r_fwd", "r_bwd")
    base = dict(lr=(-4.0, 0.3), rl=(4.0, -0.2), l_fwd=(1.5, 0.5), l_bwd=(-1.5, -0.5), r_fwd=(1.5, 0.5), r_bwd=(-1.5, -0.5))
    sets = [{n: _grid_with(w, h, step, rng, 0.04, base[n]) for n in names} for _ in range(b)]
    win = S.StereoTrackWindow(w, h, b)
    win.open(sets[0]["lr"], sets[0]["rl"])
    for k in range(1, b):
        win.advance(*[sets[k][n] for n in names[2:]], sets[k]["lr"], sets[k]["rl"])
    got = win.read()
    dense = [{n: g.dense() for n, g in s.items()} for s in sets]
    planes = ([-d["lr"][:, :, 0] for d in dense], [np.ascontiguousarray(d["rl"][:, :, 0]) for d in dense],
              [(d["l_fwd"], d["l_bwd"]) for d in dense[1:]], [(d["r_fwd"], d["r_bwd"]) for d in dense[1:]])
    want = S.stereo_track_window_host(*planes)
    assert 0.1 * w * h < len(want[1]) < 0.95 * w * h
    _same(got, want)
    _same(S.stereo_track_window(*planes), want)
    # a flow in a stereo slot moves x only, like the grid there
    win.open(dense[0]["lr"], dense[0]["rl"])
    for k in range(1, b):
        win.advance(*[dense[k][n] for n in names[2:]], dense[k]["lr"], dense[k]["rl"])
    _same(win.read(), want)


@functools.lru_cache(maxsize=None)
def _stereo_frames(w=96, h=64, n=4):
    """A rendered plane seen by a left camera that moves a little per frame and a right camera beside it."""
    step = np.array([0.15, -0.06, 0.0, 0.0, 0.0, 0.004])  # about 1.3 px per frame at fc = 75 and depth 10
    base = np.array([0.3, -0.2, 0.5, 0.02, -0.03, 0.01])
    right = np.array([-0.55, 0.0, 0.0, 0.0, 0.0, 0.0])  # about 4 px of disparity
    poses = [base + k * step for k in range(n)] + [base + k * step + right for k in range(n)]
    fr = synth.make_sequence(w, h, poses, 0, 10, seed=4)["frames"]
    return fr[:n], fr[n:]


def test_frames_in_stereo_point_tracker_and_cli(tmp_path, capsys):
    from invcompcamtrack_amd import run_stereo_track as R
    left, right = _stereo_frames()
    kw = dict(step=4, psz=8, lv_f=2)
    t = S.StereoPointTracker(96, 64, 4, keep_grids=True, **kw)
    for a, b in zip(left, right):
        t.push_frames(a, b)
    got = t.window()
    want = S.stereo_track_window_host(*R.dense_fields_of(t))
    print("StereoPointTracker keeps", len(want[1]), "of", 96 * 64)
    _same(got, want)
    assert len(want[1]) > 100
    lean = S.StereoPointTracker(96, 64, 4, **kw)  # two grid sets reused in turn
    for a, b in zip(left, right):
        lean.push_frames(a, b)
    _same(lean.window(), want)
    with pytest.raises(ValueError):
        lean.push_frames(left[0], right[0])
    # the CLI from a list file, device and --host, and from dense fields
    names = []
    for k, (a, b) in enumerate(zip(left, right)):
        names.append((str(tmp_path / f"l{k}.npy"), str(tmp_path / f"r{k}.npy")))
        np.save(names[-1][0], a)
        np.save(names[-1][1], b)
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        f.write("".join(f"{a} {b}\n" for a, b in names))
    outs = []
    for extra in ([], ["--host"]):
        out = str(tmp_path / ("o%d.npz" % len(outs)))
        assert R.main([lst, out, "--bsize", "4", "--psz", "8", "--lv_f", "2"] + extra) == 0
        outs.append(open(out, "rb").read())
        with np.load(out) as z:
            _same((z["xy_t"], z["rows"]), want)
    assert outs[0] == outs[1]
    c = golden()["odd_long"]
    zin = str(tmp_path / "fields.npz")
    np.savez(zin, **{k: c[k] for k in ("disp_lr", "disp_rl", "flow_l", "flow_r")})
    outs = []
    for extra in ([], ["--host"]):
        out = str(tmp_path / ("f%d.npz" % len(outs)))
        assert R.main(["-", out, "--fields", zin] + extra) == 0
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1]
    with np.load(out) as z:
        _same((z["xy_t"], z["rows"]), host("odd_long"))
    assert "kept" in capsys.readouterr().out


def test_chain_window_to_camera_fit_on_the_device():
    """window -> pairs_from_stereo_tracks -> split_static -> depth_from_disparity -> fit_cameras on the device-made xy_t
    equals the same chain of host stages on the host-made one."""
    from invcompcamtrack_amd import camfit as F
    from invcompcamtrack_amd import fsplit
    c = golden()["odd_long"]
    xy_t, _ = S.stereo_track_window(*fields(c))
    hsplit, hX, hleft, _, hfit = K.chain_host(host("odd_long")[0])
    pairs, rows = fsplit.pairs_from_stereo_tracks(xy_t)
    split = fsplit.split_static(pairs)
    assert np.array_equal(split["words"], hsplit["words"])
    xy = xy_t[rows]
    X = F.points_from_first_view(xy, K.CAM, F.depth_from_disparity(xy, K.FC[0], K.BASELINE))
    left, _ = F.observations_from_stereo_tracks(xy)
    assert X.tobytes() == hX.tobytes() and left.tobytes() == hleft.tobytes()
    fit = F.fit_cameras(X, left, K.CAM, mask=split["words"])
    for k in ("G", "cost", "damp", "iters", "status", "n"):
        assert np.asarray(fit[k]).tobytes() == np.asarray(hfit[k]).tobytes(), k


def test_native_caller(tmp_path):
    """tests/cxx/stereotrack_driver.cpp (CTR::StereoTrackClass of include/ctr_shim.hpp) writes the host function's bytes."""
    exe = os.path.join(ROOT, "tests", "cxx", "stereotrack_driver")
    src = exe + ".cpp"
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        r = subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                            src, "-L" + os.path.join(ROOT, "invcompcamtrack_amd"), "-l:libictr_hip.so",
                            "-Wl,-rpath,$ORIGIN/../../invcompcamtrack_amd"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    c = golden()["odd_long"]
    lr, rl, fl, fr = (np.ascontiguousarray(a, np.float32) for a in fields(c))
    b, h, w = lr.shape
    for xy0 in (None, np.random.default_rng(2).uniform([0, 0], [w - 1, h - 1], (300, 2))):
        fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([h, w, b, 0 if xy0 is None else len(xy0)], np.int64).tobytes())
            f.write(np.array([0.2, 1.0]).tobytes() + lr.tobytes() + rl.tobytes() + fl.tobytes() + fr.tobytes())
            if xy0 is not None:
                f.write(xy0.tobytes())
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        want = S.stereo_track_window_host(lr, rl, fl, fr, xy0=xy0)
        raw = open(fout, "rb").read()
        assert raw == np.int64(len(want[1])).tobytes() + want[1].tobytes() + want[0].tobytes()
