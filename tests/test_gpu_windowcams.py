"""The window hand-over on the device against its host definition (windowcams.window_cameras_host, pinned to the existing
host stages in test_windowcams_cpu.py), with tobytes() / np.array_equal on every output and no tolerance anywhere: each
device buffer on its own, M at the edges of the workgroup with rows that are not arange, the whole chain from host and
from device fields, frames in (StereoPointTracker), the refusals, the native caller and the CLI."""
import functools
import os
import subprocess

import numpy as np
import pytest

import camfit_cases as K
import windowcams_cases as WC
from invcompcamtrack_amd import IctrError
from invcompcamtrack_amd import bundle as B
from invcompcamtrack_amd import camfit as F
from invcompcamtrack_amd import camransac as R
from invcompcamtrack_amd import fsplit
from invcompcamtrack_amd import stereotrack as S
from invcompcamtrack_amd import windowcams as W
from test_gpu_stereotrack import _big, _stereo_frames
from test_stereotrack_cpu import fields, golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _counted(args, xy0=None):
    """A StereoTrackWindow with every frame in, counted."""
    lr, rl, fl, fr = args
    b, h, w = lr.shape
    win = S.StereoTrackWindow(w, h, b)
    win.open(S.field(lr[0], -1), rl[0], xy0)
    for k in range(1, b):
        win.advance(fl[k - 1][0], fl[k - 1][1], fr[k - 1][0], fr[k - 1][1], S.field(lr[k], -1), rl[k])
    win.count()
    return win


def _buffers_equal_the_host(win, xy_t, what):
    """pairs, points and both sides' observations written from the window, each read back on its own; -> (split, fit)."""
    m, _, b = xy_t.shape
    assert win.survivors == m, what
    split, fit = fsplit.StaticSplitter(m, 2 * (b // 2)), F.CameraFitter(m, b)
    split.set_pairs_from_window(win)
    pairs, rows = fsplit.pairs_from_stereo_tracks(xy_t)
    assert np.array_equal(rows, np.arange(m)), what
    assert split.debug_pairs().tobytes() == pairs.tobytes(), what
    fit.set_camera(K.CAM)
    fit.set_points_from_window(win, K.BASELINE)
    X = F.points_from_first_view(xy_t, K.CAM, F.depth_from_disparity(xy_t, K.FC[0], K.BASELINE))
    assert fit.debug_inputs()["X"].tobytes() == np.ascontiguousarray(X).tobytes(), what
    left, right = F.observations_from_stereo_tracks(xy_t)
    fit.set_observations_from_window(win, right=False)
    assert fit.debug_inputs()["xy"].tobytes() == left.tobytes(), what
    fit.set_observations_from_window(win, right=True)
    assert fit.debug_inputs()["xy"].tobytes() == right.tobytes(), what
    return split, fit


@pytest.mark.parametrize("name", ["odd_long", "two_frames", "big_odd"])
def test_each_buffer_on_its_own(name):
    if name == "big_odd":  # bsize 3, M = 7085: the middle frame is in no pair, the survivors sit in many workgroups
        args, (xy_t, want_rows) = _big()
        words = None
        assert xy_t.shape[2] == 3 and xy_t.shape[0] > 7000
    else:
        args, xy_t, want_rows = fields(golden()[name]), golden()[name]["xy_t"], golden()[name]["rows"]
        words = WC.host(name, WC.TIGHT)["words"]
    win = _counted(args)
    split, fit = _buffers_equal_the_host(win, xy_t, name)
    # the split's words reach the fit while the run is in flight, and again after its wait
    split.run_async(100, WC.TIGHT, 0)
    fit.set_mask_from_fsplit(split)
    in_flight = fit.debug_inputs()["words"]
    s = split.wait()
    assert in_flight.tobytes() == s["words"].tobytes()
    fit.set_mask(np.zeros(len(xy_t), bool))
    assert not fit.debug_inputs()["words"].any()
    fit.set_mask_from_fsplit(split)
    assert fit.debug_inputs()["words"].tobytes() == s["words"].tobytes()
    if words is not None:
        assert s["words"].tobytes() == words.tobytes()
    # the window stays counted and readable
    got, rows = win.read()
    assert got.tobytes() == np.ascontiguousarray(xy_t).tobytes() and np.array_equal(rows, want_rows)
    split.set_pairs_from_window(win)  # after read as well
    assert split.debug_pairs().tobytes() == fsplit.pairs_from_stereo_tracks(xy_t)[0].tobytes()


@functools.lru_cache(maxsize=None)
def _edge(k):
    """The first k surviving pixels of the _big window as a custom start set, each followed by a NaN start and a start
    outside the window: rows = 0, 3, 6, ..."""
    args, (_, keep) = _big()
    w = args[0].shape[2]
    px = np.stack([keep[:k] % w, keep[:k] // w], 1).astype(np.float64)
    xy0 = np.empty((3 * k, 2))
    xy0[0::3], xy0[1::3], xy0[2::3] = px, (np.nan, 1.0), (1e6, 2.0)
    want = S.stereo_track_window_host(*args, xy0=xy0)
    assert np.array_equal(want[1], 3 * np.arange(k))
    return args, xy0, want


@pytest.mark.parametrize("k", [8, 63, 64, 65, 255, 256, 257, 1025])
def test_m_at_the_edges_with_rows_that_are_not_arange(k):
    args, xy0, (xy_t, rows) = _edge(k)
    win = _counted(args, xy0)
    _buffers_equal_the_host(win, xy_t, k)
    got = win.read()
    assert got[0].tobytes() == xy_t.tobytes() and np.array_equal(got[1], rows)
    if k in (8, 65, 257):
        kw = dict(xy0=xy0, thresh=WC.TIGHT, tracks=True)
        WC.same(W.window_cameras(*args, K.CAM, K.BASELINE, **kw), W.window_cameras_host(*args, K.CAM, K.BASELINE, **kw), k,
                WC.KEYS + ("xy_t", "rows"))


@pytest.mark.parametrize("thresh", [WC.TIGHT, 2.0])
@pytest.mark.parametrize("name", WC.WINDOWS)
def test_whole_chain_equals_the_host_definition(name, thresh):
    got = W.window_cameras(*fields(golden()[name]), K.CAM, K.BASELINE, thresh=thresh)
    WC.same(got, WC.host(name, thresh), (name, thresh))
    assert "xy_t" not in got and "rows" not in got


def test_whole_chain_from_device_fields_twice_on_the_same_objects_and_with_tracks():
    import torch
    c = golden()["odd_long"]
    dev = [torch.from_numpy(np.array(a)).cuda() for a in fields(c)]
    torch.cuda.synchronize()
    want = WC.host("odd_long", WC.TIGHT)
    WC.same(W.window_cameras(*dev, K.CAM, K.BASELINE, thresh=WC.TIGHT), want)
    lr = c["disp_lr"]
    win, objects = S.StereoTrackWindow(lr.shape[2], lr.shape[1], lr.shape[0]), {}
    a = W.window_cameras(*fields(c), K.CAM, K.BASELINE, thresh=WC.TIGHT, window=win, objects=objects)
    held = (objects["split"], objects["fit"])
    b = W.window_cameras(*fields(c), K.CAM, K.BASELINE, thresh=WC.TIGHT, window=win, objects=objects, tracks=True)
    assert held == (objects["split"], objects["fit"])
    WC.same(a, want)
    WC.same(b, want, keys=WC.KEYS + ("xy_t", "rows"))
    ref = S.stereo_track_window(*fields(c))
    assert b["xy_t"].tobytes() == ref[0].tobytes() and b["rows"].tobytes() == ref[1].tobytes()
    # another schedule, start poses and offset go through as well
    kw = dict(thresh=WC.TIGHT, seed=5, ntrials=37, offset=(-0.4, 0.01, 0.0), init=np.tile(np.eye(3, 4), (lr.shape[0], 1, 1)),
              noiter=7, minres=1e-7)
    WC.same(W.window_cameras(*fields(c), K.CAM, K.BASELINE, objects=objects, **kw),
            W.window_cameras_host(*fields(c), K.CAM, K.BASELINE, **kw))


def test_frames_in_cameras_out_equals_the_host_array_stages_on_the_read_back_window():
    left, right = _stereo_frames()
    cam, baseline = ((75.0, 90.0), (49.5, 34.25)), -0.55  # synth.make_sequence at 96 x 64; the right camera of _stereo_frames
    t = S.StereoPointTracker(96, 64, 4, step=4, psz=8, lv_f=2)
    for a, b in zip(left, right):
        t.push_frames(a, b)
    got = t.cameras(cam, baseline, thresh=0.1)
    xy_t, rows = t.window()
    assert got["m"] == len(rows) > 100
    print("frames in:", got["m"], "survivors,", got["best_count"], "static, status", got["status"], "err", got["err_left"])
    WC.same(got, W.cameras_from_tracks(xy_t, cam, baseline, thresh=0.1))
    early = S.StereoPointTracker(96, 64, 4, step=4, psz=8, lv_f=2)
    early.push_frames(left[0], right[0])
    with pytest.raises(ValueError, match="frames pushed"):
        early.cameras(cam, baseline)


def test_refusals_come_with_a_message_and_launch_nothing():
    c = golden()["two_frames"]
    args = fields(c)
    m = len(c["rows"])
    lr, rl, fl, fr = args
    win = S.StereoTrackWindow(lr.shape[2], lr.shape[1], 2)
    split, fit = fsplit.StaticSplitter(m, 2), F.CameraFitter(m, 2)
    fit.set_camera(K.CAM)
    win.open(S.field(lr[0], -1), rl[0])
    for call in (lambda: split.set_pairs_from_window(win), lambda: fit.set_points_from_window(win, K.BASELINE),
                 lambda: fit.set_observations_from_window(win)):
        with pytest.raises(IctrError, match="not counted"):  # open, not counted
            call()
    win.advance(fl[0][0], fl[0][1], fr[0][0], fr[0][1], S.field(lr[1], -1), rl[1])
    with pytest.raises(IctrError, match="not counted"):
        split.set_pairs_from_window(win)
    assert win.count() == m
    with pytest.raises(IctrError, match="never run"):
        fit.set_mask_from_fsplit(split)
    for other in (fsplit.StaticSplitter(m + 1, 2), fsplit.StaticSplitter(m - 1, 2)):  # n != M
        with pytest.raises(IctrError, match="was made for"):
            other.set_pairs_from_window(win)
    with pytest.raises(IctrError, match="was made for"):
        F.CameraFitter(m + 1, 2).set_observations_from_window(win)
    nocam = F.CameraFitter(m, 2)
    with pytest.raises(IctrError, match="was made for"):  # the size is looked at first
        F.CameraFitter(m - 1, 2).set_points_from_window(win, K.BASELINE)
    with pytest.raises(IctrError, match="set_camera comes first"):
        nocam.set_points_from_window(win, K.BASELINE)
    with pytest.raises(IctrError, match="view pairs"):  # wrong npairs, wrong nframes
        fsplit.StaticSplitter(m, 4).set_pairs_from_window(win)
    with pytest.raises(IctrError, match="frames"):
        F.CameraFitter(m, 3).set_observations_from_window(win)
    # nothing was written by any of the refused calls
    assert not split.debug_pairs().any() and not fit.debug_inputs()["xy"].any() and not nocam.debug_inputs()["X"].any()
    # a setter while a run is in flight
    split.set_pairs_from_window(win)
    split.run_async(2000, WC.TIGHT, 0)
    with pytest.raises(IctrError, match="in flight"):
        split.set_pairs_from_window(win)
    fit.set_points_from_window(win, K.BASELINE)
    fit.set_observations_from_window(win)
    fit.set_mask_from_fsplit(split)
    fit.run_async()
    for call in (lambda: fit.set_points_from_window(win, K.BASELINE), lambda: fit.set_observations_from_window(win, True),
                 lambda: fit.set_mask_from_fsplit(split)):
        with pytest.raises(IctrError, match="in flight"):
            call()
    with pytest.raises(IctrError, match="points"):  # mask from a split of another size
        F.CameraFitter(m + 64, 2).set_mask_from_fsplit(split)
    split.wait()
    fit.wait()
    # bsize 1, and fewer than 8 survivors
    one = golden()["one_frame"]
    with pytest.raises(ValueError, match="bsize"):
        W.window_cameras(*fields(one), K.CAM, K.BASELINE)
    w1 = _counted(fields(one))
    with pytest.raises(ValueError, match="bsize"):
        W.cameras_from_window(w1, K.CAM, K.BASELINE)
    with pytest.raises(IctrError, match="no frame pair"):
        F.CameraFitter(w1.survivors, 1).set_observations_from_window(w1)
    xy0 = np.stack([np.arange(7) + 5.0, np.full(7, 6.0)], 1)
    with pytest.raises(ValueError, match="points"):
        W.window_cameras(*args, K.CAM, K.BASELINE, xy0=xy0)
    with pytest.raises(TypeError):
        W.window_cameras(*args, K.CAM, K.BASELINE, no_such_parameter=1)


_OBJECTS = {  # name -> (constructor of (n, nframes), C prefix, has two sides)
    "fitter": (F.CameraFitter, "camfit", False),
    "adjuster": (lambda n, f: B.BundleAdjuster(n, f, 2), "ba", True),
    "ransac": (lambda n, f: R.CameraRansac(n, f, 2), "camransac", True),
}


@pytest.mark.parametrize("name", list(_OBJECTS))
def test_every_window_stage_refuses_alike_and_takes_the_window_alike(name):
    """The from-window refusals of test_refusals_come_with_a_message_and_launch_nothing for the fitter, the adjuster and
    the RANSAC: same order, same messages, nothing written; then the good setters against the host functions. The objects
    differ in two things, kept as they are: the RANSAC takes no mask from another object's run, and its debug_inputs
    answers in words the mask in effect (every point's bit while none is set) where the other two return the buffer."""
    make, prefix, two = _OBJECTS[name]
    c = golden()["two_frames"]
    lr, rl, fl, fr = fields(c)
    xy_t, m = c["xy_t"], len(c["rows"])
    unset = F._words_of(np.ones(m, bool), m) if name == "ransac" else np.zeros((m + 63) // 64, np.uint64)

    def untouched(o, words=unset):
        d = o.debug_inputs()
        assert not d["X"].any() and not d["xy"].any() and d["words"].tobytes() == words.tobytes()

    def refused(o, call, match, words=unset):
        with pytest.raises(IctrError, match=match):
            call()
        untouched(o, words)

    obj = make(m, 2)
    obj.set_camera(K.CAM)
    win = S.StereoTrackWindow(lr.shape[2], lr.shape[1], 2)
    win.open(S.field(lr[0], -1), rl[0])
    for stage in range(2):  # open, then every frame in: not counted
        refused(obj, lambda: obj.set_points_from_window(win, K.BASELINE), "not counted")
        refused(obj, lambda: obj.set_observations_from_window(win), "not counted")
        if stage == 0:
            win.advance(fl[0][0], fl[0][1], fr[0][0], fr[0][1], S.field(lr[1], -1), rl[1])
    assert win.count() == m
    other, nocam, frames3 = make(m + 1, 2), make(m, 2), make(m, 3)  # n != M is looked at before the camera
    other_unset = F._words_of(np.ones(m + 1, bool), m + 1) if name == "ransac" else unset
    refused(other, lambda: other.set_points_from_window(win, K.BASELINE), "was made for", other_unset)
    refused(other, lambda: other.set_observations_from_window(win), "was made for", other_unset)
    refused(nocam, lambda: nocam.set_points_from_window(win, K.BASELINE), "set_camera comes first")
    refused(frames3, lambda: frames3.set_observations_from_window(win), "frames")
    # a mask from a source that never ran, and from one of another size that did
    sources = []
    if name == "ransac":
        assert not hasattr(obj, "set_mask_from_fsplit") and not hasattr(obj, "set_mask_from_camransac")
    else:
        split, ran = fsplit.StaticSplitter(m, 2), R.CameraRansac(m, 2, 1)
        refused(obj, lambda: obj.set_mask_from_fsplit(split), "never run")
        refused(obj, lambda: obj.set_mask_from_camransac(ran), "never run")
        split.set_pairs_from_window(win)
        split.run_async(8, WC.TIGHT, 0)
        ran.set_camera(K.CAM)
        ran.set_points_from_window(win, K.BASELINE)
        ran.set_observations_from_window(win)
        ran.run_async(8, 2.0, 0)
        refused(other, lambda: other.set_mask_from_fsplit(split), "points")
        refused(other, lambda: other.set_mask_from_camransac(ran), "points")
        sources = [split, ran]
    # the good setters write what the host functions give, both sides for an object of two
    obj.set_points_from_window(win, K.BASELINE)
    obj.set_observations_from_window(win)
    X = F.points_from_first_view(xy_t, K.CAM, F.depth_from_disparity(xy_t, K.FC[0], K.BASELINE))
    left, right = F.observations_from_stereo_tracks(xy_t)
    want = np.stack([left, right]) if two else left
    got = obj.debug_inputs()
    assert got["X"].tobytes() == np.ascontiguousarray(X).tobytes() and got["xy"].tobytes() == want.tobytes()
    assert got["words"].tobytes() == unset.tobytes()
    # a from-window setter while a run is in flight: refused with the object's own wait, nothing moves
    if two:
        obj.set_offset((K.BASELINE, 0.0, 0.0))
    obj.run_async(8) if name == "ransac" else obj.run_async(noiter=2)
    calls = [lambda: obj.set_points_from_window(win, K.BASELINE), lambda: obj.set_observations_from_window(win)]
    if sources:
        calls += [lambda: obj.set_mask_from_fsplit(sources[0]), lambda: obj.set_mask_from_camransac(sources[1])]
    for call in calls:
        with pytest.raises(IctrError, match="in flight.*ictr_%s_wait" % prefix):
            call()
    now = obj.debug_inputs()
    assert all(now[k].tobytes() == got[k].tobytes() for k in ("X", "xy", "words"))
    for o in sources + [obj]:
        o.wait()


def test_native_caller_and_cli(tmp_path, capsys):
    """tests/cxx/windowcams_driver.cpp (the facade of include/ctr_shim.hpp) prints the Python result in hex floats, and
    python -m invcompcamtrack_amd.run_window_cameras writes it, on the device and with --host."""
    from invcompcamtrack_amd import run_window_cameras as R
    exe = os.path.join(ROOT, "tests", "cxx", "windowcams_driver")
    src = exe + ".cpp"
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        r = subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                            src, "-L" + os.path.join(ROOT, "invcompcamtrack_amd"), "-l:libictr_hip.so",
                            "-Wl,-rpath,$ORIGIN/../../invcompcamtrack_amd"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    c = golden()["odd_long"]
    want = WC.host("odd_long", WC.TIGHT)
    lr, rl, fl, fr = (np.ascontiguousarray(a, np.float32) for a in fields(c))
    b, h, w = lr.shape
    fin = str(tmp_path / "in.bin")
    with open(fin, "wb") as f:
        f.write(np.array([h, w, b, 0], np.int64).tobytes())
        f.write(np.array([0.2, 1.0]).tobytes() + lr.tobytes() + rl.tobytes() + fl.tobytes() + fr.tobytes())
        f.write(np.array(K.FC + K.CC + (K.BASELINE, WC.TIGHT)).tobytes() + np.array([100, 0], np.int64).tobytes())
    r = subprocess.run([exe, fin], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "kept %d best_trial %d best_count %d" % (want["m"], want["best_trial"], want["best_count"])
    assert len(lines) == 1 + b
    for k, ln in enumerate(lines[1:]):
        t = ln.split()
        assert t[:9] == ["frame", str(k), "status", str(want["status"][k]), "iters", str(want["iters"][k]), "n",
                         str(want["n"][k]), "G"] and t[21] == "err"
        G = np.array([float.fromhex(v) for v in t[9:21]])
        assert G.tobytes() == want["G"][k].tobytes(), k
        err = np.array([float.fromhex(v) for v in t[22:24]])
        assert err.tobytes() == np.array([want["err_left"][k], want["err_right"][k]]).tobytes(), k
    # the CLI
    zin = str(tmp_path / "in.npz")
    np.savez(zin, fc=K.FC, cc=K.CC, baseline=K.BASELINE, **{k: c[k] for k in ("disp_lr", "disp_rl", "flow_l", "flow_r")})
    outs = []
    for extra in ([], ["--host"]):
        out = str(tmp_path / ("o%d.npz" % len(outs)))
        assert R.main([zin, out, "--thresh", str(WC.TIGHT), "--tracks"] + extra) == 0
        outs.append(open(out, "rb").read())
        with np.load(out) as z:
            assert sorted(z.files) == sorted(WC.KEYS + ("xy_t", "rows"))
            WC.same({k: z[k] for k in z.files}, {k: np.asarray(v) for k, v in want.items()}, keys=WC.KEYS + ("xy_t", "rows"))
    assert outs[0] == outs[1]
    said = capsys.readouterr().out
    assert "kept %d points in %d frames, %d static" % (want["m"], b, want["best_count"]) in said
    assert "[%.17g, %.17g]" % (want["err_left"][-1], want["err_right"][-1]) in said
    assert R.main([zin, str(tmp_path / "x.npz"), "--th_abs", "0.0"]) == 2  # no survivor: refused with a message
