"""The window camera RANSAC on the device against its host restatement (camransac.window_ransac_host, itself pinned to the
shared headers and judged in test_camransac_cpu.py), with tobytes() / np.array_equal on every output and no tolerance
anywhere: every trial through ictr_debug_camransac_trials at every score tile, whole runs, the hand-over, the pipeline on the
golden windows, the native caller and the CLI, and the edges of the interface."""
import functools
import os
import subprocess

import numpy as np
import pytest

import camfit_cases as K
import camransac_cases as CR
import windowcams_cases as WC
import invcompcamtrack_amd as ic
from invcompcamtrack_amd import bundle as B
from invcompcamtrack_amd import camfit as F
from invcompcamtrack_amd import camransac as R
from invcompcamtrack_amd import stereotrack as S
from invcompcamtrack_amd import windowcams as W
from test_gpu_fsplit import _hip_runtime
from test_gpu_windowcams import _counted, _edge
from test_stereotrack_cpu import fields, golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("best_trial", "best_count", "draws", "G", "p", "words", "mask", "inliers", "dd")
PIPE_KEYS = ("m",) + W._RANSAC_KEYS + ("G_ransac", "p_ransac") + W._FIT_KEYS + ("err_left", "err_right")
BA_KEYS = ("G", "p", "X", "cost", "damp", "iters", "status", "n")


def _same(got, want, what="", keys=KEYS):
    WC.same(got, want, what, keys)


# ---------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def _boundaries():
    """Points that do not count on wave, row and 256-point boundaries, by NaN on either side and by the mask."""
    X, xy, _ = CR.window(600, 3, 2, seed=9201)
    X, xy = X.copy(), xy.copy()
    mask = np.ones(600, bool)
    X[0, 63] = X[2, 256] = np.nan
    xy[0, 1, 1, 64] = xy[1, 2, 0, 255] = xy[1, 0, 1, 511] = np.inf
    mask[[0, 127, 128, 512, 599]] = False
    return CR._case(X, xy, mask=mask, seed=21)


@functools.lru_cache(maxsize=None)
def _tiling(nframes):
    X, xy, _ = CR.window(65, nframes, 2, seed=9300 + nframes)
    return CR._case(X, xy, seed=nframes)


def _case(key):
    if key == "boundaries":
        return _boundaries()
    if isinstance(key, tuple) and key[0] == "tiling":
        return _tiling(key[1])
    return CR.seeded(*key) if isinstance(key, tuple) else CR.crafted(key)


@functools.lru_cache(maxsize=None)
def _host(key):
    """The host's record of every trial, shared with test_camransac_cpu.py where that test has the case."""
    if key in CR.CRAFTED:
        return CR.host(key)
    if isinstance(key, tuple) and key[0] != "tiling":
        return CR.host_seeded(*key)
    c = _case(key)
    return WC.freeze(R.window_ransac_host(c["X"], c["xy"], c["cam"], c["offset"], c["mask"], c["ntrials"], c["thresh"],
                                          c["seed"], detail=True))


def _ransac(monkeypatch, c, tile=None, chunk=None):
    """Both variables are read at creation."""
    for k, v in (("ICTR_CAMRANSAC_TILE", tile), ("ICTR_CAMRANSAC_CHUNK", chunk)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))
    S_, Fr, _, n = c["xy"].shape
    r = R.CameraRansac(n, Fr, S_)
    r.set_points(c["X"])
    r.set_observations(c["xy"])
    r.set_camera(c["cam"])
    if S_ == 2:
        r.set_offset(c["offset"])
    r.set_mask(c["mask"])
    return r


def _trials_equal(dev, h, first, count, what):
    sl = slice(first, first + count)
    assert np.array_equal(dev["status"], h["status"][sl]), what
    assert np.array_equal(dev["draws"], h["all_draws"][sl]), what
    assert dev["G"].tobytes() == np.ascontiguousarray(h["all_G"][sl]).tobytes(), what
    assert np.array_equal(dev["cnt"], h["cnt"][sl]), what


ALL = CR.seeded_cases() + list(CR.CRAFTED) + ["boundaries", ("tiling", 33), ("tiling", 64)]


# ---------------------------------------------------------------- 1. every trial
@pytest.mark.parametrize("tile", [16, 32, 64])
def test_every_trial_device_equals_host(monkeypatch, tile):
    """k_cr_hyp and k_cr_score<tile> alone: status, draws, every frame's G and the counts of 64 trials at the CPU list's
    shapes (masks with a partial last word among them), at N = 65 with F = 33 and 64 (frame tiling), with points that do
    not count on wave, row and 256-point boundaries, and on every crafted case."""
    for key in ALL:
        c = _case(key)
        r = _ransac(monkeypatch, c, tile)
        _trials_equal(r.debug_trials(c["thresh"], c["seed"], 0, c["ntrials"]), _host(key), 0, c["ntrials"], (tile, key))


@functools.lru_cache(maxsize=None)
def _host_twice(key):
    """The host's record of 2 * TRIALS trials: room for a window of T + 1 trials at T = 64 that starts off the grid."""
    c = _case(key)
    return WC.freeze(R.window_ransac_host(c["X"], c["xy"], c["cam"], c["offset"], c["mask"], 2 * CR.TRIALS, c["thresh"],
                                          c["seed"], detail=True))


@pytest.mark.parametrize("tile", [16, 32, 64])
def test_trial_windows_off_the_tile_grid_and_chunk_tails(monkeypatch, tile):
    """One trial, and T + 1 trials from trial 3 (a second workgroup along x with one trial in its tile, at every T), then
    125 trials in chunks of 24 with a tail of 5."""
    for key in ((257, 3, 2, True), "boundaries"):
        c, h = _case(key), _host_twice(key)
        r = _ransac(monkeypatch, c, tile)
        for first, count in ((5, 1), (3, tile + 1)):
            _trials_equal(r.debug_trials(c["thresh"], c["seed"], first, count), h, first, count, (tile, key, first))
        r = _ransac(monkeypatch, c, tile, 24)
        assert r.chunk == 24
        count = 2 * CR.TRIALS - 3
        _trials_equal(r.debug_trials(c["thresh"], c["seed"], 3, count), h, 3, count, (tile, key, "chunks of 24"))


# ---------------------------------------------------------------- 2. whole runs
def _run(c, ntrials=None, stream=None, **kw):
    return R.window_ransac(c["X"], c["xy"], c["cam"], c["offset"], c["mask"], ntrials or c["ntrials"], c["thresh"],
                           c["seed"], stream=stream, **kw)


def test_whole_runs_of_the_crafted_cases(monkeypatch):
    for name in list(CR.CRAFTED) + ["boundaries"]:
        c = _case(name)
        _same(_run(c), _host(name), name)
        r = _ransac(monkeypatch, c, None, 24)
        r.run_async(c["ntrials"], c["thresh"], c["seed"])
        _same(r.wait(), _host(name), (name, "chunks of 24"))
    h = _host("all_fail")
    assert h["best_trial"] == -1 and np.isnan(h["G"]).all()


@functools.lru_cache(maxsize=None)
def _large():
    xy_t, moving, _ = K.stereo_window(n=5000, seed=77)
    X, xy = CR.stereo_inputs(xy_t)
    c = CR._case(X, xy, ntrials=300, seed=3)
    h = WC.freeze(R.window_ransac_host(c["X"], c["xy"], c["cam"], c["offset"], None, 300, 2.0, 3))
    assert h["best_count"] > 2500 and not h["mask"][moving].any()
    return c, h


def test_whole_run_5000_points_8_frames_both_sides_and_a_stream(monkeypatch):
    import ctypes as C
    c, h = _large()
    _same(_run(c), h, "one chunk")
    r = _ransac(monkeypatch, c, None, 24)
    r.run_async(300, 2.0, 3)
    _same(r.wait(), h, "chunks of 24")
    hip, stream = _hip_runtime(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
    try:
        _same(_run(c, stream=stream.value), h, "stream")
    finally:
        assert hip.hipStreamDestroy(stream) == 0


@pytest.mark.parametrize("chunk", [None, 24])
def test_one_object_run_four_times_equals_fresh_ones(monkeypatch, chunk):
    c = _case((257, 8, 2, False))
    r = _ransac(monkeypatch, c, None, chunk)
    for ntrials, thresh, seed, mask in ((64, 2.0, 0, None), (64, 2.0, 5, None), (40, 0.7, 5, None),
                                        (40, 2.0, 5, CR.mask_of(257))):
        r.set_mask(mask)
        r.run_async(ntrials, thresh, seed)
        dev = r.wait()
        _same(dev, R.window_ransac_host(c["X"], c["xy"], c["cam"], c["offset"], mask, ntrials, thresh, seed),
              (chunk, ntrials, thresh, seed))
        d = dict(c, mask=mask)
        fresh = _ransac(monkeypatch, d, None, chunk)
        fresh.run_async(ntrials, thresh, seed)
        _same(fresh.wait(), dev)


# ---------------------------------------------------------------- 3. hand-over
@pytest.mark.parametrize("k", [8, 63, 64, 65, 257, 1025])
def test_inputs_from_the_window_and_the_words_handed_on(k):
    """The object's device X and xy after set_*_from_window against the host repacking, with rows that are not arange; the
    fitter's and the adjuster's mask words after set_mask_from_camransac, in flight and after the wait."""
    args, xy0, (xy_t, rows) = _edge(k)
    win = _counted(args, xy0)
    b = xy_t.shape[2]
    r = R.CameraRansac(k, b, 2)
    r.set_camera(K.CAM)
    r.set_offset(CR.OFFSET)
    r.set_points_from_window(win, K.BASELINE)
    r.set_observations_from_window(win)
    X, xy = CR.stereo_inputs(xy_t)
    got = r.debug_inputs()
    assert got["X"].tobytes() == np.ascontiguousarray(X).tobytes() and got["xy"].tobytes() == xy.tobytes(), k
    every = F._words_of(np.ones(k, bool), k)   # the mask in effect: every point before a mask is set and after None
    assert got["words"].tobytes() == every.tobytes(), k
    r.set_mask(CR.mask_of(k))
    assert r.debug_inputs()["words"].tobytes() == F._words_of(CR.mask_of(k), k).tobytes(), k
    r.set_mask(None)
    assert r.debug_inputs()["words"].tobytes() == every.tobytes(), k
    fit, ba = F.CameraFitter(k, b), B.BundleAdjuster(k, b, 2)
    r.run_async(50, 0.05, 1)
    fit.set_mask_from_camransac(r)
    ba.set_mask_from_camransac(r)
    in_flight = (fit.debug_inputs()["words"], ba.debug_inputs()["words"])
    dev = r.wait()
    _same(dev, R.window_ransac_host(X, xy, K.CAM, CR.OFFSET, None, 50, 0.05, 1), k)
    assert in_flight[0].tobytes() == in_flight[1].tobytes() == dev["words"].tobytes()
    fit.set_mask(np.zeros(k, bool))
    fit.set_mask_from_camransac(r)
    assert fit.debug_inputs()["words"].tobytes() == dev["words"].tobytes()
    one = R.CameraRansac(k, b, 1)   # one side: only the left observations are written
    one.set_observations_from_window(win)
    assert one.debug_inputs()["xy"].tobytes() == xy[:1].tobytes()


# ---------------------------------------------------------------- 4. pipeline
def _pipe_same(got, want, what, bundle):
    _same(got, want, what, PIPE_KEYS)
    if bundle:
        _same(got["ba"], want["ba"], what, BA_KEYS)
        _same(got, want, what, ("err_left_ba", "err_right_ba"))


@pytest.mark.parametrize("bundle", [False, True])
@pytest.mark.parametrize("name", WC.WINDOWS)
def test_pipeline_equals_the_host_definition_from_device_fields_twice(name, bundle):
    import torch
    c = golden()[name]
    kw = dict(thresh=0.05, bundle=bundle)
    want = W.window_ransac_cameras_host(*fields(c), K.CAM, K.BASELINE, **kw)
    assert want["best_trial"] >= 0 and 4 <= want["best_count"] < want["m"]
    dev = [torch.from_numpy(np.array(a)).cuda() for a in fields(c)]
    torch.cuda.synchronize()
    lr = c["disp_lr"]
    win, objects = S.StereoTrackWindow(lr.shape[2], lr.shape[1], lr.shape[0]), {}
    for turn in range(2):
        got = W.ransac_cameras(*dev, K.CAM, K.BASELINE, window=win, objects=objects, **kw)
        _pipe_same(got, want, (name, bundle, turn), bundle)
    held = objects["ransac"]
    got = W.ransac_cameras_from_window(win, K.CAM, K.BASELINE, objects=objects, **kw)
    assert objects["ransac"] is held
    _pipe_same(got, want, (name, "from the window"), bundle)


def test_pipeline_with_a_winner_that_has_no_inlier():
    c = golden()["two_frames"]
    kw = dict(thresh=float("-inf"), ntrials=3)   # no distance is below it, but trials succeed: the winner counts 0
    want = W.window_ransac_cameras_host(*fields(c), K.CAM, K.BASELINE, **kw)
    got = W.ransac_cameras(*fields(c), K.CAM, K.BASELINE, **kw)
    assert want["best_trial"] >= 0 and want["best_count"] == 0 and (want["status"] == F.FEW_OBS).all()
    _pipe_same(got, want, "count 0", False)


def _driver():
    exe = os.path.join(ROOT, "tests", "cxx", "camransac_driver")
    src = exe + ".cpp"
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        r = subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                            src, "-L" + os.path.join(ROOT, "invcompcamtrack_amd"), "-l:libictr_hip.so",
                            "-Wl,-rpath,$ORIGIN/../../invcompcamtrack_amd"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    return exe


def _hex(tokens):
    return np.array([float.fromhex(v) for v in tokens])


def test_native_caller_and_cli(tmp_path, capsys):
    """tests/cxx/camransac_driver.cpp (CTR::CamRansacClass and the mask hand-over of CTR::CamFitClass) prints the Python
    result in hexadecimal floats; python -m invcompcamtrack_amd.run_window_ransac writes the same bytes on the device and
    with --host."""
    from invcompcamtrack_amd import run_window_ransac
    key = (257, 3, 2, True)
    c, h = _case(key), _host(key)
    words = F._words_of(c["mask"], 257)
    fin = str(tmp_path / "in.bin")
    with open(fin, "wb") as f:
        f.write(np.array([257, 3, 2, 1], np.int64).tobytes())
        f.write(np.array(F._as_cam(c["cam"]) + tuple(c["offset"])).tobytes())
        f.write(c["X"].tobytes() + c["xy"].tobytes() + words.tobytes())
    r = subprocess.run([_driver(), fin, str(c["ntrials"]), repr(c["thresh"]), str(c["seed"])], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "best_trial %d best_count %d draws %d %d %d %d" % ((h["best_trial"], h["best_count"]) +
                                                                          tuple(h["draws"]))
    for k in range(3):
        t = lines[1 + k].split()
        assert t[:3] == ["frame", str(k), "G"] and t[15] == "p"
        assert _hex(t[3:15]).tobytes() == h["G"][k].tobytes() and _hex(t[16:22]).tobytes() == h["p"][k].tobytes()
    assert lines[4].split()[1:] == ["%016x" % w for w in h["words"]]
    assert _hex(lines[5].split()[1:]).tobytes() == h["dd"].tobytes()
    fit = F.fit_cameras_host(c["X"], c["xy"][0], c["cam"], mask=h["words"], init=h["G"])
    for k in range(3):
        t = lines[6 + k].split()
        assert t[:7] == ["fit", str(k), "status", str(fit["status"][k]), "iters", str(fit["iters"][k]), "G"]
        assert _hex(t[7:19]).tobytes() == fit["G"][k].tobytes()
    # the CLI
    g = golden()["odd_long"]
    zin = str(tmp_path / "in.npz")
    np.savez(zin, fc=K.FC, cc=K.CC, baseline=K.BASELINE, **{k: g[k] for k in ("disp_lr", "disp_rl", "flow_l", "flow_r")})
    want = W.window_ransac_cameras_host(*fields(g), K.CAM, K.BASELINE, thresh=0.05, seed=2, ntrials=60, bundle=True)
    outs = []
    for extra in ([], ["--host"]):
        out = str(tmp_path / ("o%d.npz" % len(outs)))
        assert run_window_ransac.main([zin, out, "--thresh", "0.05", "--seed", "2", "--ntrials", "60", "--bundle"] + extra) == 0
        outs.append(open(out, "rb").read())
        with np.load(out) as z:
            got = {k: z[k] for k in z.files}
        _same(got, want, extra, PIPE_KEYS + ("err_left_ba", "err_right_ba"))
        _same({k: got["ba_" + k] for k in BA_KEYS}, want["ba"], extra, BA_KEYS)
    assert outs[0] == outs[1]
    assert "%d inliers of trial %d" % (want["best_count"], want["best_trial"]) in capsys.readouterr().out


# ---------------------------------------------------------------- 5. edges
def test_refusals_leave_the_object_usable(monkeypatch):
    for n, f, s in ((3, 2, 2), ((1 << 22) + 1, 2, 2), (100, 0, 2), (100, 65, 2), (100, 2, 0), (100, 2, 3)):
        with pytest.raises(ic.IctrError):
            R.CameraRansac(n, f, s)
    key = (65, 3, 2, False)
    c, h = _case(key), _host(key)
    monkeypatch.delenv("ICTR_CAMRANSAC_CHUNK", raising=False)
    r = R.CameraRansac(65, 3, 2)
    with pytest.raises(ic.IctrError, match="come first"):
        r.run_async(10, 2.0, 0)
    with pytest.raises(ic.IctrError):  # wait without run
        r.wait()
    with pytest.raises(ValueError):
        r.set_observations(c["xy"][:, :2])
    with pytest.raises(ValueError):
        r.set_points(c["X"][:, :64])
    r.set_points(c["X"])
    r.set_observations(c["xy"])
    for bad in (((0.0, 1.0), (1.0, 1.0)), ((1.0, float("nan")), (1.0, 1.0))):
        with pytest.raises(ic.IctrError):
            r.set_camera(bad)
    r.set_camera(c["cam"])
    with pytest.raises(ic.IctrError, match="set_offset"):  # S = 2 without an offset
        r.run_async(10, 2.0, 0)
    with pytest.raises(ic.IctrError, match="set_offset"):
        r.debug_trials(2.0, 0, 0, 4)
    with pytest.raises(ic.IctrError):
        r.set_offset([0.0, float("inf"), 0.0])
    r.set_offset(c["offset"])
    for ntrials, thresh in ((0, 2.0), ((1 << 20) + 1, 2.0), (10, float("nan"))):
        with pytest.raises(ic.IctrError):
            r.run_async(ntrials, thresh, 0)
    for first, count in ((0, 0), (-1, 4), (0, (1 << 20) + 1), ((1 << 20) - 3, 4)):
        with pytest.raises(ic.IctrError):
            r.debug_trials(2.0, 0, first, count)
    with pytest.raises(ic.IctrError):  # still nothing to wait for
        r.wait()
    r.run_async(c["ntrials"], c["thresh"], c["seed"])
    for call in (lambda: r.run_async(10, 2.0, 1), lambda: r.set_points(c["X"]), lambda: r.set_mask(None),
                 lambda: r.set_offset(c["offset"]), lambda: r.debug_trials(2.0, 1, 0, 4)):
        with pytest.raises(ic.IctrError, match="in flight"):  # run twice, setters and inspection while a run is in flight
            call()
    _same(r.wait(), h)
    with pytest.raises(ic.IctrError):  # the run has been waited for
        r.wait()
    r.debug_trials(2.0, 9, 3, 20)  # leaves no trace in the next run
    r.set_timing(True)
    r.run_async(c["ntrials"], c["thresh"], c["seed"])
    _same(r.wait(), h)
    t = r.kernel_times()
    assert t["score"] > 0 and all(v >= 0 for v in t.values()), t
    with pytest.raises(ic.IctrError, match="never run"):
        F.CameraFitter(65, 3).set_mask_from_camransac(R.CameraRansac(65, 3, 1))
    with pytest.raises(ic.IctrError, match="points"):
        F.CameraFitter(66, 3).set_mask_from_camransac(r)


def test_destroy_with_a_run_pending():
    c, _ = _large()
    r = R.CameraRansac(5000, 8, 2)
    r.set_points(c["X"])
    r.set_observations(c["xy"])
    r.set_camera(c["cam"])
    r.set_offset(c["offset"])
    r.run_async(2000, 2.0, 0)
    del r
    key = (65, 2, 2, False)
    _same(_run(_case(key)), _host(key))
