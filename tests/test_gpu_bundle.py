"""The window bundle adjustment on the device against its host restatement (itself judged in test_bundle_cpu.py), bit for
bit: the system alone through ictr_debug_ba_system, whole runs, and the edges of the interface. Nothing here has a
tolerance."""
import ctypes as CT
import functools

import numpy as np
import pytest

import bundle_cases as BC
import camfit_cases as K
import invcompcamtrack_amd as ic
from invcompcamtrack_amd import bundle as B

pytestmark = pytest.mark.gpu
SIZES = (8, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
EDGES = (0, 63, 64, 255, 256, 1023, 1024, 1087, 1088, 2048)  # wave, workgroup-row and chunk boundaries
DAMPS = (0.0, 2.0, 1e-3)
STARTS = ("identity", "true", "crafted")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _base():
    """One window of 2049 points seen from two sides in 5 frames, with points that are not adjusted on the boundaries (a
    NaN observation in some frame and side, or a coordinate that is not finite), sliced for every shape."""
    w = BC.window(2049, 5, 2, 0.3, seed=930, pose_err=0.05)
    for k, e in enumerate(EDGES):
        if k % 2 == 0:
            w["xy"][k % 2, k % 5, (k // 2) % 2, e] = np.nan
    w["X0"][1, 65] = np.inf
    for a in w.values():
        a.setflags(write=False)
    return w


def _shape(n, nframes, nsides):
    w = _base()
    mask = np.random.default_rng(n).uniform(size=n) < 0.8
    mask[-1] = True  # the last word is partial wherever n is no multiple of 64, and its top bit in use
    for e in EDGES[1::2]:
        if e < n - 1:
            mask[e] = False
    poses = dict(identity=K.identity(nframes), true=w["G"][:nframes], crafted=w["G0"][:nframes])
    return (np.ascontiguousarray(w["X0"][:, :n]), np.ascontiguousarray(w["xy"][:nsides, :nframes, :, :n]), poses, mask,
            BC.OFFSET if nsides == 2 else None)


def _adjuster(X, xy, cam=BC.CAM, offset=None, mask=None):
    b = B.BundleAdjuster(X.shape[1], xy.shape[1], xy.shape[0])
    b.set_points(X)
    b.set_observations(xy)
    b.set_camera(cam)
    b.set_offset(offset)
    b.set_mask(mask)
    return b


def _system_equal(dev, host, what):
    assert dev["n"] == host["n"] and dev["nfail"] == host["nfail"], (what, dev["n"], host["n"], dev["nfail"], host["nfail"])
    for k in ("cost", "V", "gp", "A", "rhs"):
        bad = np.nonzero(_bits(dev[k]).reshape(-1) != _bits(host[k]).reshape(-1))[0]
        assert bad.size == 0, (what, k, bad[:8].tolist(), bad.size)


def _same(dev, host, what="", points=True):
    for k in ("status", "iters", "n"):
        assert dev[k] == host[k], (what, k, dev[k], host[k])
    for k in ("G", "cost", "damp", "p") + (("X",) if points else ()):
        assert np.array_equal(_bits(dev[k]), _bits(host[k])), (what, k)


def _device(c, stream=None, **kw):
    sched = dict(c["schedule"])
    sched.update(kw)
    return B.adjust_window(c["X"], c["xy"], c["cam"], offset=c["offset"], mask=c["mask"], init=c["init"], stream=stream,
                           **sched)


# ---------------------------------------------------------------- the system alone
@pytest.mark.parametrize("nsides", (1, 2))
@pytest.mark.parametrize("nframes", (2, 3, 5))
def test_system_device_equals_host(nframes, nsides):
    """n, the cost, V, gp, the reduced upper triangle and the right-hand side at every size, with and without a mask;
    the dampings and the start poses go round so that every pair of them is met."""
    left_out = seen = 0
    for i, n in enumerate(SIZES):
        X, xy, poses, mask, off = _shape(n, nframes, nsides)
        m = mask if i % 2 else None
        b = _adjuster(X, xy, offset=off, mask=m)
        for k in range(2):
            damp, start = DAMPS[(i + k) % 3], STARTS[(i // 3 + i + 2 * k) % 3]
            host = B.system_host(X, xy, BC.CAM, poses[start], damp, offset=off, mask=m)
            _system_equal(b.debug_system(poses[start], damp), host, (n, damp, start, m is not None))
            left_out += n - host["n"]
            seen += 1
            assert host["n"] >= 6
    assert left_out > 0 and seen == 22


def test_every_damping_at_every_start():
    X, xy, poses, mask, off = _shape(1025, 3, 2)
    b = _adjuster(X, xy, offset=off, mask=mask)
    for damp in DAMPS:
        for start in STARTS:
            host = B.system_host(X, xy, BC.CAM, poses[start], damp, offset=off, mask=mask)
            _system_equal(b.debug_system(poses[start], damp), host, (damp, start))
    # at points given to the call: the set ones stay
    w = _base()
    Xt = np.ascontiguousarray(w["X"][:, :1025])
    host = B.system_host(Xt, xy, BC.CAM, poses["true"], 2.0, offset=off, mask=mask)
    _system_equal(b.debug_system(poses["true"], 2.0, X=Xt), host, "given points")
    host = B.system_host(X, xy, BC.CAM, poses["true"], 2.0, offset=off, mask=mask)
    _system_equal(b.debug_system(poses["true"], 2.0), host, "set points again")


@pytest.mark.parametrize("nframes,n", ((14, 1025), (32, 65)))
def test_system_at_the_scripts_frame_count_and_at_the_upper_limit(nframes, n):
    w = BC.window(n, nframes, 2, 0.3, seed=931 + nframes, pose_err=0.02)
    mask = BC.spotted_mask(n, 5)
    b = _adjuster(w["X0"], w["xy"], offset=BC.OFFSET, mask=mask)
    host = B.system_host(w["X0"], w["xy"], BC.CAM, w["G0"], 2.0, offset=BC.OFFSET, mask=mask)
    assert host["A"].size == 6 * (nframes - 1) * (6 * (nframes - 1) + 1) // 2 and host["nfail"] == 0
    _system_equal(b.debug_system(w["G0"], 2.0), host, nframes)


# ---------------------------------------------------------------- whole runs
@functools.lru_cache(maxsize=None)
def _host_of(name):
    return BC.run_host(BC.crafted(name))


@pytest.mark.parametrize("name", sorted(BC.CRAFTED))
def test_whole_run_on_every_crafted_case(name):
    c, host = BC.crafted(name), _host_of(name)
    dev = _device(c)
    _same(dev, host, name)
    if name == "far_start":
        assert "reject" in host["trace"] and "accept" in host["trace"]
    if name in ("failed_between", "on_the_axis"):
        assert "failed-solve" in host["trace"]
    if name == "nan_observation":
        assert dev["n"] == 129 and np.array_equal(_bits(dev["X"][:, 64]), _bits(c["X"][:, 64]))


def test_script_frame_count_runs_through_the_lds_solve():
    w = BC.window(300, 14, 2, 0.3, seed=940, pose_err=0.01)
    host = B.adjust_window_host(w["X0"], w["xy"], BC.CAM, offset=BC.OFFSET, init=w["G0"], noiter=6)
    assert host["iters"] >= 3
    _same(B.adjust_window(w["X0"], w["xy"], BC.CAM, offset=BC.OFFSET, init=w["G0"], noiter=6), host, "F = 14")


def test_above_the_lds_solve():
    w = BC.window(80, 16, 1, 0.3, seed=941, pose_err=0.01)
    host = B.adjust_window_host(w["X0"], w["xy"], BC.CAM, init=w["G0"], noiter=3)
    assert host["iters"] == 3
    _same(B.adjust_window(w["X0"], w["xy"], BC.CAM, init=w["G0"], noiter=3), host, "F = 16")


def _hip_runtime():
    """The HIP runtime that libictr_hip.so runs on (already in the process), for a stream of the test's own."""
    from invcompcamtrack_amd import _lib
    _lib.load()
    for name in (None, "libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            hip = CT.CDLL(name)
            hip.hipStreamCreate, hip.hipStreamDestroy
            return hip
        except (OSError, AttributeError):
            continue
    raise RuntimeError("no HIP runtime to create a stream with")


@functools.lru_cache(maxsize=None)
def _big():
    w = BC.window(5000, 6, 2, 0.3, seed=950, pose_err=0.02)
    mask = BC.spotted_mask(5000, 6)
    return w, mask, B.adjust_window_host(w["X0"], w["xy"], BC.CAM, offset=BC.OFFSET, mask=mask, init=w["G0"])


def test_whole_run_5000_points_6_frames_and_a_stream():
    w, mask, host = _big()
    assert host["status"] == B.CONVERGED and host["n"] == int(mask.sum()) and host["iters"] >= 3
    args = (w["X0"], w["xy"], BC.CAM)
    _same(B.adjust_window(*args, offset=BC.OFFSET, mask=mask, init=w["G0"]), host, "null stream")
    hip, stream = _hip_runtime(), CT.c_void_p()
    assert hip.hipStreamCreate(CT.byref(stream)) == 0 and stream.value
    try:
        _same(B.adjust_window(*args, offset=BC.OFFSET, mask=mask, init=w["G0"], stream=stream.value), host, "stream")
    finally:
        assert hip.hipStreamDestroy(stream) == 0


def test_one_adjuster_run_four_times_equals_fresh_ones():
    c = BC.crafted("far_start")
    n = c["X"].shape[1]
    mask = np.arange(n) % 3 != 1
    b = _adjuster(c["X"], c["xy"], offset=c["offset"])
    for k, (m, kw) in enumerate(((None, {}), (mask, {}), (mask, dict(noiter=4, damp_init=0.5)), (None, dict(minres=1e-2)))):
        b.set_mask(m)
        b.run_async(c["init"], **kw)
        dev = b.wait()
        host = B.adjust_window_host(c["X"], c["xy"], c["cam"], offset=c["offset"], mask=m, init=c["init"], **kw)
        _same(dev, host, "run %d" % k)
        _same(B.adjust_window(c["X"], c["xy"], c["cam"], offset=c["offset"], mask=m, init=c["init"], **kw), dev, "fresh %d" % k)


def test_wait_without_the_points():
    c, host = BC.crafted("two_frames"), _host_of("two_frames")
    b = _adjuster(c["X"], c["xy"], offset=c["offset"])
    b.run_async(c["init"])
    dev = b.wait(points=False)
    assert dev["X"] is None
    _same(dev, host, "X = NULL", points=False)


# ---------------------------------------------------------------- edges
def test_refusals_leave_the_object_usable():
    for args in ((7, 3, 1), ((1 << 22) + 1, 3, 1), (100, 1, 1), (100, 33, 1), (100, 3, 0), (100, 3, 3)):
        with pytest.raises(ic.IctrError):
            B.BundleAdjuster(*args)
    c, host = BC.crafted("nan_observation"), _host_of("nan_observation")
    X, xy, init = c["X"], c["xy"], c["init"]
    b = B.BundleAdjuster(130, 4, 2)
    with pytest.raises(ic.IctrError):  # nothing set
        b.run_async(init)
    with pytest.raises(ic.IctrError):
        b.debug_system(init, 2.0)
    with pytest.raises(ic.IctrError):  # wait without run
        b.wait()
    with pytest.raises(ValueError):
        b.set_points(X[:, :10])
    with pytest.raises(ValueError):
        b.set_observations(xy[:, :2])
    with pytest.raises(ValueError):
        b.set_observations(xy[:1])
    with pytest.raises(ValueError):
        b.set_mask(np.ones(5, bool))
    with pytest.raises(ValueError):
        b.set_offset([0.0, np.inf, 0.0])
    with pytest.raises(ic.IctrError):
        b.set_camera(((0.0, 1000.0), K.CC))
    b.set_points(X)
    b.set_observations(xy)
    b.set_camera(c["cam"])
    with pytest.raises(ic.IctrError):  # two sides and no offset yet
        b.run_async(init)
    b.set_offset(c["offset"])
    for kw in (dict(noiter=-1), dict(noiter=1001), dict(damp_init=0.0), dict(damp_fct=1.0), dict(minres=-1.0),
               dict(minres=float("nan")), dict(maxdamp=0.0), dict(damp_init=float("inf"))):
        with pytest.raises(ic.IctrError):
            b.run_async(init, **kw)
    bad = init.copy()
    bad[2, 1, 3] = np.nan
    for call in (lambda: b.run_async(bad), lambda: b.debug_system(bad, 2.0), lambda: b.debug_system(init, -1.0),
                 lambda: b.debug_system(init, float("nan"))):
        with pytest.raises(ic.IctrError):
            call()
    with pytest.raises(ic.IctrError):  # still nothing to wait for
        b.wait()
    b.run_async(init)
    for call in (lambda: b.run_async(init), lambda: b.set_points(X), lambda: b.set_observations(xy), lambda: b.set_mask(None),
                 lambda: b.set_camera(c["cam"]), lambda: b.set_offset(c["offset"]), lambda: b.debug_system(init, 2.0),
                 lambda: b.set_timing(True)):
        with pytest.raises(ic.IctrError):  # refused while the run is in flight
            call()
    _same(b.wait(), host)
    with pytest.raises(ic.IctrError):  # the run has been waited for
        b.wait()
    with pytest.raises(ic.IctrError):  # no timed run yet
        b.kernel_times()
    b.debug_system(K.identity(4), 0.5, X=np.ascontiguousarray(X + 1.0))  # leaves no trace in the next run
    b.run_async(init)
    _same(b.wait(), host)
    b.set_timing(True)
    b.run_async(init)
    _same(b.wait(), host)
    t = b.kernel_times()
    assert set(t) == set(B.BundleAdjuster.KERNELS) and all(v > 0 for v in t.values()), t


def test_destroy_with_a_run_pending():
    w, mask, _ = _big()
    b = _adjuster(w["X0"], w["xy"], offset=BC.OFFSET)
    b.run_async(w["G0"], noiter=100, minres=0.0)
    del b
    c = BC.crafted("one_side")
    _same(_device(c), _host_of("one_side"))


# ---------------------------------------------------------------- from a window
def _window_tools():
    import windowcams_cases as WC
    from invcompcamtrack_amd import windowcams as W
    from test_gpu_windowcams import _counted
    from test_stereotrack_cpu import fields, golden
    return WC, W, _counted, fields, golden


BA_KEYS = ("G", "p", "X", "cost", "damp", "iters", "status", "n")


@functools.lru_cache(maxsize=None)
def _window_host(name):
    WC, W, _, fields, golden = _window_tools()
    return W.window_bundle_host(*fields(golden()[name]), K.CAM, K.BASELINE, thresh=WC.TIGHT)


def _bundle_same(got, want, what):
    WC = _window_tools()[0]
    WC.same(got, want, what, WC.KEYS + ("err_left_ba", "err_right_ba"))
    WC.same(got["ba"], want["ba"], what, BA_KEYS)


@pytest.mark.parametrize("name", ["small_disp", "large_disp", "odd_long", "two_frames"])
def test_bundle_from_window_equals_the_host_definition_twice_on_the_same_objects(name):
    """The fields are torch tensors on the device; whichever test of a session is the first to touch torch pays its
    start-up, the runs themselves take milliseconds."""
    import torch
    from invcompcamtrack_amd import stereotrack as S
    WC, W, _counted, fields, golden = _window_tools()
    c, want = golden()[name], _window_host(name)
    dev = [torch.from_numpy(np.array(a)).cuda() for a in fields(c)]
    torch.cuda.synchronize()
    lr = c["disp_lr"]
    win, objects = S.StereoTrackWindow(lr.shape[2], lr.shape[1], lr.shape[0]), {}
    for k in range(2):
        win.open(S.field(dev[0][0], -1), dev[1][0])
        for fr in range(1, lr.shape[0]):
            win.advance(dev[2][fr - 1][0], dev[2][fr - 1][1], dev[3][fr - 1][0], dev[3][fr - 1][1], S.field(dev[0][fr], -1),
                        dev[1][fr])
        win.count()
        got = W.bundle_from_window(win, K.CAM, K.BASELINE, thresh=WC.TIGHT, objects=objects)
        if k == 0:
            held = (objects["split"], objects["fit"], objects["ba"])
        assert held == (objects["split"], objects["fit"], objects["ba"])
        _bundle_same(got, want, (name, k))
    assert want["ba"]["status"] in (B.CONVERGED, B.NOITER, B.MAXDAMP)


@pytest.mark.parametrize("k", [8, 63, 64, 65, 257, 1025])
def test_adjuster_inputs_from_a_window_with_rows_that_are_not_arange(k):
    from invcompcamtrack_amd import camfit as F
    from test_gpu_windowcams import _counted, _edge
    args, xy0, (xy_t, rows) = _edge(k)
    assert not np.array_equal(rows, np.arange(k))
    win = _counted(args, xy0)
    b = B.BundleAdjuster(k, xy_t.shape[2], 2)
    b.set_camera(K.CAM)
    b.set_points_from_window(win, K.BASELINE)
    b.set_observations_from_window(win)
    got = b.debug_inputs()
    X = F.points_from_first_view(xy_t, K.CAM, F.depth_from_disparity(xy_t, K.FC[0], K.BASELINE))
    left, right = F.observations_from_stereo_tracks(xy_t)
    assert got["X"].tobytes() == np.ascontiguousarray(X).tobytes()
    assert got["xy"].tobytes() == np.stack([left, right]).tobytes()
    one = B.BundleAdjuster(k, xy_t.shape[2], 1)
    one.set_observations_from_window(win)
    assert one.debug_inputs()["xy"].tobytes() == left[None].tobytes()


# ---------------------------------------------------------------- the callers
def test_native_caller_and_cli_print_the_same_bytes(tmp_path, capsys):
    """tests/cxx/bundle_driver.cpp (CTR::BundleClass) and python -m invcompcamtrack_amd.run_bundle, with and without
    --host, print the same hexadecimal floats."""
    import os
    import subprocess
    from invcompcamtrack_amd import camfit as F
    from invcompcamtrack_amd import run_bundle
    from test_gpu_camfit import _cxx_driver
    w = BC.window(150, 4, 2, 0.3, seed=971, pose_err=0.02)
    mask = BC.spotted_mask(150, 7)
    words = F._words_of(mask, 150)
    fin, zin, zout = str(tmp_path / "in.bin"), str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    with open(fin, "wb") as f:
        f.write(np.array([150, 4, 2, 1], np.int64).tobytes() + np.array(K.FC + K.CC + BC.OFFSET).tobytes())
        f.write(w["X0"].tobytes() + w["xy"].tobytes() + w["G0"].tobytes() + words.tobytes())
    r = subprocess.run([_cxx_driver("bundle_driver"), fin, "20", "1e-5"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    np.savez(zin, X=w["X0"], xy=w["xy"], fc=K.FC, cc=K.CC, offset=BC.OFFSET, mask=mask, init=w["G0"])
    outs = []
    for extra in ([], ["--host"]):
        assert run_bundle.main([zin, zout] + extra) == 0
        outs.append(capsys.readouterr().out)
    assert outs[0] == outs[1] == r.stdout and len(r.stdout.splitlines()) == 1 + 4 + 150
    host = B.adjust_window_host(w["X0"], w["xy"], BC.CAM, offset=BC.OFFSET, mask=mask, init=w["G0"])
    with np.load(zout) as z:
        assert z["X"].tobytes() == host["X"].tobytes() and z["G"].tobytes() == host["G"].tobytes()
    bad = subprocess.run([_cxx_driver("bundle_driver"), fin, "-1", "1e-5"], capture_output=True, text=True)
    assert bad.returncode == 1 and "noiter" in bad.stderr
