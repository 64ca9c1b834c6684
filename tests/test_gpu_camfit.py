"""The camera fit on the device against its host restatement (itself judged in test_camfit_cpu.py), bit for bit: the pass
alone through ictr_debug_camfit_pass, whole runs, the reprojection means, the edges of the interface, and the chain
split_static -> depth -> fit_cameras with the native caller and the CLI."""
import functools
import os
import subprocess

import numpy as np
import pytest

import camfit_cases as K
import invcompcamtrack_amd as ic
from invcompcamtrack_amd import camfit as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = F.CHUNK
SIZES = (3, 4, 63, 64, 65, C - 1, C, C + 1, 2 * C + 1)
FRAMES = (1, 2, 10)
EDGES = (0, 63, 64, 255, 256, C - 1, C, C + 63, C + 64, 2 * C)  # wave, workgroup-row and chunk boundaries


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _base():
    """One window of 2 C + 1 points in 10 frames with NaN observations on the boundaries, sliced for every shape."""
    X, xy, G = K.window(2 * C + 1, 10, 0.3, seed=900)
    for f in range(10):
        for k, e in enumerate(EDGES):
            if (k + f) % 2 == 0:
                xy[f, k % 2, e] = np.nan
    X[1, 65] = np.inf
    for a in (X, xy, G):
        a.setflags(write=False)
    return X, xy, G


def _shape(n, nframes):
    X, xy, G = _base()
    mask = np.random.default_rng(n).uniform(size=n) < 0.8
    mask[-1] = True  # the last word is partial wherever n is no multiple of 64, and its top bit in use
    return np.ascontiguousarray(X[:, :n]), np.ascontiguousarray(xy[:nframes, :, :n]), G[:nframes], mask


def _fitter(X, xy, cam=K.CAM, mask=None):
    f = F.CameraFitter(X.shape[1], xy.shape[0])
    f.set_points(X)
    f.set_observations(xy)
    f.set_camera(cam)
    f.set_mask(mask)
    return f


def _pass_equal(dev, host, what):
    assert np.array_equal(dev["n"], host["n"]), what
    for k in ("s", "H", "b"):
        bad = np.nonzero(_bits(dev[k]).reshape(len(host["n"]), -1) != _bits(host[k]).reshape(len(host["n"]), -1))[0]
        assert bad.size == 0, (what, k, "frames", sorted(set(bad.tolist())))


def _same(dev, host, what=""):
    for k in ("status", "iters", "n"):
        assert np.array_equal(dev[k], host[k]), (what, k, dev[k], host[k])
    for k in ("G", "cost", "damp", "p"):
        assert np.array_equal(_bits(dev[k]), _bits(host[k])), (what, k)


# ---------------------------------------------------------------- 6. the pass alone
@pytest.mark.parametrize("nframes", FRAMES)
def test_pass_device_equals_host(nframes):
    counted = 0
    for n in SIZES:
        X, xy, G, mask = _shape(n, nframes)
        for m in (None, mask):
            f = _fitter(X, xy, mask=m)
            for name, poses in (("identity", K.identity(nframes)), ("true", G)):
                host = F.pass_host(X, xy, K.CAM, poses, mask=m)
                _pass_equal(f.debug_pass(poses), host, "N %d F %d mask %s at %s" % (n, nframes, m is not None, name))
                counted += int(host["n"].sum())
                assert np.isfinite(host["H"]).all() and (host["n"] <= n).all()
        if n > 65:
            assert (F.pass_host(X, xy, K.CAM, G)["n"] < n).all()  # the NaN observations and the infinite point are left out
    assert counted > 0


def test_pass_on_the_crafted_cases():
    for name in K.CRAFTED:
        c = K.crafted(name)
        f = _fitter(c["X"], c["xy"], c["cam"], c["mask"])
        host = F.pass_host(c["X"], c["xy"], c["cam"], c["init"], mask=c["mask"])
        _pass_equal(f.debug_pass(c["init"]), host, name)
    host = F.pass_host(**{k: K.crafted("depth_zero_at_start")[k] for k in ("X", "xy", "cam")}, G=K.identity())
    assert not np.isfinite(host["s"][0])  # the comparison above covered sums that are not finite


# ---------------------------------------------------------------- 7. whole runs
def test_whole_runs_on_the_crafted_cases():
    seen = set()
    for name in K.CRAFTED:
        c = K.crafted(name)
        host = F.fit_cameras_host(c["X"], c["xy"], c["cam"], mask=c["mask"], init=c["init"], **c["schedule"])
        dev = F.fit_cameras(c["X"], c["xy"], c["cam"], mask=c["mask"], init=c["init"], **c["schedule"])
        _same(dev, host, name)
        seen.add(int(host["status"][0]))
    assert seen == {F.CONVERGED, F.NOITER, F.MAXDAMP, F.FEW_OBS, F.START_NOT_FINITE}


def _hip_runtime():
    """The HIP runtime that libictr_hip.so runs on (already in the process), for a stream of the test's own."""
    import ctypes as CT
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
    X, xy, G = K.window(5000, 10, 0.3, seed=800)
    return X, xy, G, F.fit_cameras_host(X, xy, K.CAM)


def test_whole_run_5000_points_10_frames_and_a_stream():
    import ctypes as CT
    X, xy, G, host = _big()
    assert (host["status"] == F.CONVERGED).all() and np.abs(host["G"] - G).max() < 1e-3
    _same(F.fit_cameras(X, xy, K.CAM), host, "null stream")
    hip, stream = _hip_runtime(), CT.c_void_p()
    assert hip.hipStreamCreate(CT.byref(stream)) == 0 and stream.value
    try:
        _same(F.fit_cameras(X, xy, K.CAM, stream=stream.value), host, "stream")
    finally:
        assert hip.hipStreamDestroy(stream) == 0


def _mixed():
    """Six frames of one run that stop at different iterations: a start at the true pose, a frame without observations,
    noisy and noise-free frames of growing motion."""
    X, xy, G = K.window(700, 6, 0.0, seed=830)
    xy[1] = np.nan
    xy[3] += np.random.default_rng(1).normal(0, 0.3, xy[3].shape)
    xy[4] += np.random.default_rng(2).normal(0, 2.0, xy[4].shape)
    init = K.identity(6)
    init[0] = G[0]
    return X, xy, init


def test_frames_of_one_run_stop_at_different_iterations():
    X, xy, init = _mixed()
    host = F.fit_cameras_host(X, xy, K.CAM, init=init)
    assert host["status"][1] == F.FEW_OBS and host["iters"][0] == 0 and len(set(host["iters"].tolist())) >= 3
    _same(F.fit_cameras(X, xy, K.CAM, init=init), host, "mixed")
    _same(F.fit_cameras(X, xy, K.CAM, init=init, noiter=3), F.fit_cameras_host(X, xy, K.CAM, init=init, noiter=3), "noiter 3")


def test_one_fitter_run_four_times_equals_fresh_ones():
    X, xy, init = _mixed()
    mask = np.arange(700) % 3 != 1
    f = _fitter(X, xy)
    for k, (m, kw) in enumerate(((None, {}), (mask, {}), (mask, dict(noiter=4, damp_init=0.5)), (None, dict(minres=1e-2)))):
        f.set_mask(m)
        f.run_async(init, **kw)
        dev = f.wait()
        _same(dev, F.fit_cameras_host(X, xy, K.CAM, mask=m, init=init, **kw), "run %d" % k)
        _same(F.fit_cameras(X, xy, K.CAM, mask=m, init=init, **kw), dev, "fresh %d" % k)


def test_reprojection_errors_with_and_without_an_offset():
    X, xy, G, host = _big()
    mask = np.arange(5000) % 7 != 0
    for m in (None, mask):
        for off in (None, [K.BASELINE, 0.0, 0.0], [0.1, -0.2, 0.3]):
            he, hn = F.reprojection_errors_host(X, xy, K.CAM, host["G"], mask=m, offset=off)
            de, dn = F.reprojection_errors(X, xy, K.CAM, host["G"], mask=m, offset=off)
            assert np.array_equal(dn, hn) and np.array_equal(_bits(de), _bits(he)), (m is not None, off)
    assert 0.2 < he.min() and hn[0] == int(mask.sum())
    c = K.crafted("all_masked")
    de, dn = F.reprojection_errors(c["X"], c["xy"], c["cam"], c["init"], mask=c["mask"])
    assert dn[0] == 0 and _bits(de)[0] == 0x7ff8000000000000


# ---------------------------------------------------------------- 8. edges
def test_refusals_leave_the_object_usable():
    for n, nframes in ((0, 1), ((1 << 22) + 1, 1), (100, 0), (100, 4097)):
        with pytest.raises(ic.IctrError):
            F.CameraFitter(n, nframes)
    X, xy, init = _mixed()
    host = F.fit_cameras_host(X, xy, K.CAM, init=init)
    f = F.CameraFitter(700, 6)
    with pytest.raises(ic.IctrError):  # nothing set
        f.run_async(init)
    with pytest.raises(ic.IctrError):
        f.debug_pass(init)
    with pytest.raises(ic.IctrError):
        f.reprojection_errors(init)
    with pytest.raises(ic.IctrError):  # wait without run
        f.wait()
    with pytest.raises(ValueError):
        f.set_points(X[:, :10])
    with pytest.raises(ValueError):
        f.set_observations(xy[:2])
    with pytest.raises(ValueError):
        f.set_mask(np.ones(5, bool))
    with pytest.raises(ic.IctrError):
        f.set_camera(((0.0, 1000.0), K.CC))
    f.set_points(X)
    f.set_observations(xy)
    with pytest.raises(ic.IctrError):  # still no camera
        f.run_async(init)
    f.set_camera(K.CAM)
    for kw in (dict(noiter=-1), dict(noiter=1001), dict(damp_init=0.0), dict(damp_fct=1.0), dict(minres=-1.0),
               dict(minres=float("nan")), dict(maxdamp=0.0), dict(damp_init=float("inf"))):
        with pytest.raises(ic.IctrError):
            f.run_async(init, **kw)
    bad = init.copy()
    bad[2, 1, 3] = np.nan
    for call in (lambda: f.run_async(bad), lambda: f.debug_pass(bad), lambda: f.reprojection_errors(bad),
                 lambda: f.reprojection_errors(init, offset=[0.0, np.inf, 0.0])):
        with pytest.raises(ic.IctrError):
            call()
    with pytest.raises(ic.IctrError):  # still nothing to wait for
        f.wait()
    f.run_async(init)
    for call in (lambda: f.run_async(init), lambda: f.set_points(X), lambda: f.set_observations(xy), lambda: f.set_mask(None),
                 lambda: f.set_camera(K.CAM), lambda: f.debug_pass(init), lambda: f.reprojection_errors(init),
                 lambda: f.set_timing(True)):
        with pytest.raises(ic.IctrError):  # refused while the run is in flight
            call()
    _same(f.wait(), host)
    with pytest.raises(ic.IctrError):  # the run has been waited for
        f.wait()
    with pytest.raises(ic.IctrError):  # no timed run yet
        f.kernel_times()
    f.debug_pass(K.identity(6))  # leaves no trace in the next run
    f.reprojection_errors(host["G"], offset=[1.0, 0.0, 0.0])
    f.run_async(init)
    _same(f.wait(), host)
    f.set_timing(True)
    f.run_async(init)
    _same(f.wait(), host)
    t = f.kernel_times()
    assert t["pass"] > 0 and t["step"] > 0, t


def test_destroy_with_a_run_pending():
    X, xy, G, _ = _big()
    f = _fitter(X, xy)
    f.run_async(noiter=200, minres=0.0)
    del f
    c = K.crafted("nan_masked_and_not")
    _same(F.fit_cameras(c["X"], c["xy"], c["cam"], mask=c["mask"]),
          F.fit_cameras_host(c["X"], c["xy"], c["cam"], mask=c["mask"]))


# ---------------------------------------------------------------- 9. the chain and the callers
def _cxx_driver(name):
    exe = os.path.join(ROOT, "tests", "cxx", name)
    src = exe + ".cpp"
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        r = subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                            src, "-L" + os.path.join(ROOT, "invcompcamtrack_amd"), "-l:libictr_hip.so",
                            "-Wl,-rpath,$ORIGIN/../../invcompcamtrack_amd"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    return exe


def test_chain_on_the_device_native_caller_and_cli(tmp_path, capsys):
    """The stereo window of test_camfit_cpu.py through split_static and fit_cameras on the device: the bits of the host
    chain. tests/cxx/camfit_driver.cpp (CTR::CamFitClass) and python -m invcompcamtrack_amd.run_fit_cameras, with and
    without --host, print the same bytes."""
    from invcompcamtrack_amd import fsplit as S
    from invcompcamtrack_amd import run_fit_cameras
    xy_t, moving, _ = K.stereo_window()
    hsplit, X, left, right, hfit = K.chain_host(xy_t)
    pairs, rows = S.pairs_from_stereo_tracks(xy_t)
    split = S.split_static(pairs)
    assert np.array_equal(split["words"], hsplit["words"]) and not split["mask"][moving].any()
    words = split["words"]
    fit = F.fit_cameras(X, left, K.CAM, mask=words)
    _same(fit, hfit, "chain")
    off = [K.BASELINE, 0.0, 0.0]
    for obs, o in ((left, None), (right, off)):
        de, dn = F.reprojection_errors(X, obs, K.CAM, fit["G"], mask=words, offset=o)
        he, hn = F.reprojection_errors_host(X, obs, K.CAM, hfit["G"], mask=words, offset=o)
        assert np.array_equal(dn, hn) and np.array_equal(_bits(de), _bits(he))
    # the native caller and the CLI on the chain's fit
    n, nframes = X.shape[1], left.shape[0]
    fin = str(tmp_path / "in.bin")
    with open(fin, "wb") as f:
        f.write(np.array([n, nframes, 1], np.int64).tobytes() + np.array(K.FC + K.CC).tobytes())
        f.write(X.tobytes() + left.tobytes() + K.identity(nframes).tobytes() + words.tobytes())
    r = subprocess.run([_cxx_driver("camfit_driver"), fin, "20", "1e-05"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    zin, zout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(zin, X=X, xy=left, fc=K.FC, cc=K.CC, mask=words)
    capsys.readouterr()
    outs = []
    for extra in ([], ["--host"]):
        assert run_fit_cameras.main([zin, zout] + extra) == 0
        with np.load(zout) as z:
            outs.append((capsys.readouterr().out, {k: z[k].tobytes() for k in z.files}))
    assert outs[0] == outs[1] and r.stdout == outs[0][0] and len(r.stdout.splitlines()) == nframes
    assert outs[0][1]["G"] == hfit["G"].tobytes()
    # the script's chain and its per-frame pair of numbers
    np.savez(zin, xy_t=xy_t, fc=K.FC, cc=K.CC, baseline=K.BASELINE)
    outs = []
    for extra in ([], ["--host"]):
        assert run_fit_cameras.main([zin, zout, "--stereo"] + extra) == 0
        with np.load(zout) as z:
            outs.append((capsys.readouterr().out, {k: z[k].tobytes() for k in z.files}))
    assert outs[0] == outs[1] and len(outs[0][0].splitlines()) == 8
