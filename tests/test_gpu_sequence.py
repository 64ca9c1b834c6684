"""Frame-to-frame sequence tracking on the device (ictr_sequence_*, invcompcamtrack_amd.sequence) against the same loop
on the host through the public per-pair API, against the CPU oracle chain and against the ground truth."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import invcompcamtrack_amd as ic
from invcompcamtrack_amd import io_formats as iof
from invcompcamtrack_amd import sequence as sq
from seq_scene import bound_margin, make_pan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, optparam args without maxpttrack, maxpttrack, stride, expected form: 1 = single workgroup, > 1 = team)
SETS = {
    "p8_single": ((4, 0, 8, 10, 0.01, 1, 1), 128, 10, "single"),
    "p8_team": ((4, 0, 8, 10, 0.01, 1, 1), 400, 2, "team"),
    "p4_single": ((4, 0, 4, 5, 0.01, 0, 0), 128, 10, "single"),
}
W, H, NF, NW = 640, 480, 10, 2000


@pytest.fixture(scope="module")
def scene():
    # a plane turned 0.5 rad away from frame 0's optical axis (depth varies across the view, which pins translation
    # against rotation); seed 8: no point within 1e-3 px of a cull bound at any frame, at the ground truth or at the
    # tracked poses
    sc = make_pan(W, H, NF, NW, step=-0.5, seed=8, tilt=0.5)
    return sc


def _setup(sc, args, cap):
    op = ic.optparam(*args, cap)
    cam = ic.CamClass(args[0] + 1, sc["cam"]["fc"], sc["cam"]["cc"], sc["cam"]["wh"], args[2])
    return op, cam


@pytest.fixture(scope="module")
def runs(scene):
    out = {}
    for name, (args, cap, stride, _) in SETS.items():
        op, cam = _setup(scene, args, cap)
        st = sq.SequenceTracker(cam, op, scene["pts3d"], stride)
        st.track_async(scene["frames"], scene["poses"][0])
        dev = st.wait()
        dev["hash"] = st.selection_hashes()
        dev["team"] = st.last_team
        host = sq.track_sequence_host_loop(cam, op, scene["pts3d"], scene["frames"], scene["poses"][0], stride,
                                           return_selection=True)
        out[name] = (dev, host, op, cam)
    return out


def test_scene_has_no_point_on_a_bound(scene, runs):
    """f64 ulp differences (device vs host exp map) cannot flip a selection: no point within 1e-3 px of a bound at any
    pose either chain starts a pair from, or at the ground truth."""
    for dev, host, _, _ in runs.values():
        for p in list(dev["poses"]) + list(host["poses"]) + list(scene["poses"]):
            assert bound_margin(scene["pts3d"], p, scene["cam"]) > 1e-3


@pytest.mark.parametrize("name", list(SETS))
def test_launch_form_follows_the_cap(runs, name):
    dev = runs[name][0]
    if SETS[name][3] == "single":
        assert dev["team"] == 1
    else:
        assert dev["team"] > 1


@pytest.mark.parametrize("name", list(SETS))
def test_device_chain_equals_host_loop(runs, name):
    dev, host, op, _ = runs[name]
    # the scene makes points leave and enter: the counts change along the sequence
    assert len(set(host["npts"].tolist())) > 1 or SETS[name][3] == "team"
    assert (host["npts"] > 0).all()
    want_hash = np.array([sq.selection_hash(s) for s in host["selection"]], np.uint64)
    np.testing.assert_array_equal(dev["npts"], host["npts"])
    np.testing.assert_array_equal(dev["hash"], want_hash)
    np.testing.assert_array_equal(dev["iters"], host["iters"])
    assert np.abs(dev["poses"] - host["poses"]).max() <= 1e-5
    np.testing.assert_array_equal(dev["poses"][0], host["poses"][0])


@pytest.mark.parametrize("name", list(SETS))
def test_device_chain_vs_cpu_oracle_chain(scene, runs, oracle, name):
    dev, _, op, cam = runs[name]
    args, cap, stride, _ = SETS[name]
    O = oracle
    oop = O.make_op(*args, cap)
    poses = [np.asarray(scene["poses"][0], np.float64)]
    npts = []
    step = []  # each pair tracked by the oracle from the DEVICE's starting pose: one tracking against one tracking
    pyr = [O.Pyramid(scene["frames"][0], args[0], args[2]), None]

    def oracle_pair(p, t, pyr):
        sel = sq.select_points(scene["pts3d"], p, scene["cam"], stride, op.maxpttrack)
        tr = O.Tracker(oop, scene["cam"]["fc"], scene["cam"]["cc"], scene["cam"]["wh"])  # a fresh process per pair
        tr.set3dpoints(np.ascontiguousarray(scene["pts3d"][:, sel]))
        tr.setpose(p, pyr[0], pyr[1])
        out = tr.trackpose()
        tr.close()
        return sel.size, out

    for t in range(NF - 1):
        pyr[1] = O.Pyramid(scene["frames"][t + 1], args[0], args[2])
        n, p = oracle_pair(poses[t], t, pyr)
        npts.append(n)
        poses.append(p)
        step.append(oracle_pair(dev["poses"][t], t, pyr)[1])
        pyr[0] = pyr[1]
    poses = np.array(poses)
    np.testing.assert_array_equal(dev["npts"], np.array(npts))
    # every tracking of the chain within the project's pose bar of the oracle's tracking of the same pair
    assert np.abs(dev["poses"][1:] - np.array(step)).max() <= 1e-4
    # the two chains: each pair starts where its own chain ended, so the per-pair differences compound over nine
    # dependent pairs (the plane's tilt makes the later pairs sensitive to their start); 1e-3 for the whole chain
    assert np.abs(dev["poses"] - poses).max() <= 1e-3
    assert np.abs(dev["poses"][-1] - scene["poses"][-1]).max() <= 1e-2


def test_hand_off_alone(scene):
    """maxiter = 0, two frames: p_1 is the device's setpose / getpose round trip of p_0 on the selected points."""
    args = (4, 0, 8, 0, 0.01, 1, 1)
    op, cam = _setup(scene, args, 64)
    r = sq.track_sequence(cam, op, scene["pts3d"], scene["frames"][:2], scene["poses"][0], 10)
    sel = sq.select_points(scene["pts3d"], scene["poses"][0], cam, 10, op.maxpttrack)
    odo = ic.OdometerClass(ic.PoseClass(cam, op), op)
    odo.Set3Dpoints(np.ascontiguousarray(scene["pts3d"][:, sel]))
    pa = ic.Pyramid(scene["frames"][0], 4, 8)  # (Pyramid(img, lv_f, padding))
    pb = ic.Pyramid(scene["frames"][1], 4, 8)
    odo.SetPose(scene["poses"][0], pa, pb)
    want = odo.TrackPose()
    got = r["poses"][1]
    assert r["iters"][0] == 0 and r["npts"][0] == sel.size
    assert np.all(np.abs(got - want) <= np.maximum(1e-6 * np.abs(want), 1e-9)), (got, want)


def test_deterministic(scene):
    args, cap, stride, _ = SETS["p8_team"]
    op, cam = _setup(scene, args, cap)
    st = sq.SequenceTracker(cam, op, scene["pts3d"], stride)
    outs = []
    for _ in range(2):
        st.track_async(scene["frames"], scene["poses"][0])
        outs.append(st.wait())
    for k in ("poses", "npts", "iters"):
        assert outs[0][k].tobytes() == outs[1][k].tobytes()


def test_no_host_synchronisation_per_frame():
    torch = pytest.importorskip("torch")
    sc = make_pan(320, 240, 32, 1000, step=-0.01, seed=9)
    args, cap, stride, _ = SETS["p8_single"]
    op, cam = _setup(sc, args, cap)
    frames = torch.from_numpy(sc["frames"]).cuda()
    ref = sq.track_sequence(cam, op, sc["pts3d"], sc["frames"], sc["poses"][0], stride)
    st = sq.SequenceTracker(cam, op, sc["pts3d"], stride)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(400_000_000)  # well over 0.1 s of GPU time in front of the sequence
        t0 = time.perf_counter()
        st.track_async(frames, sc["poses"][0], stream=stream)
        dt = time.perf_counter() - t0
        busy = not stream.query()
    out = st.wait()
    assert busy, "the stream drained during track_async: the host waited for the GPU"
    assert dt < 0.05, dt
    for k in ("poses", "npts", "iters"):
        assert out[k].tobytes() == ref[k].tobytes()


@pytest.mark.parametrize("name", ["p8_single", "p8_team"])
def test_lost_from_the_start(scene, name):
    """The camera is moved far aside: no point survives the cull of frame 0, nor of any later (carried) pose. Every
    pair's tracking still runs, on an empty record (both launch forms), and its result is not used."""
    args, cap, stride, form = SETS[name]
    op, cam = _setup(scene, args, cap)
    st = sq.SequenceTracker(cam, op, scene["pts3d"], stride)
    p0 = scene["poses"][0] + np.array([100.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    st.track_async(scene["frames"][:5], p0)
    r = st.wait()
    assert (st.last_team > 1) == (form == "team")
    assert (r["npts"] == 0).all() and (r["iters"] == 0).all()
    np.testing.assert_array_equal(r["poses"], np.tile(p0, (5, 1)))
    # and the same tracker then follows the real sequence
    st.track_async(scene["frames"], scene["poses"][0])
    assert (st.wait()["npts"] > 0).all()


def test_lost_track_carries_the_pose(scene):
    args, cap, stride, _ = SETS["p8_single"]
    op, cam = _setup(scene, args, cap)
    # points in a strip at the left edge of frame 0 leave the view as the camera pans: tracked pairs, then lost ones
    sc = make_pan(W, H, 9, 3000, step=-1.2, seed=3, strip=(0.02, 0.2))
    dev = sq.track_sequence(cam, op, sc["pts3d"], sc["frames"], sc["poses"][0], stride)
    host = sq.track_sequence_host_loop(cam, op, sc["pts3d"], sc["frames"], sc["poses"][0], stride)
    np.testing.assert_array_equal(dev["npts"], host["npts"])
    lost = np.nonzero(dev["npts"] == 0)[0]
    assert dev["npts"][0] > 0 and lost.size > 0
    k = lost[0]
    assert (dev["iters"][lost] == 0).all()
    np.testing.assert_array_equal(dev["poses"][k + 1:], np.tile(dev["poses"][k], (len(dev["poses"]) - k - 1, 1)))
    # the pairs just before the loss track a handful of points (a nearly singular normal matrix), where the device's
    # summation order (f64 normalisation sums) moves the result by up to ~1e-3; the 1e-5 parity of well-posed pairs is
    # test_device_chain_equals_host_loop's
    assert np.abs(dev["poses"] - host["poses"]).max() <= 1e-2


def _nothing_enqueued(st):
    # a run that was enqueued would be waitable; nothing was launched when the wait finds no run
    with pytest.raises(ic.IctrError, match="ictr error 4:.*nothing has been tracked"):
        st.wait()


def test_refusals(scene):
    args, cap, stride, _ = SETS["p8_single"]
    op, cam = _setup(scene, args, cap)
    st = sq.SequenceTracker(cam, op, scene["pts3d"], stride)
    _nothing_enqueued(st)
    with pytest.raises(ic.IctrError, match="ictr error 1:.*robust"):
        st.set_robust(1)
    with pytest.raises(ic.IctrError, match="ictr error 1:.*at least 2"):
        st.track_async(scene["frames"][:1], scene["poses"][0])
    _nothing_enqueued(st)
    with pytest.raises(ic.IctrError, match="ictr error 1:.*camera"):
        st.track_async(np.zeros((3, H, W + 2), np.float32), scene["poses"][0])
    _nothing_enqueued(st)
    op4, cam4 = _setup(scene, (4, 0, 4, 5, 0.01, 0, 0), 4096)
    with pytest.raises(ic.IctrError, match="ictr error 1:.*one-launch"):
        sq.SequenceTracker(cam4, op4, scene["pts3d"], 10)
    # the tracker still works after the refused calls
    st.track_async(scene["frames"][:3], scene["poses"][0])
    assert st.wait()["npts"].shape == (2,)


def test_destroy_with_a_run_pending(scene):
    """A tracker dropped with its run in flight ends that run before its buffers, ring pyramids and inner batch go; a
    fresh one then gives what the host loop gives (the bars of test_device_chain_equals_host_loop)."""
    args, cap, stride, _ = SETS["p8_single"]
    op, cam = _setup(scene, args, cap)
    frames, p0 = scene["frames"][:3], scene["poses"][0]
    st = sq.SequenceTracker(cam, op, scene["pts3d"], stride)
    st.track_async(frames, p0)
    del st
    st = sq.SequenceTracker(cam, op, scene["pts3d"], stride)
    st.track_async(frames, p0)
    dev = st.wait()
    host = sq.track_sequence_host_loop(cam, op, scene["pts3d"], frames, p0, stride, return_selection=True)
    assert (host["npts"] > 0).all()
    np.testing.assert_array_equal(dev["npts"], host["npts"])
    want_hash = np.array([sq.selection_hash(s) for s in host["selection"]], np.uint64)
    np.testing.assert_array_equal(st.selection_hashes(), want_hash)
    np.testing.assert_array_equal(dev["iters"], host["iters"])
    assert np.abs(dev["poses"] - host["poses"]).max() <= 1e-5
    np.testing.assert_array_equal(dev["poses"][0], host["poses"][0])


def test_inputs_stay_fixed_while_a_run_is_in_flight(scene):
    args, cap, stride, _ = SETS["p8_single"]
    op, cam = _setup(scene, args, cap)
    st = sq.SequenceTracker(cam, op, scene["pts3d"], stride)
    ref = sq.track_sequence(cam, op, scene["pts3d"], scene["frames"][:4], scene["poses"][0], stride)
    st.track_async(scene["frames"][:4], scene["poses"][0])
    with pytest.raises(ic.IctrError, match="ictr error 4:.*in flight"):
        st.track_async(scene["frames"][:6], scene["poses"][0])  # set_frames is refused
    with pytest.raises(ic.IctrError, match="ictr error 4:.*in flight"):
        ic._lib.check(ic._lib.load().ictr_sequence_set_points(st._h, ic._lib.dp(np.ascontiguousarray(scene["pts3d"]))))
    out = st.wait()  # the run in flight is still the one that comes back, with its own layout
    for k in ("poses", "npts", "iters"):
        assert out[k].tobytes() == ref[k].tobytes()
    assert st.selection_hashes().shape == (3,)


def test_cli_and_cxx_driver(tmp_path, scene):
    args, cap, stride, _ = SETS["p8_single"]
    names = []
    for k in range(4):
        fn = tmp_path / f"f{k}.pgm"
        img = np.clip(scene["frames"][k], 0, 255).astype(np.uint8)
        fn.write_bytes(b"P5\n%d %d\n255\n" % (W, H) + img.tobytes())
        names.append(str(fn))
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(names) + "\n")
    inf = tmp_path / "in.bin"
    iof.write_pointcam_file(str(inf), scene["poses"][0], scene["cam"]["fc"], scene["cam"]["cc"], scene["cam"]["wh"],
                            scene["pts3d"])
    argv = [str(a) for a in args] + [str(cap), str(stride)]
    out_py = tmp_path / "out_py.bin"
    subprocess.check_call([sys.executable, "-m", "invcompcamtrack_amd.run_track_sequence", str(lst), str(inf),
                           str(out_py)] + argv, cwd=ROOT, timeout=300)
    exe = tmp_path / "sequence_driver"
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "cxx", "sequence_driver.cpp"),
                           "-L" + os.path.join(ROOT, "invcompcamtrack_amd"), "-l:libictr_hip.so",
                           "-Wl,-rpath," + os.path.join(ROOT, "invcompcamtrack_amd")], timeout=300)
    out_cx = tmp_path / "out_cx.bin"
    subprocess.check_call([str(exe), str(lst), str(inf), str(out_cx)] + argv, timeout=300)
    assert out_py.read_bytes() == out_cx.read_bytes()
    frames = np.stack([iof.read_image_gray(n) for n in names]).astype(np.float32)
    op, cam = _setup(scene, args, cap)
    api = sq.track_sequence(cam, op, scene["pts3d"], frames, scene["poses"][0], stride)
    got = np.fromfile(str(out_py), "<f8").reshape(-1, 6)
    assert got.tobytes() == api["poses"].tobytes()
