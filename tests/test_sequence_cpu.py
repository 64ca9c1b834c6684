"""Sequence tracking without a GPU: the point selection against a literal restatement of run_odometer_test.m:206-213,
the file layouts of the sequence driver, and the CPU oracle chain the GPU tests compare against."""
import os
import sys

import numpy as np
import pytest

from invcompcamtrack_amd import io_formats as iof
from invcompcamtrack_amd import sequence as sq
from invcompcamtrack_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = dict(fc=np.array([64.0, 64.0], np.float32), cc=np.array([0.0, 0.0], np.float32), wh=np.array([40, 30], np.int32))


def script_select(pts3d, p, cam, stride):
    """run_odometer_test.m:206-213, literally (1-based pixel bounds, deletion of the points outside, every
    stride-th of the rest), with the projection of func_reproject written as G X."""
    G = synth.se3_exp(p)
    Xc = G[:, :3] @ pts3d + G[:, 3:]
    fc, cc, wh = cam["fc"].astype(np.float64), cam["cc"].astype(np.float64), cam["wh"]
    pt2d = np.stack([fc[0] * Xc[0] / Xc[2] + cc[0], fc[1] * Xc[1] / Xc[2] + cc[1]], 1)
    idx = np.arange(pts3d.shape[1])
    idxdel = np.nonzero((pt2d[:, 0] < 1) | (pt2d[:, 1] < 1) | (pt2d[:, 0] > wh[0]) | (pt2d[:, 1] > wh[1]))[0]
    idx = np.delete(idx, idxdel)
    return idx[0::stride]


def edge_points():
    """Points at identity pose, Z = 1: u = 64 X, v = 64 Y exactly (powers of two). On each bound and one ulp-ish step
    (2^-20 px) outside it, plus interior points."""
    eps = 2.0 ** -20
    uv = [(1, 10), (40, 10), (10, 1), (10, 30),                      # on u = 1, u = w, v = 1, v = h
          (1 - eps, 10), (40 + eps, 10), (10, 1 - eps), (10, 30 + eps),  # just outside each
          (1, 1), (40, 30)]
    rng = np.random.default_rng(1)
    uv += [tuple(x) for x in rng.uniform(0.5, 41, (60, 2))]
    uv = np.array(uv)
    return np.ascontiguousarray(np.stack([uv[:, 0] / 64.0, uv[:, 1] / 64.0, np.ones(len(uv))]))


@pytest.mark.parametrize("stride", [1, 10])
def test_select_points_matches_the_script_on_the_bounds(stride):
    X = edge_points()
    p = np.zeros(6)
    got = sq.select_points(X, p, CAM, stride)
    want = script_select(X, p, CAM, stride)
    np.testing.assert_array_equal(got, want)
    if stride == 1:
        assert set([0, 1, 2, 3, 8, 9]) <= set(got.tolist())       # on a bound: kept
        assert not set([4, 5, 6, 7]) & set(got.tolist())           # just outside: dropped


def test_select_points_general_pose_and_cap():
    rng = np.random.default_rng(2)
    X = np.ascontiguousarray(np.stack([rng.uniform(-1, 1.5, 5000), rng.uniform(-1, 1.5, 5000), rng.uniform(2, 4, 5000)]))
    p = np.array([0.05, -0.02, 0.1, 0.01, -0.02, 0.03])
    cam = dict(fc=np.array([30.0, 32.0], np.float32), cc=np.array([20.0, 15.0], np.float32), wh=CAM["wh"])
    for stride in (1, 3, 10):
        want = script_select(X, p, cam, stride)
        np.testing.assert_array_equal(sq.select_points(X, p, cam, stride), want)
        assert want.size > 20
        cap = want.size // 2  # Set3Dpoints' cap: the first cap of the selected list
        np.testing.assert_array_equal(sq.select_points(X, p, cam, stride, cap), want[:cap])


def test_select_points_without_survivors():
    X = edge_points()
    p = np.array([100.0, 0, 0, 0, 0, 0])  # everything far to the right of the frame
    assert sq.select_points(X, p, CAM, 10).size == 0
    assert script_select(X, p, CAM, 10).size == 0


def test_selection_hash_is_order_aware():
    a = np.array([3, 17, 40])
    assert sq.selection_hash(a) != sq.selection_hash(a[::-1])
    assert sq.selection_hash(a) != sq.selection_hash(a[:2])
    assert sq.selection_hash([]) == 0


def test_cli_file_layouts(tmp_path):
    # the list file
    lst = tmp_path / "list.txt"
    lst.write_text("a.pgm\n\n b.pgm \nc.pgm\n")
    assert iof.read_image_list(str(lst)) == ["a.pgm", "b.pgm", "c.pgm"]
    # the point/cam file without the reference's 10 000-point cap
    rng = np.random.default_rng(3)
    n = iof.MAXPTREAD + 5
    X = rng.normal(size=(3, n))
    fn = tmp_path / "in.bin"
    p0 = np.arange(6) * 0.1
    iof.write_pointcam_file(str(fn), p0, [500, 600], [320, 240], [640, 480], X)
    with pytest.raises(ValueError):
        iof.read_pointcam_file(str(fn))
    d = iof.read_pointcam_file_uncapped(str(fn))
    np.testing.assert_array_equal(d["pts3d"], X)
    np.testing.assert_array_equal(d["pose"], p0)
    np.testing.assert_array_equal(d["wh"], [640, 480])
    # the result: N x 6 f64, little endian, the poses in frame order
    poses = rng.normal(size=(5, 6))
    out = tmp_path / "out.bin"
    np.asarray(poses, "<f8").tofile(str(out))
    assert out.stat().st_size == 5 * 48
    np.testing.assert_array_equal(np.fromfile(str(out), "<f8").reshape(-1, 6), poses)


def test_cli_usage_without_arguments(capsys):
    from invcompcamtrack_amd import run_track_sequence
    assert run_track_sequence.main([]) == 2
    assert "listfile" in capsys.readouterr().out


def test_cpu_oracle_chain_follows_the_ground_truth(oracle):
    """The tests' own reference: oracle.Tracker per pair (a fresh process per pair, as the script runs
    run_io_reprojection_test) on a short synthetic pan lands close to the ground truth."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from seq_scene import make_pan
    O = oracle
    sc = make_pan(320, 240, 4, 1000, step=-0.25, seed=5)
    args, cap, stride = (4, 0, 4, 5, 0.01, 0, 0), 128, 10
    oop = O.make_op(*args, cap)
    poses = [sc["poses"][0]]
    pyr = [O.Pyramid(sc["frames"][0], args[0], args[2]), None]
    for t in range(3):
        pyr[1] = O.Pyramid(sc["frames"][t + 1], args[0], args[2])
        sel = sq.select_points(sc["pts3d"], poses[t], sc["cam"], stride, cap)
        assert sel.size > 20
        tr = O.Tracker(oop, sc["cam"]["fc"], sc["cam"]["cc"], sc["cam"]["wh"])
        tr.set3dpoints(np.ascontiguousarray(sc["pts3d"][:, sel]))
        tr.setpose(poses[t], pyr[0], pyr[1])
        poses.append(tr.trackpose())
        tr.close()
        pyr[0] = pyr[1]
    err = np.abs(np.array(poses) - sc["poses"]).max(1)
    assert err[-1] <= 2e-2, err


class _FakeLib:
    """Stands in for libictr_hip.so: records the calls of SequenceTracker.track_async and succeeds."""

    def __init__(self):
        self.frames_calls = []

    def ictr_sequence_set_frames(self, h, ptr, n, w, hh, on_device):
        self.frames_calls.append((int(n), int(w), int(hh), int(on_device)))
        return 0

    def ictr_sequence_set_stream(self, h, s):
        return 0

    def ictr_sequence_track_async(self, h, p0):
        return 0


def test_cpu_tensor_frames_are_copied_not_borrowed(monkeypatch):
    """A CPU tensor has a data_ptr too; it must take the host copy path (on_device = 0), never be handed to the
    device kernels as device memory."""
    torch = pytest.importorskip("torch")
    from invcompcamtrack_amd import _lib
    fake = _FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: fake)
    st = sq.SequenceTracker.__new__(sq.SequenceTracker)
    st._h, st._n, st._keep = None, 0, None
    frames = torch.zeros((3, 6, 8), dtype=torch.float32)
    st.track_async(frames, np.zeros(6))
    st.track_async(frames.numpy(), np.zeros(6))
    assert fake.frames_calls == [(3, 8, 6, 0), (3, 8, 6, 0)]
    st._h = None  # (nothing to destroy)
