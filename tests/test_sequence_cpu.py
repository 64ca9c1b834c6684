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


# ---------------------------------------------------------------- the selection case table (tests/seq_select_cases.py)
# Conditions on the INPUTS of tests/test_gpu_sequence_select.py, decided by select_points alone: every case reaches the
# workgroup bounds, cap limits and cull edges it is in the table for.
import math  # noqa: E402

import seq_select_cases as sc  # noqa: E402


def test_identity_pose_gives_the_identity_exactly():
    from invcompcamtrack_amd._hostmath import se3_exp_d
    np.testing.assert_array_equal(se3_exp_d(np.zeros(6)), np.eye(4)[:3])


@pytest.mark.parametrize("case", list(sc.TABLE))
def test_case_selections_contain_the_workgroups_they_name(case):
    wname, _, reach = sc.TABLE[case]
    wd = sc.world(wname)
    got = set()
    for _, stride, _, cap in sc.runs(case):
        sel = sc.expected(case, stride, cap)
        assert sel.size <= cap
        got |= set((sel // sc.C).tolist())
    assert reach <= got, (sorted(reach), sorted(got))
    assert max(reach, default=0) < sc.nblk(wd["X"].shape[1])
    assert bool(reach) == (case != "none") and (got or case == "none")
    if wd["keep"] is not None:  # the world keeps exactly the points it was built to keep
        np.testing.assert_array_equal(sc.survivors(case), np.nonzero(wd["keep"])[0])


def test_case_tail1_and_edge_pairs():
    assert sc.world("tail1")["X"].shape[1] == sc.C + 1 and sc.nblk(sc.C + 1) == 2
    assert sc.expected("tail1", 1, 2048).tolist() == list(range(2048))          # the cap binds inside workgroup 0
    assert sc.expected("tail1", 1, 8192).tolist() == list(range(sc.C + 1))      # never: the last workgroup's one point
    assert sc.expected("edge_pairs", 1, 2048).tolist() == [sc.C - 1, sc.C, 2 * sc.C - 1, 2 * sc.C]
    counts = np.bincount(sc.survivors("edge_pairs") // sc.C, minlength=3)
    assert np.cumsum(counts)[:2].tolist() == [1, 3]                              # `before` of workgroups 1 and 2


def test_case_phase_carries_the_stride_over_two_bounds():
    nw = sc.world("phase")["X"].shape[1]
    assert nw == 2 * sc.C + 100
    for _, stride, _, cap in sc.runs("phase"):
        sel = sc.expected("phase", stride, cap)
        np.testing.assert_array_equal(sel, np.arange(0, nw, stride)[:cap])
        if stride >= nw:
            assert sel.tolist() == [0]                                           # stride >= total keeps rank 0 only
    for stride in (3, 7):  # the first rank of workgroups 1 and 2 is no multiple of the stride: the phase is carried
        assert sc.C % stride != 0 and (2 * sc.C) % stride != 0
        sel = sc.expected("phase", stride, 4096)
        assert {0, 1, 2} <= set((sel // sc.C).tolist())


def test_case_cap_at_bound_limits():
    for _, stride, _, cap in sc.runs("cap_at_bound"):
        sel = sc.expected("cap_at_bound", stride, cap)
        assert cap % 4 == 0 and cap * stride == sc.CAP_LIMITS[(stride, cap)]
        assert len(sel) == cap
        assert len(sc.expected("cap_at_bound", stride, 1 << 30)) > cap          # the uncapped list is longer
        assert sel[-1] == (cap - 1) * stride
    lim = sorted(set(sc.CAP_LIMITS.values()))
    assert lim == [sc.C, sc.C + 4, 4 * 1366, 2 * sc.C + 1780]
    assert sc.expected("cap_at_bound", 1366, 4)[-1] == sc.C + 2                  # the last selected point: workgroup 1
    assert sc.expected("cap_at_bound", 1, 4100)[-1] == sc.C + 3
    assert sc.expected("cap_at_bound", 1, 4096)[-1] == sc.C - 1                  # the limit at the end of workgroup 0
    assert sc.expected("cap_at_bound", 9, 1108)[-1] // sc.C == 2                 # mid workgroup 2


def test_case_holes_slots_sparse():
    s = sc.survivors("holes")
    counts = np.bincount(s // sc.C, minlength=5)
    assert sc.world("holes")["X"].shape[1] == 4 * sc.C + 613 and 613 % 64 != 0
    assert counts[0] == 0 and counts[2] == 0 and counts[1] > 1000 and counts[3] > 1000 and counts[4] > 100
    s = sc.survivors("slots")
    slot = s // 64                                                               # (workgroup, step, wave) in world order
    assert slot.tolist() == list(range(2 * sc.C // 64))                          # exactly one per slot
    lanes = (s % 64).reshape(2, 64)
    assert all(sorted(l.tolist()) == list(range(64)) for l in lanes)             # each at a different lane
    s = sc.survivors("sparse")
    counts = np.bincount(s // sc.C, minlength=6)
    assert sc.world("sparse")["X"].shape[1] == 5 * sc.C + 613
    assert 100 < s.size < 400 and (counts > 0).all()
    masks = np.bincount(s // 64, minlength=sc.nblk(5 * sc.C + 613) * 64)
    assert (masks == 0).sum() > 200                                              # many (step, wave) slots count zero


def test_case_bounds_keeps_exactly_the_points_on_a_bound():
    sp, kp = sc.bounds_specials()
    assert sp.shape[1] == 15 and kp.sum() == 7
    got = sq.select_points(sp, sc.P_ZERO, sc.CAM_ID, 1)
    np.testing.assert_array_equal(got, np.nonzero(kp)[0])
    np.testing.assert_array_equal(got, [0, 1, 2, 3, 8, 9, 13])                   # four bounds, two corners, Z < 0 inside
    # one ulp outside is not on the bound
    assert sp[0, 4] * 32 < 1.0 and sp[0, 5] * 32 > sc.W and sp[1, 6] * 32 < 1.0 and sp[1, 7] * 32 > sc.H
    wd = sc.world("bounds")
    s = sc.survivors("bounds")
    np.testing.assert_array_equal(s, np.nonzero(wd["keep"])[0])
    assert s.size == 6 * 7
    ends = set()
    for blk in range(3):
        head, tail = wd["keep"][blk * sc.C:blk * sc.C + 15], wd["keep"][blk * sc.C + sc.C - 15:(blk + 1) * sc.C]
        assert head.sum() == 7 and tail.sum() == 7
        assert wd["keep"][blk * sc.C + 15:blk * sc.C + sc.C - 15].sum() == 0
        ends |= {(blk, 0, bool(head[0])), (blk, 1, bool(tail[-1]))}
    assert {e[2] for e in ends} == {True, False}   # first / last lanes of a workgroup: kept in some, dropped in others


@pytest.mark.parametrize("case", ["many_wg_30", "many_wg_01"])
def test_case_many_wg_takes_a_second_trip_through_the_prefix_loop(case):
    nw = sc.world(case)["X"].shape[1]
    assert nw == 257 * sc.C + 5 and nw // sc.C == 257       # 257 full workgroups and one of five points
    assert sc.nblk(nw) == 258 and sc.nblk(nw) > sc.BLOCK    # thread tid of seq_prefix also adds cnt[tid + 256]
    counts = np.bincount(sc.survivors(case) // sc.C, minlength=258)
    assert counts[256] > 0 and counts[257] > 0
    frac = sc.survivors(case).size / nw
    assert abs(frac - (0.3 if case == "many_wg_30" else 0.001)) < 0.1 * (0.3 if case == "many_wg_30" else 0.001)
    assert sc.expected(case, 1, 2048).size == (2048 if case == "many_wg_30" else sc.survivors(case).size)


def test_case_general_has_no_point_on_a_bound():
    from seq_scene import bound_margin
    wd = sc.world("general")
    assert wd["X"].shape[1] == 3 * sc.C + 37 and np.abs(wd["p0"]).min() > 0
    assert bound_margin(wd["X"], wd["p0"], wd["cam"]) > 1e-6
    s = sc.survivors("general")
    assert 0.1 < s.size / wd["X"].shape[1] < 0.9
    np.testing.assert_array_equal(s, script_select(wd["X"], wd["p0"], wd["cam"], 1))


def test_kept_points_of_the_identity_worlds_are_well_inside():
    """A kept filler point projects at least half a pixel inside the view and a dropped one far outside, so that only
    the `bounds` case decides anything on a bound."""
    for case, (wname, _, _) in sc.TABLE.items():
        wd = sc.world(wname)
        if wd["keep"] is None or case == "bounds":
            continue
        X = wd["X"]
        u, v = 32.0 * X[0] / X[2], 32.0 * X[1] / X[2]
        k = wd["keep"]
        assert not k.any() or u[k].min() > 1.5 and u[k].max() < sc.W - 0.5 and v[k].min() > 1.5 and v[k].max() < sc.H - 0.5
        assert k.all() or u[~k].min() > 10 * sc.W


@pytest.mark.parametrize("case,stride,cap", [("phase", 3, 4096), ("holes", 1, 4096), ("sparse", 10, 2048),
                                             ("edge_pairs", 1, 2048), ("many_wg_30", 1000, 2048),
                                             ("general", 1, 4096)])
def test_finish_sums_restatement_against_fsum(case, stride, cap):
    """The restated order (256 strided partial sums, then the halving tree) against exactly rounded sums. Any order of
    n f64 additions is within (n - 1) u sum|terms| of the exact sum, u = 2^-53 (Higham, Accuracy and Stability of
    Numerical Algorithms, eq. 4.4 to first order), and fsum rounds the exact sum once; so the means differ by at most
    n 2^-53 sum|terms| / n. varval's terms are formed about the restated mean, itself off by that much, hence twice the
    bound there. The bound is derived, not measured: it guards the restatement against a misreading of the kernel's
    order (a sum that skips or repeats a term misses it by orders of magnitude), not the other way round."""
    wd = sc.world(sc.TABLE[case][0])
    sel = sc.expected(case, stride, cap)
    n = sel.size
    assert n > 0
    ms, varval = sc.finish_sums(wd["X"], sel)
    P = wd["X"][:, sel]
    u = 2.0 ** -53
    ms_ref = np.array([math.fsum(P[c]) / n for c in range(3)])
    for c in range(3):
        assert abs(ms[c] - ms_ref[c]) <= n * u * math.fsum(np.abs(P[c])) / n
    terms = (P[0] - ms_ref[0]) ** 2 + (P[1] - ms_ref[1]) ** 2 + (P[2] - ms_ref[2]) ** 2
    assert abs(varval - math.fsum(terms) / n) <= 2 * n * u * math.fsum(terms) / n
    if n > 1:
        assert varval > 0


def test_finish_sums_order_is_the_strided_one():
    """Terms chosen so that the order shows: thread 0 adds 1e16, 1, -1e16 (its 256-strided terms) left to right."""
    t = np.zeros(3 * 256)
    t[0], t[256], t[512] = 1e16, 1.0, -1e16
    t[1] = 3.0
    assert sc._kernel_order_sum(t) == 3.0        # (1e16 + 1) - 1e16 = 0 in thread 0; thread 1 holds 3
    t[256], t[257] = 0.0, 1.0                    # now the 1 is thread 1's: 3 + 1, and thread 0 cancels exactly
    assert sc._kernel_order_sum(t) == 4.0
    t2 = np.zeros(256)
    t2[0], t2[128], t2[1] = 1e16, -1e16, 1.0     # the tree's first level adds slot 128 onto slot 0
    assert sc._kernel_order_sum(t2) == 1.0
