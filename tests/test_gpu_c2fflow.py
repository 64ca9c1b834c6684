"""Coarse-to-fine dense flow on the device (csrc/ictr_c2fflow.hip) against its f32 restatement (c2fflow_f32.py), bit for bit
and with nothing left out: per table entry and per level the node displacements, the status bytes and the level's field,
and the final field, so that every figure c2fflow_cases.py records for the restatement against the definition
(patchflow.c2f_flow_host) is the device's too. Then the exact properties of the rule on the device, the hand-over to the
refinement, the refusals, the C++ facade, the stereo pipeline and the CLI.

The device pyramids are built from the host pyramids' planes, so that both sides read the same bits."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import c2fflow_cases as CC
import c2fflow_f32 as R
import invcompcamtrack_amd as ic
from invcompcamtrack_amd import patchflow as pf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATUS_CASE = next(c for c in CC.TABLE if c[0] == "status-96x64")

_pyrs = {}


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):  # the host pyramids are the oracle's
    return oracle


def pyramids(frame, pad, lv_f=2):
    """Device pyramids holding the planes of c2fflow_cases.host_pyramids."""
    if (frame, pad, lv_f) not in _pyrs:
        w, h = CC.frame_size(frame)
        _pyrs[frame, pad, lv_f] = tuple(ic.Pyramid(lv_f=lv_f, imgpadding=pad, wh=(w, h), host_planes=(o.img, o.dx, o.dy))
                                        for o in CC.host_pyramids(frame, pad, lv_f))
    return _pyrs[frame, pad, lv_f]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _flow(case, **over):
    frame, psz, lv_f, maxiter, eps, _, step = case
    w, h = CC.frame_size(frame)
    kw = dict(maxiter=maxiter, eps=eps, refine=CC.refine_of(case))
    kw.update(over)
    return pf.CoarseToFineFlow(w, h, lv_f, step, psz, **kw)


def _same_as_restatement(c, case, want=None):
    field, stages = want or CC.restated(case)
    for level, f, d, status in stages:
        gf, gd, gs = c.level(level)
        assert np.array_equal(gs, status), (case, level, "status")
        assert np.array_equal(_bits(gd), _bits(d)), (case, level, "d")
        assert np.array_equal(_bits(gf), _bits(f)), (case, level, "field")
    assert np.array_equal(_bits(c.dense()), _bits(field)), (case, "final field")


# ---------------------------------------------------------------- the table, bit for bit
@pytest.mark.parametrize("case", CC.TABLE, ids=lambda c: "-".join(str(v) for v in c))
def test_table_has_the_restatements_bits(case):
    c = _flow(case).run(*pyramids(case[0], CC.pad_of(case)))
    _same_as_restatement(c, case)


@pytest.mark.parametrize("case", CC.STATUS_FORMS, ids=lambda c: f"psz{c[1]}")
def test_every_status_has_the_restatements_bits_in_the_other_forms(case):
    """The status pair at psz 15 (form <4,1>) and 17 (form <8,2>): the restatement's run holds every status value 0..4,
    and at every level d, status and the field have its bits."""
    want = CC.restated(case)
    seen = np.zeros(5, int)
    for _, _, _, status in want[1]:
        seen += np.bincount(status.ravel(), minlength=5)
    assert len(want[1]) == 3 and (seen > 0).all(), seen
    c = _flow(case).run(*pyramids(case[0], CC.pad_of(case)))
    _same_as_restatement(c, case, want)


def test_same_bits_twice_on_a_stream_and_timed():
    from test_gpu_flowrefine import _hip_runtime
    case = CC.TABLE[0]
    pa, pb = pyramids(case[0], CC.pad_of(case))
    c = _flow(case).run(pa, pb)
    _same_as_restatement(c, case)
    _same_as_restatement(c.run(pa, pb), case)  # twice from one object
    hip, stream = _hip_runtime(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
    try:
        _same_as_restatement(c.run(pa, pb, stream=stream.value), case)
        c.set_timing(True)
        ms = c.run(pa, pb, stream=stream.value).kernel_ms()
        assert ms.shape == (3, 3) and (ms[:, :2] > 0).all() and (ms[:, 2] >= 0).all()
        _same_as_restatement(c, case)
        c.set_timing(False)
        assert not c.run(pa, pb).kernel_ms().any()
    finally:
        assert hip.hipStreamDestroy(stream) == 0
    frame, psz, lv_f, maxiter, eps, _, step = case
    assert np.array_equal(_bits(pf.c2f_flow(pa, pb, step, psz, lv_f, maxiter=maxiter, eps=eps)), _bits(CC.restated(case)[0]))
    other = _flow(case).run(pa, pb)  # its buffer receives the result on the device
    assert other.device_ptr() and other.device_ptr() != c.device_ptr()
    c.dense(out=other.device_ptr(), on_device=True)
    assert np.array_equal(_bits(other.dense()), _bits(CC.restated(case)[0]))


# ---------------------------------------------------------------- exact properties, on the device
def test_maxiter_0_gives_zeros_at_every_level():
    for case in (CC.TABLE[0], STATUS_CASE):
        c = _flow(case, maxiter=0).run(*pyramids(case[0], CC.pad_of(case)))
        for level in range(case[2], -1, -1):
            field, d, status = c.level(level)
            assert not _bits(field).any() and not _bits(d).any(), (case, level)
            assert np.isin(status, (pf.C2F_TRACKED, pf.C2F_HELD_COND)).all()


def test_held_nodes_keep_their_starts_bits_and_lost_ones_start_out_of_view():
    case = STATUS_CASE
    step, lv_f = case[6], case[2]
    c = _flow(case).run(*pyramids(case[0], CC.pad_of(case)))
    seen = np.zeros(5, int)
    coarse = None
    for level in range(lv_f, -1, -1):
        field, d, status = c.level(level)
        h, w = field.shape[:2]
        init = R.init_of(coarse, w, h, step)
        held = status >= pf.C2F_HELD_COND
        assert np.array_equal(_bits(d[held]), _bits(init[held])), level
        xs, ys = np.meshgrid(np.arange(step // 2, w, step), np.arange(step // 2, h, step))
        sx, sy = (xs.astype(np.float32) + init[..., 0]), (ys.astype(np.float32) + init[..., 1])  # as the kernel forms them
        out = ~((sx >= 0) & (sx <= w) & (sy >= 0) & (sy <= h))
        assert np.array_equal(status == pf.C2F_LOST, out), level
        seen += np.bincount(status.ravel(), minlength=5)
        coarse = field
    assert (seen > 0).all(), seen


def test_one_level_without_held_or_lost_nodes_is_the_densifier_on_the_same_nodes():
    case = next(c for c in CC.TABLE if c[0] == "farxy-320x64" and c[1] == 8)
    frame, psz, _, maxiter, eps, _, step = case
    w, h = CC.frame_size(frame)
    pa, pb = pyramids(frame, CC.pad_of(case))
    c = pf.CoarseToFineFlow(w, h, 0, step, psz, maxiter=maxiter, eps=eps).run(pa, pb)
    field, d, status = c.level(0)
    assert (status == pf.C2F_TRACKED).all()
    g = pf.FlowGrid(w, h, step).set_nodes(d, np.zeros(status.shape, np.uint8))
    assert np.array_equal(_bits(pf.FlowDensifier(w, h).run(g, pa, pb, psz).dense()), _bits(field))
    assert np.array_equal(_bits(c.dense()), _bits(field))


def test_the_object_is_a_field_source_of_the_refiner():
    case = CC.TABLE[0]
    frame, psz = case[0], case[1]
    w, h = CC.frame_size(frame)
    pa, pb = pyramids(frame, CC.pad_of(case))
    c = _flow(case).run(pa, pb)
    r = pf.FlowRefiner(w, h, n_outer=2, n_sor=3)
    want = r.run(pa, pb, c.dense()).dense().copy()
    assert np.array_equal(_bits(r.run(pa, pb, c).dense()), _bits(want))
    with pytest.raises(ValueError, match="where the frames are"):
        pf.FlowRefiner(w + 1, h, n_outer=1).run(pa, pb, c)


def test_refusals_say_why():
    pa, pb = pyramids("67x53", 9)
    with pytest.raises(ic.IctrError, match="has no node"):
        pf.CoarseToFineFlow(67, 53, 2, step=40)
    with pytest.raises(ic.IctrError, match=r"psz is 33 \(1 .. 32\)"):
        pf.CoarseToFineFlow(67, 53, 2, psz=33)
    with pytest.raises(ic.IctrError, match="smaller than 2 px"):
        pf.CoarseToFineFlow(9, 7, 3, step=1)
    with pytest.raises(ic.IctrError, match="refinement needs 4 x 4"):
        pf.CoarseToFineFlow(9, 7, 2, step=2, refine={})
    with pytest.raises(ic.IctrError, match="padding must be >= psz"):
        pf.CoarseToFineFlow(67, 53, 2, psz=10).run(pa, pb)
    with pytest.raises(ic.IctrError, match="fewer than lv_f"):
        pf.CoarseToFineFlow(67, 53, 3, psz=8).run(pa, pb)
    with pytest.raises(ic.IctrError, match="of the object"):
        pf.CoarseToFineFlow(68, 53, 2, psz=8).run(pa, pb)
    with pytest.raises(ic.IctrError, match="no run yet"):
        pf.CoarseToFineFlow(67, 53, 2).dense()
    with pytest.raises(TypeError, match="unknown parameter"):
        pf.CoarseToFineFlow(67, 53, 2, densify=dict(sigma=1))


# ---------------------------------------------------------------- the C++ facade
def test_cxx_driver(tmp_path):
    """tests/cxx/c2fflow_driver.cpp (CTR::CoarseFlowClass of include/ctr_shim.hpp) prints the Python call's bits."""
    exe = str(tmp_path / "c2fflow_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "c2fflow_driver.cpp"),
                           "-L" + os.path.join(ROOT, "invcompcamtrack_amd"), "-l:libictr_hip.so",
                           "-Wl,-rpath," + os.path.join(ROOT, "invcompcamtrack_amd")], timeout=300)
    frame, lv_f, step = "67x53", 2, 4
    a, b = CC.pair(frame)
    frames = str(tmp_path / "frames.f32")
    np.stack([a, b]).astype(np.float32).tofile(frames)
    for psz, maxiter, eps, refine in ((8, 10, 0.01, 0), (23, 3, 0.0, 1)):
        pad = psz + 1
        r = subprocess.run([exe, frames, "67", "53", str(pad), str(lv_f), str(step), str(psz), str(maxiter), repr(eps),
                            str(refine)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.splitlines()
        got = np.array([[float.fromhex(t) for t in ln.split()] for ln in lines[:67 * 53]], np.float32)
        pa, pb = ic.Pyramid(a, lv_f, pad, True), ic.Pyramid(b, lv_f, pad, True)
        c = pf.CoarseToFineFlow(67, 53, lv_f, step, psz, maxiter=maxiter, eps=eps,
                                refine=dict(n_outer=refine, n_sor=2) if refine else None).run(pa, pb)
        assert np.array_equal(_bits(got.reshape(53, 67, 2)), _bits(c.dense())), (psz, refine)
        for ln, level in zip(lines[67 * 53:], range(lv_f, -1, -1)):
            assert [int(t) for t in ln.split()[1:]] == [level] + np.bincount(c.level(level)[2].ravel(), minlength=5).tolist()
    r = subprocess.run([exe, frames, "67", "53", "8", "2", "4", "9", "10", "0.01", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1 and "padding" in r.stderr


# ---------------------------------------------------------------- the stereo pipeline and the CLI
def _same(got, want):
    assert got[1].tobytes() == want[1].tobytes()
    assert got[0].tobytes() == want[0].tobytes()


def test_window_with_coarse_to_fine_flow(tmp_path, capsys):
    from invcompcamtrack_amd import run_stereo_track as RS
    from invcompcamtrack_amd import stereotrack as S
    from test_gpu_stereotrack import _stereo_frames
    left, right = _stereo_frames()
    kw = dict(step=4, psz=8, lv_f=2)

    def window(**extra):
        t = S.StereoPointTracker(96, 64, 4, **kw, **extra)
        for a, b in zip(left, right):
            t.push_frames(a, b)
        return t, t.window()

    t, got = window(keep_grids=True, flow="c2f")
    assert len(t.flows) == 4 and sorted(t.flows[1]) == ["l_bwd", "l_fwd", "lr", "r_bwd", "r_fwd", "rl"]
    assert sorted(t.flows[0]) == ["lr", "rl"] and t.grids == [] and t.densifiers == [] and t.refiners == []
    want = S.stereo_track_window_host(*RS.dense_fields_of(t))
    _same(got, want)
    assert len(want[1]) > 100
    # an object's field is the stage's on that pair
    pl, pr, ql = ic.Pyramid(left[1], 2, 8, True), ic.Pyramid(right[1], 2, 8, True), ic.Pyramid(left[0], 2, 8, True)
    assert np.array_equal(_bits(pf.c2f_flow(pl, pr, 4, 8, 2)), _bits(t.flows[1]["lr"].dense()))
    assert np.array_equal(_bits(pf.c2f_flow(ql, pl, 4, 8, 2)), _bits(t.flows[1]["l_fwd"].dense()))
    _same(window(flow="c2f")[1], want)  # two sets reused in turn
    # the per-level parameters
    params = dict(densify=dict(power=2), refine=dict(n_outer=1, n_sor=2))
    tr, both = window(keep_grids=True, flow="c2f", **params)
    _same(both, S.stereo_track_window_host(*RS.dense_fields_of(tr)))
    assert np.array_equal(_bits(pf.c2f_flow(pl, pr, 4, 8, 2, **params)), _bits(tr.flows[1]["lr"].dense()))
    assert not np.array_equal(tr.flows[1]["lr"].dense(), t.flows[1]["lr"].dense())
    # flow="grid" is the path of before: no object, the grids' window
    plain_t, plain = window(keep_grids=True)
    grid_t, grid = window(keep_grids=True, flow="grid")
    _same(grid, plain)
    _same(plain, S.stereo_track_window_host(*RS.dense_fields_of(plain_t)))
    assert grid_t.flows == [] and grid_t._fsets == [None, None] and len(grid_t.grids) == 4
    for n in ("lr", "l_fwd"):
        assert np.array_equal(_bits(grid_t.grids[1][n].dense()), _bits(pf.dense_flow(*((pl, pr) if n == "lr" else (ql, pl)),
                                                                                   4, 8, 2)))
    with pytest.raises(ValueError, match="1-D form"):
        S.StereoPointTracker(96, 64, 4, flow="c2f", disparity="1d")
    with pytest.raises(ValueError, match="flow is"):
        S.StereoPointTracker(96, 64, 4, flow="dense")
    # the CLI, on the device and with --host
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        for k, (a, b) in enumerate(zip(left, right)):
            np.save(str(tmp_path / f"l{k}.npy"), a)
            np.save(str(tmp_path / f"r{k}.npy"), b)
            f.write(f"{tmp_path / f'l{k}.npy'} {tmp_path / f'r{k}.npy'}\n")
    base = [lst, str(tmp_path / "o.npz"), "--bsize", "4", "--psz", "8", "--lv_f", "2"]
    for extra in ([], ["--host"]):
        assert RS.main(base + ["--flow", "c2f"] + extra) == 0
        with np.load(base[1]) as zf:
            _same((zf["xy_t"], zf["rows"]), want)
        assert RS.main(base + ["--flow", "c2f", "--densify", "2,2", "--refine", "16,13,4.5,1,2"] + extra) == 0
        with np.load(base[1]) as zf:
            _same((zf["xy_t"], zf["rows"]), both)
        assert RS.main(base + extra) == 0
        with np.load(base[1]) as zf:
            _same((zf["xy_t"], zf["rows"]), plain)
    assert "kept" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        RS.main(base + ["--flow", "c2f", "--disparity", "1d"])
    with capsys.disabled():  # recorded, no bar
        print("survivors of", 96 * 64, "start points: grids", len(plain[1]), "coarse to fine", len(got[1]),
              "with power 2 and refinement", len(both[1]))
