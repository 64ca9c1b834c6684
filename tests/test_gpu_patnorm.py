"""Patch-mean normalisation of the coarse-to-fine dense flow on the device (the MEAN forms of k_c2f_level with their bias
tail, k_densify<true, 1>) against its f32 restatement (patnorm_f32.py), bit for bit and with nothing left out: per table entry
and per level the node displacements, the status bytes, the node bias and the level's field, and the final field, so that
every figure patnorm_cases.py records for the restatement against the definition is the device's too. Then the switch
(off: today's bits), the stereo pipeline, the CLI, the C++ facade and the refusals.

The device pyramids are built from the host pyramids' planes, so that both sides read the same bits."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import c2fflow_cases as CC
import invcompcamtrack_amd as ic
import patnorm_cases as PN
from invcompcamtrack_amd import patchflow as pf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_pyrs = {}


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):  # the host pyramids are the oracle's
    return oracle


def pyramids(case):
    """Device pyramids holding the planes of patnorm_cases.pyramids_of."""
    key = (case[0], case[7], PN.pad_of(case), case[2])
    if key not in _pyrs:
        w, h = CC.frame_size(case[0])
        _pyrs[key] = tuple(ic.Pyramid(lv_f=case[2], imgpadding=PN.pad_of(case), wh=(w, h), host_planes=(o.img, o.dx, o.dy))
                           for o in PN.pyramids_of(case))
    return _pyrs[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _flow(case, patnorm=True):
    frame, psz, lv_f, maxiter, eps, _, step, _ = case
    w, h = CC.frame_size(frame)
    return pf.CoarseToFineFlow(w, h, lv_f, step, psz, maxiter=maxiter, eps=eps, refine=PN.refine_of(case), patnorm=patnorm)


def _same_as_restatement(c, case):
    field, stages = PN.restated(case)
    for level, f, d, status, bias in stages:
        gf, gd, gs = c.level(level)
        gb = c.level_bias(level)
        assert np.array_equal(gs, status), (case, level, "status")
        assert np.array_equal(_bits(gd), _bits(d)), (case, level, "d")
        assert np.array_equal(_bits(gb), _bits(bias)), (case, level, "bias")
        assert np.array_equal(_bits(gf), _bits(f)), (case, level, "field")
    assert np.array_equal(_bits(c.dense()), _bits(field)), (case, "final field")


# ---------------------------------------------------------------- the table, bit for bit
@pytest.mark.parametrize("case", PN.TABLE, ids=lambda c: "-".join(str(v) for v in c))
def test_table_has_the_restatements_bits(case):
    _same_as_restatement(_flow(case).run(*pyramids(case)), case)


def test_same_bits_twice_and_on_a_stream():
    from test_gpu_flowrefine import _hip_runtime
    case = PN.TABLE[1]
    pa, pb = pyramids(case)
    c = _flow(case).run(pa, pb)
    _same_as_restatement(c, case)
    _same_as_restatement(c.run(pa, pb), case)  # twice from one object
    hip, stream = _hip_runtime(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
    try:
        _same_as_restatement(c.run(pa, pb, stream=stream.value), case)
    finally:
        assert hip.hipStreamDestroy(stream) == 0
    frame, psz, lv_f, maxiter, eps, _, step, _ = case
    assert np.array_equal(_bits(pf.c2f_flow(pa, pb, step, psz, lv_f, maxiter=maxiter, eps=eps, patnorm=True)),
                          _bits(PN.restated(case)[0]))


@pytest.mark.parametrize("case", (PN.TABLE[0], PN.TABLE[1], PN.TABLE[3]), ids=lambda c: f"psz{c[1]}")
def test_patnorm_off_gives_the_bits_of_before(case):
    """On the changed frames: the object with patnorm=False, c2f_flow without the keyword and the plain restatement."""
    import c2fflow_f32 as R0
    frame, psz, lv_f, maxiter, eps, _, step, _ = case
    pa, pb = pyramids(case)
    st = []
    want = R0.run(*PN.pyramids_of(case), step, psz, lv_f, maxiter, eps, refine=PN.refine_of(case), stages=st)
    c = _flow(case, patnorm=False).run(pa, pb)
    for level, f, d, status in st:
        gf, gd, gs = c.level(level)
        assert np.array_equal(gs, status) and np.array_equal(_bits(gd), _bits(d)) and np.array_equal(_bits(gf), _bits(f))
    assert np.array_equal(_bits(c.dense()), _bits(want))
    assert np.array_equal(_bits(pf.c2f_flow(pa, pb, step, psz, lv_f, maxiter=maxiter, eps=eps, refine=PN.refine_of(case))),
                          _bits(want))
    assert not np.array_equal(_bits(want), _bits(PN.restated(case)[0]))
    with pytest.raises(ic.IctrError, match="patnorm off"):
        c.level_bias(0)


# ---------------------------------------------------------------- the C++ facade
def test_cxx_driver(tmp_path):
    """tests/cxx/patnorm_driver.cpp (CTR::CoarseFlowClass::SetPatnorm, ReadLevelBias) prints the Python call's bits."""
    exe = str(tmp_path / "patnorm_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "patnorm_driver.cpp"),
                           "-L" + os.path.join(ROOT, "invcompcamtrack_amd"), "-l:libictr_hip.so",
                           "-Wl,-rpath," + os.path.join(ROOT, "invcompcamtrack_amd")], timeout=300)
    frame, lv_f, step = "67x53", 2, 4
    a, b = CC.pair(frame)
    b = PN.changed(b, "+20")
    frames = str(tmp_path / "frames.f32")
    np.stack([a, b]).astype(np.float32).tofile(frames)
    for psz, maxiter, eps in ((8, 10, 0.01), (23, 3, 0.0)):
        pad = psz + 1
        r = subprocess.run([exe, frames, "67", "53", str(pad), str(lv_f), str(step), str(psz), str(maxiter), repr(eps)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.splitlines()
        got = np.array([[float.fromhex(t) for t in ln.split()] for ln in lines[:67 * 53]], np.float32)
        pa, pb = ic.Pyramid(a, lv_f, pad, True), ic.Pyramid(b, lv_f, pad, True)
        c = pf.CoarseToFineFlow(67, 53, lv_f, step, psz, maxiter=maxiter, eps=eps, patnorm=True).run(pa, pb)
        assert np.array_equal(_bits(got.reshape(53, 67, 2)), _bits(c.dense())), psz
        for ln, level in zip(lines[67 * 53:], range(lv_f, -1, -1)):
            t = ln.split()
            assert [int(v) for v in t[1:7]] == [level] + np.bincount(c.level(level)[2].ravel(), minlength=5).tolist()
            bias = np.array([float.fromhex(v) for v in t[7:]], np.float32)
            assert np.array_equal(_bits(bias), _bits(c.level_bias(level).ravel())), (psz, level)
            assert bias.any()


# ---------------------------------------------------------------- the stereo pipeline and the CLI
def _same(got, want):
    assert got[1].tobytes() == want[1].tobytes()
    assert got[0].tobytes() == want[0].tobytes()


def test_window_with_patnorm_on_a_brighter_right_camera(tmp_path, capsys):
    from invcompcamtrack_amd import run_stereo_track as RS
    from invcompcamtrack_amd import stereotrack as S
    from test_gpu_stereotrack import _stereo_frames
    left, right = _stereo_frames()
    right = [np.ascontiguousarray(r + np.float32(20)) for r in right]
    kw = dict(step=4, psz=8, lv_f=2)

    def window(**extra):
        t = S.StereoPointTracker(96, 64, 4, **kw, **extra)
        for a, b in zip(left, right):
            t.push_frames(a, b)
        return t, t.window()

    t, got = window(keep_grids=True, flow="c2f", patnorm=True)
    want = S.stereo_track_window_host(*RS.dense_fields_of(t))
    _same(got, want)
    pl, pr = ic.Pyramid(left[1], 2, 8, True), ic.Pyramid(right[1], 2, 8, True)
    assert np.array_equal(_bits(pf.c2f_flow(pl, pr, 4, 8, 2, patnorm=True)), _bits(t.flows[1]["lr"].dense()))
    assert t.flows[1]["lr"].level_bias(0).any()
    _same(window(flow="c2f", patnorm=True)[1], want)  # two sets reused in turn
    plain = window(flow="c2f")[1]
    with pytest.raises(ValueError, match="patnorm=True needs flow='c2f'"):
        S.StereoPointTracker(96, 64, 4, flow="grid", patnorm=True)
    # the CLI, on the device and with --host
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        for k, (a, b) in enumerate(zip(left, right)):
            np.save(str(tmp_path / f"l{k}.npy"), a)
            np.save(str(tmp_path / f"r{k}.npy"), b)
            f.write(f"{tmp_path / f'l{k}.npy'} {tmp_path / f'r{k}.npy'}\n")
    base = [lst, str(tmp_path / "o.npz"), "--bsize", "4", "--psz", "8", "--lv_f", "2"]
    for extra in ([], ["--host"]):
        assert RS.main(base + ["--flow", "c2f", "--patnorm"] + extra) == 0
        with np.load(base[1]) as zf:
            _same((zf["xy_t"], zf["rows"]), want)
    assert "kept" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        RS.main(base + ["--patnorm"])
    with capsys.disabled():  # recorded, no bar
        print("survivors of", 96 * 64, "start points with the right frames + 20: plain coarse to fine", len(plain[1]),
              "with patnorm", len(got[1]))
