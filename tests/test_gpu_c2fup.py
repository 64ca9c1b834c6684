"""A finest level above 0 of the coarse-to-fine dense flow on the device (CoarseToFineFlow(lv_l=...), k_flow_upsample)
against its f32 restatement (c2fup_f32.py), bit for bit and with nothing left out: the stand-alone kernel on seeded fields
of every shape of c2fup_cases.SHAPES, the stage per level and of the result, then the surface (refusals, timing, the
refiner, the stereo pipeline, the CLI and the C++ facade).

The device pyramids are built from the host pyramids' planes, so that both sides read the same bits."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import c2fflow_cases as CC
import c2fup_cases as UC
import c2fup_f32 as R
import invcompcamtrack_amd as ic
from invcompcamtrack_amd import _lib
from invcompcamtrack_amd import patchflow as pf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = 1   # ICTR_ERR_INVALID of include/ictr.h

_pyrs = {}


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):  # the host pyramids are the oracle's
    return oracle


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pyramids(case, patnorm):
    """Device pyramids holding the planes of c2fup_cases.host_pyramids."""
    key = (case[0], CC.pad_of(case), case[2], bool(patnorm))
    if key not in _pyrs:
        w, h = CC.frame_size(case[0])
        _pyrs[key] = tuple(ic.Pyramid(lv_f=case[2], imgpadding=CC.pad_of(case), wh=(w, h), host_planes=(o.img, o.dx, o.dy))
                           for o in UC.host_pyramids(case, patnorm))
    return _pyrs[key]


def _flow(case, lv_l, patnorm=False, x_only=False, **over):
    frame, psz, lv_f, maxiter, eps, _, step = case
    w, h = CC.frame_size(frame)
    kw = dict(maxiter=maxiter, eps=eps, refine=CC.refine_of(case), patnorm=patnorm, x_only=x_only, lv_l=lv_l)
    kw.update(over)
    return pf.CoarseToFineFlow(w, h, lv_f, step, psz, **kw)


# ---------------------------------------------------------------- the stand-alone kernel
@pytest.mark.parametrize("x_only", (False, True), ids=("2d", "x_only"))
@pytest.mark.parametrize("shape", UC.SHAPES, ids=lambda s: "%dx%d-lv%d" % s)
def test_kernel_has_the_restatements_bits(shape, x_only):
    w, h, lv = shape
    f = UC.field(w, h, lv)
    assert f.min() < 0 < f.max()
    got = pf.upsample_flow(f, w, h, lv, x_only)
    assert np.array_equal(_bits(got), _bits(UC.restated(w, h, lv, x_only))), shape
    if x_only:
        assert not _bits(got[..., 1]).any()


def test_the_exact_properties_hold_on_the_device():
    """test_c2fup_cpu.py's constant field and ramp, and x_only on a field whose v is NaN."""
    for w, h, lv in UC.SHAPES[:8]:
        wl, hl = UC.level_size(w, h, lv)
        s = float(1 << lv)
        f = np.empty((hl, wl, 2), np.float32)
        f[...] = (1.5, -0.75)
        want = np.empty((h, w, 2), np.float32)
        want[...] = (1.5 * s, -0.75 * s)
        assert np.array_equal(_bits(pf.upsample_flow(f, w, h, lv)), _bits(want)), (w, h, lv)
        f[..., 0] = np.arange(wl)[None, :] / 4.0
        f[..., 1] = np.arange(hl)[:, None] / 4.0
        want[..., 0] = (s * np.clip((np.arange(w) + 0.5) / s - 0.5, 0.0, wl - 1.0) / 4)[None, :]
        want[..., 1] = (s * np.clip((np.arange(h) + 0.5) / s - 0.5, 0.0, hl - 1.0) / 4)[:, None]
        assert np.array_equal(_bits(pf.upsample_flow(f, w, h, lv)), _bits(want)), (w, h, lv)
        f[..., 1] = np.nan
        got = pf.upsample_flow(f, w, h, lv, True)
        assert not _bits(got[..., 1]).any() and np.array_equal(_bits(got[..., 0]), _bits(want[..., 0]))


def test_device_pointers_on_a_callers_stream_and_the_refusals():
    from test_gpu_flowrefine import _hip_runtime
    w, h, lv = 67, 53, 2
    f = UC.field(w, h, lv)
    wl, hl = UC.level_size(w, h, lv)
    hip, L = _hip_runtime(), _lib.load()
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    src, dst, stream = C.c_void_p(), C.c_void_p(), C.c_void_p()
    out = np.zeros((h, w, 2), np.float32)
    assert hip.hipMalloc(C.byref(src), f.nbytes) == 0 and hip.hipMalloc(C.byref(dst), out.nbytes) == 0
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
    try:
        assert hip.hipMemcpy(src, f.ctypes.data_as(C.c_void_p), f.nbytes, 1) == 0  # hipMemcpyHostToDevice
        pf.check(L.ictr_flow_upsample(src, wl, hl, lv, dst, w, h, 0, 1, stream))
        assert hip.hipStreamSynchronize(stream) == 0
        assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), dst, out.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        assert np.array_equal(_bits(out), _bits(UC.restated(w, h, lv, False)))
        assert UC.level_size(w - 1, h, lv) != (wl, hl)  # 66 -> 33 -> 16: a smaller frame that the field does not fit
        assert L.ictr_flow_upsample(src, wl, hl, lv, dst, w - 1, h, 0, 1, stream) == ERR_INVALID
        assert L.ictr_flow_upsample(src, wl, hl, 0, dst, w, h, 0, 1, stream) == ERR_INVALID
        assert L.ictr_flow_upsample(None, wl, hl, lv, dst, w, h, 0, 1, stream) == ERR_INVALID
    finally:
        assert hip.hipStreamDestroy(stream) == 0
        assert hip.hipFree(src) == 0 and hip.hipFree(dst) == 0


# ---------------------------------------------------------------- the stage
def _same_as_restatement(c, case, lv_l, patnorm, x_only):
    want, stages = UC.restated_run(case, lv_l, patnorm, x_only)
    assert [s[0] for s in stages] == list(range(case[2], lv_l - 1, -1))
    for level, f, d, status, *bias in stages:
        gf, gd, gs = c.level(level)
        assert np.array_equal(gs, status), (case, lv_l, level, "status")
        assert np.array_equal(_bits(gd), _bits(d)), (case, lv_l, level, "d")
        assert np.array_equal(_bits(gf), _bits(f)), (case, lv_l, level, "field")
        if patnorm:
            assert np.array_equal(_bits(c.level_bias(level)), _bits(bias[0])), (case, level, "bias")
    got = c.dense()
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), (case, lv_l, "result")
    if x_only:
        assert got[..., 0].any() and not _bits(got[..., 1]).any()


@pytest.mark.parametrize("entry", UC.STAGE_CASES,
                         ids=lambda e: "-".join(str(v) for v in e[0]) + f"-lvl{e[1]}" + ("-patnorm" if e[2] else "")
                         + ("-x_only" if e[3] else ""))
def test_stage_has_the_restatements_bits(entry):
    case, lv_l, patnorm, x_only = entry
    c = _flow(case, lv_l, patnorm, x_only)
    assert c.lv_l == lv_l
    _same_as_restatement(c.run(*pyramids(case, patnorm)), case, lv_l, patnorm, x_only)


def test_same_bits_twice_on_a_stream_and_from_the_one_call_form():
    from test_gpu_flowrefine import _hip_runtime
    case, lv_l, patnorm, x_only = UC.STAGE_CASES[0]
    pa, pb = pyramids(case, patnorm)
    c = _flow(case, lv_l).run(pa, pb)
    _same_as_restatement(c, case, lv_l, patnorm, x_only)
    _same_as_restatement(c.run(pa, pb), case, lv_l, patnorm, x_only)  # twice from one object
    hip, stream = _hip_runtime(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
    try:
        _same_as_restatement(c.run(pa, pb, stream=stream.value), case, lv_l, patnorm, x_only)
    finally:
        assert hip.hipStreamDestroy(stream) == 0
    frame, psz, lv_f, maxiter, eps, _, step = case
    assert np.array_equal(_bits(pf.c2f_flow(pa, pb, step, psz, lv_f, maxiter=maxiter, eps=eps, lv_l=lv_l)),
                          _bits(UC.restated_run(case, lv_l, patnorm, x_only)[0]))
    assert c.device_ptr()


def test_lv_l_0_through_create_lvl_has_the_bits_of_create():
    case = UC.STAGE_CASES[0][0]
    frame, psz, lv_f, maxiter, eps, _, step = case
    w, h = CC.frame_size(frame)
    pa, pb = pyramids(case, False)
    want = _flow(case, 0).run(pa, pb)
    assert np.array_equal(_bits(want.dense()), _bits(CC.restated(case)[0]))
    L, hnd, lv_l = _lib.load(), C.c_void_p(), C.c_int(-1)
    assert want.lv_l == 0  # the Python object goes through create_lvl; the handle below through create
    pf.check(L.ictr_c2fflow_create(C.byref(hnd), w, h, lv_f, step, psz))
    try:
        pf.check(L.ictr_c2fflow_get_lv_l(hnd, C.byref(lv_l)))
        assert lv_l.value == 0
        pf.check(L.ictr_c2fflow_set_params(hnd, maxiter, eps, 2.0, 1))
        pf.check(L.ictr_c2fflow_run(hnd, pa._h, pb._h, None))
        got = np.empty((h, w, 2), np.float32)
        pf.check(L.ictr_c2fflow_result(hnd, got.ctypes.data_as(C.c_void_p), 0))
        assert np.array_equal(_bits(got), _bits(want.dense()))
        f0, f1 = np.empty((h, w, 2), np.float32), want.level(0)[0]
        pf.check(L.ictr_c2fflow_read_level(hnd, 0, pf.fp(f0), None, None))
        assert np.array_equal(_bits(f0), _bits(f1))
        ms = C.c_float(-1)
        pf.check(L.ictr_c2fflow_get_upsample_ms(hnd, C.byref(ms)))
        assert ms.value == 0.0
    finally:
        L.ictr_c2fflow_destroy(hnd)
    for bad in (-1, lv_f + 1):
        assert L.ictr_c2fflow_create_lvl(C.byref(hnd), w, h, lv_f, bad, step, psz) == ERR_INVALID
        assert b"lv_l" in L.ictr_last_error()


# ---------------------------------------------------------------- the surface
def test_levels_below_lv_l_are_refused_and_the_timing_rows():
    case = UC.STAGE_CASES[0][0]
    pa, pb = pyramids(case, False)
    c = _flow(case, 1)
    c.set_timing(True)
    c.run(pa, pb)
    for call in (c.level, c.level_dims):
        with pytest.raises(_lib.IctrError, match=r"level is 0 \(1 \.\. 2\)"):
            call(0)
    assert c.level_dims(1)[:2] == UC.level_size(*CC.frame_size(case[0]), 1)
    ms = c.kernel_ms()
    assert ms.shape == (3, 3) and not ms[0].any() and (ms[1:, :2] > 0).all()
    assert c.upsample_ms() > 0
    c.set_timing(False)
    assert c.run(pa, pb).upsample_ms() == 0 and not c.kernel_ms().any()
    cp = _flow(case, 1, patnorm=True).run(*pyramids(case, True))
    with pytest.raises(_lib.IctrError, match=r"level is 0 \(1 \.\. 2\)"):
        cp.level_bias(0)


def test_the_object_is_a_field_source_of_the_refiner():
    """FlowRefiner.run(src=c2f) on an lv_l = 1 object: the refinement restatement on the restated up-sampled field."""
    import flowrefine_f32 as FR
    case, lv_l = UC.STAGE_CASES[0][0], 1
    w, h = CC.frame_size(case[0])
    pa, pb = pyramids(case, False)
    c = _flow(case, lv_l).run(pa, pb)
    r = pf.FlowRefiner(w, h, **CC.REFINE)
    got = r.run(pa, pb, c).dense()
    ha, hb = UC.host_pyramids(case, False)
    import c2fflow_f32 as R0
    want = FR.refine(R0.plane(ha, 0), R0.plane(hb, 0), UC.restated_run(case, lv_l, False, False)[0], **CC.REFINE)
    assert np.array_equal(_bits(got), _bits(want))


def _host_view(p, lv_f):
    """A device pyramid's planes as the restatements read a host pyramid."""
    return types.SimpleNamespace(img=[p.download(l, 0) for l in range(lv_f + 1)], dx=[p.download(l, 1) for l in range(lv_f + 1)],
                                 dy=[p.download(l, 2) for l in range(lv_f + 1)], pad=p.pad)


def test_window_with_lv_l_1_and_the_cli(tmp_path, capsys):
    """StereoPointTracker(flow="c2f", lv_l=1) on test_gpu_c2fdisp's small sequence: every object has lv_l = 1, and the
    window is the host path's on the restated fields (restated on the planes of device pyramids of the same frames)."""
    from invcompcamtrack_amd import run_stereo_track as RS
    from invcompcamtrack_amd import stereotrack as S
    from test_gpu_c2fdisp import _stereo_frames
    left, right = _stereo_frames()
    psz, lv_f, step = 8, 2, 4
    t = S.StereoPointTracker(96, 64, 4, step=step, psz=psz, lv_f=lv_f, flow="c2f", lv_l=1, keep_grids=True)
    for a, b in zip(left, right):
        t.push_frames(a, b)
    got = t.window()
    assert t.lv_l == 1 and all(f[n].lv_l == 1 for f in t.flows for n in f)
    hl = [_host_view(ic.Pyramid(a, lv_f, psz, True), lv_f) for a in left]
    hr = [_host_view(ic.Pyramid(b, lv_f, psz, True), lv_f) for b in right]
    assert hl[0].pad == psz

    def restated(a, b):
        return R.run(a, b, step, psz, lv_f, 1)

    lr = [-restated(a, b)[:, :, 0] for a, b in zip(hl, hr)]
    rl = [np.ascontiguousarray(restated(b, a)[:, :, 0]) for a, b in zip(hl, hr)]
    fl = [(restated(hl[k - 1], hl[k]), restated(hl[k], hl[k - 1])) for k in range(1, 4)]
    fr = [(restated(hr[k - 1], hr[k]), restated(hr[k], hr[k - 1])) for k in range(1, 4)]
    assert np.array_equal(_bits(t.flows[1]["l_fwd"].dense()), _bits(fl[0][0]))
    want = S.stereo_track_window_host(lr, rl, fl, fr)
    assert got[1].tobytes() == want[1].tobytes() and got[0].tobytes() == want[0].tobytes()
    assert len(want[1]) > 100
    with pytest.raises(ValueError, match="lv_l > 0 needs flow"):
        S.StereoPointTracker(96, 64, 4, flow="grid", lv_l=1)
    # the CLI, on the device and with --host
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        for k, (a, b) in enumerate(zip(left, right)):
            np.save(str(tmp_path / f"l{k}.npy"), a)
            np.save(str(tmp_path / f"r{k}.npy"), b)
            f.write(f"{tmp_path / f'l{k}.npy'} {tmp_path / f'r{k}.npy'}\n")
    base = [lst, str(tmp_path / "o.npz"), "--bsize", "4", "--psz", "8", "--lv_f", "2", "--flow", "c2f", "--lv-l", "1"]
    for extra in ([], ["--host"]):
        assert RS.main(base + extra) == 0
        with np.load(base[1]) as zf:
            assert zf["rows"].tobytes() == want[1].tobytes() and zf["xy_t"].tobytes() == want[0].tobytes()
    assert "kept" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        RS.main([lst, base[1], "--flow", "grid", "--lv-l", "1"])


def test_cxx_driver(tmp_path):
    """tests/cxx/c2fup_driver.cpp (CTR::CoarseFlowClass with lv_l, LvL, CTR::UpsampleFlow) prints the Python call's bits."""
    exe = str(tmp_path / "c2fup_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "c2fup_driver.cpp"),
                           "-L" + os.path.join(ROOT, "invcompcamtrack_amd"), "-l:libictr_hip.so",
                           "-Wl,-rpath," + os.path.join(ROOT, "invcompcamtrack_amd")], timeout=300)
    frame, lv_f, step, psz, maxiter, eps, pad = "67x53", 2, 4, 8, 10, 0.01, 9
    a, b = CC.pair(frame)
    frames = str(tmp_path / "frames.f32")
    np.stack([a, b]).astype(np.float32).tofile(frames)
    pa, pb = ic.Pyramid(a, lv_f, pad, True), ic.Pyramid(b, lv_f, pad, True)
    for lv_l in (1, 2):
        r = subprocess.run([exe, frames, "67", "53", str(pad), str(lv_f), str(lv_l), str(step), str(psz), str(maxiter),
                            repr(eps)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.splitlines()
        n = 67 * 53
        assert len(lines) == 2 * n + 1
        c = pf.CoarseToFineFlow(67, 53, lv_f, step, psz, maxiter=maxiter, eps=eps, lv_l=lv_l).run(pa, pb)
        for part in (lines[:n], lines[n + 1:]):
            got = np.array([[float.fromhex(t) for t in ln.split()] for ln in part], np.float32)
            assert np.array_equal(_bits(got.reshape(53, 67, 2)), _bits(c.dense())), lv_l
        assert lines[n].split() == ["level", str(lv_l)] + [str(v) for v in UC.level_size(67, 53, lv_l)]
