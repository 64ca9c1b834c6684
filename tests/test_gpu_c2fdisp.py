"""The 1-D (x only) form of the coarse-to-fine dense flow on the device (the XONLY forms of k_c2f_level, plain and MEAN, the
refinement along x) against its f32 restatement (c2fdisp_f32.py), bit for bit and with nothing left out: per table entry,
plain and with patnorm, and per level the node displacements, the status bytes, the node bias and the level's field, and
the final field, so that every figure c2fdisp_cases.py records for the restatement against the definition is the device's
too. Then the switch (off: the bits of before), the exact properties, the C++ facade, the stereo pipeline and the CLI.

The device pyramids are built from the host pyramids' planes, so that both sides read the same bits."""
from __future__ import annotations

import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import c2fdisp_cases as XC
import c2fdisp_f32 as R
import invcompcamtrack_amd as ic
from invcompcamtrack_amd import patchflow as pf
from invcompcamtrack_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATUS8 = XC.STATUS_CASES[0]

_pyrs = {}


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):  # the host pyramids are the oracle's
    return oracle


def pyramids(case, patnorm):
    """Device pyramids holding the planes of c2fdisp_cases.pyramids_of."""
    key = (case[0], bool(patnorm), XC.pad_of(case), case[2])
    if key not in _pyrs:
        w, h = XC.frame_size(case[0])
        _pyrs[key] = tuple(ic.Pyramid(lv_f=case[2], imgpadding=XC.pad_of(case), wh=(w, h), host_planes=(o.img, o.dx, o.dy))
                           for o in XC.pyramids_of(case, patnorm))
    return _pyrs[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _flow(case, patnorm, x_only=True, **over):
    frame, psz, lv_f, maxiter, eps, _, step = case
    w, h = XC.frame_size(frame)
    kw = dict(maxiter=maxiter, eps=eps, refine=XC.refine_of(case), patnorm=patnorm, x_only=x_only)
    kw.update(over)
    return pf.CoarseToFineFlow(w, h, lv_f, step, psz, **kw)


def _same_as_restatement(c, case, patnorm):
    field, stages = XC.restated(case, patnorm)
    for level, f, d, status, bias in stages:
        gf, gd, gs = c.level(level)
        assert np.array_equal(gs, status), (case, patnorm, level, "status")
        assert np.array_equal(_bits(gd), _bits(d)), (case, patnorm, level, "d")
        if patnorm:
            assert np.array_equal(_bits(c.level_bias(level)), _bits(bias)), (case, level, "bias")
        assert np.array_equal(_bits(gf), _bits(f)), (case, patnorm, level, "field")
        assert not _bits(gf[..., 1]).any() and not _bits(gd[..., 1]).any(), (case, patnorm, level, "v is not +0.0")
    got = c.dense()
    assert np.array_equal(_bits(got), _bits(field)), (case, patnorm, "final field")
    assert not _bits(got[..., 1]).any()


# ---------------------------------------------------------------- the table, bit for bit
@pytest.mark.parametrize("patnorm", XC.MODES, ids=("plain", "patnorm"))
@pytest.mark.parametrize("case", XC.TABLE, ids=lambda c: "-".join(str(v) for v in c))
def test_table_has_the_restatements_bits(case, patnorm):
    c = _flow(case, patnorm)
    assert c.x_only
    _same_as_restatement(c.run(*pyramids(case, patnorm)), case, patnorm)


@pytest.mark.parametrize("patnorm", XC.MODES, ids=("plain", "patnorm"))
def test_same_bits_twice_and_on_a_stream(patnorm):
    from test_gpu_flowrefine import _hip_runtime
    case = XC.TABLE[2]
    pa, pb = pyramids(case, patnorm)
    c = _flow(case, patnorm).run(pa, pb)
    _same_as_restatement(c, case, patnorm)
    _same_as_restatement(c.run(pa, pb), case, patnorm)  # twice from one object
    hip, stream = _hip_runtime(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
    try:
        _same_as_restatement(c.run(pa, pb, stream=stream.value), case, patnorm)
    finally:
        assert hip.hipStreamDestroy(stream) == 0
    frame, psz, lv_f, maxiter, eps, _, step = case
    assert np.array_equal(_bits(pf.c2f_flow(pa, pb, step, psz, lv_f, maxiter=maxiter, eps=eps, patnorm=patnorm, x_only=True)),
                          _bits(XC.restated(case, patnorm)[0]))
    assert c.device_ptr()


@pytest.mark.parametrize("case", (XC.TABLE[0], XC.TABLE[2], XC.TABLE[8], XC.STRIPE_CASE), ids=lambda c: f"{c[0]}-psz{c[1]}")
def test_x_only_off_gives_the_bits_of_before(case):
    """On the same frames: the object with x_only=False, c2f_flow without the keyword and the existing restatements."""
    import c2fflow_f32 as R0
    import patnorm_f32 as RP
    frame, psz, lv_f, maxiter, eps, _, step = case
    for patnorm in XC.MODES:
        pa, pb = pyramids(case, patnorm)
        st = []
        want = (RP if patnorm else R0).run(*XC.pyramids_of(case, patnorm), step, psz, lv_f, maxiter, eps,
                                           refine=XC.refine_of(case), stages=st)
        c = _flow(case, patnorm, x_only=False).run(pa, pb)
        assert not c.x_only
        for level, f, d, status, *_ in st:
            gf, gd, gs = c.level(level)
            assert np.array_equal(gs, status) and np.array_equal(_bits(gd), _bits(d)) and np.array_equal(_bits(gf), _bits(f))
        assert np.array_equal(_bits(c.dense()), _bits(want))
        assert np.array_equal(_bits(pf.c2f_flow(pa, pb, step, psz, lv_f, maxiter=maxiter, eps=eps, patnorm=patnorm,
                                                refine=XC.refine_of(case))), _bits(want))
        assert not np.array_equal(_bits(want), _bits(XC.restated(case, patnorm)[0]))


# ---------------------------------------------------------------- exact properties, on the device
@pytest.mark.parametrize("patnorm", XC.MODES, ids=("plain", "patnorm"))
def test_maxiter_0_gives_zeros_at_every_level(patnorm):
    for case in (XC.TABLE[0], STATUS8):
        c = _flow(case, patnorm, maxiter=0).run(*pyramids(case, patnorm))
        for level in range(case[2], -1, -1):
            field, d, status = c.level(level)
            assert not _bits(field).any() and not _bits(d).any(), (case, level)
            assert np.isin(status, (pf.C2F_TRACKED, pf.C2F_HELD_COND)).all()


@pytest.mark.parametrize("patnorm", XC.MODES, ids=("plain", "patnorm"))
def test_held_nodes_keep_their_starts_bits_and_lost_ones_start_out_of_view(patnorm):
    for case in XC.STATUS_CASES:
        step, lv_f = case[6], case[2]
        c = _flow(case, patnorm).run(*pyramids(case, patnorm))
        seen = np.zeros(5, int)
        coarse = None
        for level in range(lv_f, -1, -1):
            field, d, status = c.level(level)
            h, w = field.shape[:2]
            init = R.init_of(coarse, w, h, step)
            held = status >= pf.C2F_HELD_COND
            assert np.array_equal(_bits(d[held]), _bits(init[held])), level
            sx = np.arange(step // 2, w, step, dtype=np.float32)[None, :] + init[..., 0]  # as the kernel forms it
            assert np.array_equal(status == pf.C2F_LOST, ~((sx >= 0) & (sx <= w))), level
            seen += np.bincount(status.ravel(), minlength=5)
            coarse = field
        assert tuple(seen) == XC.STATUS_COUNTS[case[1], patnorm], seen


def test_one_level_without_held_or_lost_nodes_is_the_densifier_on_the_same_nodes():
    case = next(c for c in XC.TABLE if c[0] == "farxy-320x64" and c[1] == 8)
    frame, psz, _, maxiter, eps, _, step = case
    w, h = XC.frame_size(frame)
    pa, pb = pyramids(case, False)
    c = pf.CoarseToFineFlow(w, h, 0, step, psz, maxiter=maxiter, eps=eps, x_only=True).run(pa, pb)
    field, d, status = c.level(0)
    assert (status == pf.C2F_TRACKED).all() and d[..., 0].any() and not _bits(d[..., 1]).any()
    g = pf.FlowGrid(w, h, step).set_nodes(d, np.zeros(status.shape, np.uint8))
    assert np.array_equal(_bits(pf.FlowDensifier(w, h).run(g, pa, pb, psz).dense()), _bits(field))
    assert np.array_equal(_bits(c.dense()), _bits(field))


def test_the_object_is_a_field_source_of_the_refiner():
    case = XC.TABLE[0]
    w, h = XC.frame_size(case[0])
    pa, pb = pyramids(case, False)
    c = _flow(case, False).run(pa, pb)
    r = pf.FlowRefiner(w, h, n_outer=2, n_sor=3)
    want = r.run(pa, pb, c.dense(), x_only=True).dense().copy()
    got = r.run(pa, pb, c, x_only=True).dense()
    assert np.array_equal(_bits(got), _bits(want)) and not _bits(got[..., 1]).any()


# ---------------------------------------------------------------- the C++ facade
def test_cxx_driver(tmp_path):
    """tests/cxx/c2fdisp_driver.cpp (CTR::CoarseFlowClass::SetXOnly) prints the Python call's bits."""
    exe = str(tmp_path / "c2fdisp_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "c2fdisp_driver.cpp"),
                           "-L" + os.path.join(ROOT, "invcompcamtrack_amd"), "-l:libictr_hip.so",
                           "-Wl,-rpath," + os.path.join(ROOT, "invcompcamtrack_amd")], timeout=300)
    frame, lv_f, step = "67x53", 2, 4
    for psz, maxiter, eps, patnorm in ((8, 10, 0.01, 0), (23, 3, 0.0, 1)):
        a, b = XC.pair(frame, bool(patnorm))
        frames = str(tmp_path / f"frames{patnorm}.f32")
        np.stack([a, b]).astype(np.float32).tofile(frames)
        pad = psz + 1
        r = subprocess.run([exe, frames, "67", "53", str(pad), str(lv_f), str(step), str(psz), str(maxiter), repr(eps),
                            str(patnorm)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.splitlines()
        got = np.array([[float.fromhex(t) for t in ln.split()] for ln in lines[:67 * 53]], np.float32)
        pa, pb = ic.Pyramid(a, lv_f, pad, True), ic.Pyramid(b, lv_f, pad, True)
        c = pf.CoarseToFineFlow(67, 53, lv_f, step, psz, maxiter=maxiter, eps=eps, patnorm=bool(patnorm), x_only=True).run(pa, pb)
        assert np.array_equal(_bits(got.reshape(53, 67, 2)), _bits(c.dense())), psz
        assert got[:, 0].any() and not _bits(got[:, 1]).any()
        for ln, level in zip(lines[67 * 53:], range(lv_f, -1, -1)):
            t = ln.split()
            _, d, status = c.level(level)
            assert [int(v) for v in t[1:7]] == [level] + np.bincount(status.ravel(), minlength=5).tolist()
            assert np.array_equal(_bits(np.array([float.fromhex(v) for v in t[7:]], np.float32)), _bits(d.ravel())), (psz, level)


# ---------------------------------------------------------------- the stereo pipeline and the CLI
@functools.lru_cache(maxsize=None)
def _stereo_frames(w=96, h=64, n=4):
    """A rendered plane seen by a left camera that moves a little per frame and a right camera beside it."""
    step = np.array([0.15, -0.06, 0.0, 0.0, 0.0, 0.004])  # about 1.3 px per frame at fc = 75 and depth 10
    base = np.array([0.3, -0.2, 0.5, 0.02, -0.03, 0.01])
    right = np.array([-0.55, 0.0, 0.0, 0.0, 0.0, 0.0])  # about 4 px of disparity
    poses = [base + k * step for k in range(n)] + [base + k * step + right for k in range(n)]
    fr = synth.make_sequence(w, h, poses, 0, 10, seed=4)["frames"]
    return fr[:n], fr[n:]


def _same(got, want):
    assert got[1].tobytes() == want[1].tobytes()
    assert got[0].tobytes() == want[0].tobytes()


@pytest.mark.parametrize("patnorm", XC.MODES, ids=("plain", "patnorm"))
def test_window_with_the_1d_stereo_pair(tmp_path, capsys, patnorm):
    from invcompcamtrack_amd import run_stereo_track as RS
    from invcompcamtrack_amd import stereotrack as S
    left, right = _stereo_frames()
    if patnorm:
        right = [np.ascontiguousarray(r + np.float32(20)) for r in right]
    kw = dict(step=4, psz=8, lv_f=2, patnorm=patnorm)

    def window(**extra):
        t = S.StereoPointTracker(96, 64, 4, **kw, **extra)
        for a, b in zip(left, right):
            t.push_frames(a, b)
        return t, t.window()

    t, got = window(keep_grids=True, flow="c2f-1d", disparity="2d")
    assert len(t.flows) == 4 and sorted(t.flows[1]) == ["l_bwd", "l_fwd", "lr", "r_bwd", "r_fwd", "rl"]
    assert sorted(t.flows[0]) == ["lr", "rl"] and t.grids == [] and t.densifiers == [] and t.refiners == []
    assert all(f[n].x_only == (n in ("lr", "rl")) and f[n].patnorm == patnorm for f in t.flows for n in f)
    want = S.stereo_track_window_host(*RS.dense_fields_of(t))
    _same(got, want)
    assert len(want[1]) > 100
    # an object's field is the stage's on that pair: the stereo pair 1-D, the temporal fields 2-D
    pl, pr, ql = ic.Pyramid(left[1], 2, 8, True), ic.Pyramid(right[1], 2, 8, True), ic.Pyramid(left[0], 2, 8, True)
    lr = t.flows[1]["lr"].dense()
    assert np.array_equal(_bits(pf.c2f_flow(pl, pr, 4, 8, 2, patnorm=patnorm, x_only=True)), _bits(lr))
    assert not _bits(lr[..., 1]).any() and not _bits(t.flows[1]["rl"].dense()[..., 1]).any()
    assert np.array_equal(_bits(pf.c2f_flow(ql, pl, 4, 8, 2, patnorm=patnorm)), _bits(t.flows[1]["l_fwd"].dense()))
    _same(window(flow="c2f-1d")[1], want)  # two sets reused in turn
    _same(window(flow="c2f-1d", disparity="1d")[1], want)  # disparity is not consulted
    params = dict(densify=dict(power=2), refine=dict(n_outer=1, n_sor=2))
    tr, both = window(keep_grids=True, flow="c2f-1d", **params)
    _same(both, S.stereo_track_window_host(*RS.dense_fields_of(tr)))
    assert np.array_equal(_bits(pf.c2f_flow(pl, pr, 4, 8, 2, patnorm=patnorm, x_only=True, **params)),
                          _bits(tr.flows[1]["lr"].dense()))
    two_d = window(flow="c2f")[1]
    # the CLI, on the device and with --host
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        for k, (a, b) in enumerate(zip(left, right)):
            np.save(str(tmp_path / f"l{k}.npy"), a)
            np.save(str(tmp_path / f"r{k}.npy"), b)
            f.write(f"{tmp_path / f'l{k}.npy'} {tmp_path / f'r{k}.npy'}\n")
    base = [lst, str(tmp_path / "o.npz"), "--bsize", "4", "--psz", "8", "--lv_f", "2"] + (["--patnorm"] if patnorm else [])
    for extra in ([], ["--host"]):
        assert RS.main(base + ["--flow", "c2f-1d"] + extra) == 0
        with np.load(base[1]) as zf:
            _same((zf["xy_t"], zf["rows"]), want)
        assert RS.main(base + ["--flow", "c2f-1d", "--densify", "2,2", "--refine", "16,13,4.5,1,2"] + extra) == 0
        with np.load(base[1]) as zf:
            _same((zf["xy_t"], zf["rows"]), both)
    assert "kept" in capsys.readouterr().out
    with capsys.disabled():  # recorded, no bar
        print("survivors of", 96 * 64, "start points" + (" with the right frames + 20 and patnorm" if patnorm else "") + ":",
              "flow='c2f'", len(two_d[1]), "flow='c2f-1d'", len(got[1]))
