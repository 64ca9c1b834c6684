"""The Huber patch cost of the coarse-to-fine dense flow on the device (the ROBUST forms of k_c2f_level,
csrc/ictr_c2fflow_robust.hip) against its f32 restatement (c2fcost_f32.py), bit for bit and with nothing left out: per table
entry and per level the node displacements, the status bytes, the node bias and the level's field, and the final field, so
that every figure c2fcost_cases.py records for the restatement against the definition
(patchflow.c2f_flow_host(cost="huber")) is the device's too. Then the cost switched off, a clip that never binds, the C++
facade, the stereo pipeline with its command-line tool, and the refusals.

The device pyramids are built from the host pyramids' planes, so that both sides read the same bits."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import c2fcost_cases as K
import invcompcamtrack_amd as ic
from invcompcamtrack_amd import _lib
from invcompcamtrack_amd import patchflow as pf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_pyrs = {}


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):  # the host pyramids are the oracle's
    return oracle


def pyramids(case):
    """Device pyramids holding the planes of c2fcost_cases.pyramids_of: (A, B), lists of three on colour frames."""
    key = (case[0], K.pad_of(case), case[2], case[8], case[7])
    if key not in _pyrs:
        w, h = K.frame_size(case[0])
        dev = lambda o: ic.Pyramid(lv_f=case[2], imgpadding=K.pad_of(case), wh=(w, h), host_planes=(o.img, o.dx, o.dy))
        _pyrs[key] = tuple(dev(side) if case[8] == 1 else [dev(o) for o in side] for side in K.pyramids_of(case))
    return _pyrs[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _flow(case, **over):
    frame, psz, lv_f, maxiter, eps, step, x_only, patnorm, channels, k, _ = case
    w, h = K.frame_size(frame)
    kw = dict(maxiter=maxiter, eps=eps, patnorm=patnorm, x_only=x_only, lv_l=K.lv_l_of(case), refine=K.refine_of(case),
              channels=channels, cost="huber", huber_k=k)
    kw.update(over)
    return pf.CoarseToFineFlow(w, h, lv_f, step, psz, **kw)


def _same_as_restatement(c, case, want=None):
    field, stages = want or K.restated(case)
    assert len(stages) == case[2] - K.lv_l_of(case) + 1
    for level, f, d, status, bias in stages:
        gf, gd, gs = c.level(level)
        assert np.array_equal(gs, status), (case, level, "status")
        assert np.array_equal(_bits(gd), _bits(d)), (case, level, "d")
        if case[7]:
            gb = c.level_bias(level)
            assert gb.shape == bias.shape and np.array_equal(_bits(gb), _bits(bias)), (case, level, "bias")
        assert np.array_equal(_bits(gf), _bits(f)), (case, level, "field")
    assert np.array_equal(_bits(c.dense()), _bits(field)), (case, "final field")


# ---------------------------------------------------------------- the table, bit for bit
@pytest.mark.parametrize("case", K.TABLE, ids=K.case_id)
def test_table_has_the_restatements_bits(case):
    c = _flow(case)
    assert c.cost == "huber" and c.huber_k == case[9]
    _same_as_restatement(c.run(*pyramids(case)), case)


def test_same_bits_twice_and_on_a_stream():
    from test_gpu_flowrefine import _hip_runtime
    for case in (K.TABLE[9], K.TABLE[17]):  # <8,2> with patnorm, grey and colour: the two-pass iteration's barriers
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
    frame, psz, lv_f, maxiter, eps, step, x_only, patnorm, _, k, _ = case
    got = pf.c2f_flow(pa, pb, step, psz, lv_f, maxiter=maxiter, eps=eps, patnorm=patnorm, cost="huber", huber_k=k)
    assert np.array_equal(_bits(got), _bits(K.restated(case)[0]))


# ---------------------------------------------------------------- the cost switched off, and a clip that never binds
def test_cost_l2_has_the_l2_restatements_bits_on_the_salted_frames():
    """cost="l2", spelled out or left out, on the salted frames: the bits of c2fflow_f32 / patnorm_f32 / c2fdisp_f32 /
    c2frgb_f32, which differ from the Huber bits; and an object switched from Huber back to L2 has them too."""
    for case in (K.TABLE[0], K.TABLE[1], K.TABLE[2], K.TABLE[10], K.TABLE[13], K.TABLE[22]):
        pa, pb = pyramids(case)
        want = K.restated_l2(case)
        for over in (dict(cost="l2"), dict(cost="l2", huber_k=0.5)):
            assert np.array_equal(_bits(_flow(case, **over).run(pa, pb).dense()), _bits(want)), (case, over)
        c = _flow(case)
        huber = c.run(pa, pb).dense()
        assert not np.array_equal(_bits(huber), _bits(want)), case
        c.set_cost("l2")
        assert c.cost == "l2" and np.array_equal(_bits(c.run(pa, pb).dense()), _bits(want)), case
        c.set_cost("huber", case[9])
        assert np.array_equal(_bits(c.run(pa, pb).dense()), _bits(huber)), case


def test_a_huge_k_is_the_l2_cost():
    """huber_k = 1e30 on the entries with eps = 0. Without patnorm the ROBUST forms give the L2 forms' bits exactly, per
    level and in the final field. With patnorm the direct form rounds differently from b = s + mean(I) sum G; the worst
    difference is measured against c2fcost_cases.IDENTITY_PATNORM_DIFF, above which or below half of which it fails."""
    worst = 0.0
    for case in K.TABLE:
        if case[4] != 0.0:
            continue
        pa, pb = pyramids(case)
        huge, l2 = _flow(case, huber_k=K.IDENTITY_K).run(pa, pb), _flow(case, cost="l2").run(pa, pb)
        if case[7]:
            gap = float(np.abs(huge.dense().astype(np.float64) - l2.dense()).max())
            print(K.case_id(case), f"|direct form - L2 patnorm form| {gap:.3e} px")
            worst = max(worst, gap)
        else:
            for level in range(case[2], -1, -1):
                assert all(x.tobytes() == y.tobytes() for x, y in zip(huge.level(level), l2.level(level))), (case, level)
            assert huge.dense().tobytes() == l2.dense().tobytes(), case
    print(f"patnorm at k = 1e30 against the L2 patnorm forms: {worst:.3e}, record {K.IDENTITY_PATNORM_DIFF:.3e}")
    assert 0.5 * K.IDENTITY_PATNORM_DIFF <= worst <= K.IDENTITY_PATNORM_DIFF


# ---------------------------------------------------------------- the C++ facade
def test_cxx_driver(tmp_path):
    """tests/cxx/c2fcost_driver.cpp (CTR::CoarseFlowClass::SetCost / GetCost of include/ctr_shim.hpp) checks the facade's
    refusals and prints the Python call's bits."""
    exe = str(tmp_path / "c2fcost_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "c2fcost_driver.cpp"),
                           "-L" + os.path.join(ROOT, "invcompcamtrack_amd"), "-l:libictr_hip.so",
                           "-Wl,-rpath," + os.path.join(ROOT, "invcompcamtrack_amd")], timeout=300)
    lv_f, step = 2, 4
    for psz, maxiter, eps, patnorm, x_only, k in ((8, 10, 0.01, 1, 0, 5.0), (17, 3, 0.0, 0, 1, 1.5)):
        a, b = K.frames("67x53", 1, bool(patnorm))
        frames = str(tmp_path / "frames.f32")
        np.stack([a, b]).astype(np.float32).tofile(frames)
        pad = psz + 1
        r = subprocess.run([exe, frames, "67", "53", str(pad), str(lv_f), str(step), str(psz), str(maxiter), repr(eps),
                            str(patnorm), str(x_only), repr(k)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.splitlines()
        got = np.array([[float.fromhex(t) for t in ln.split()] for ln in lines[:67 * 53]], np.float32)
        pa, pb = ic.Pyramid(np.ascontiguousarray(a), lv_f, pad, True), ic.Pyramid(np.ascontiguousarray(b), lv_f, pad, True)
        c = pf.CoarseToFineFlow(67, 53, lv_f, step, psz, maxiter=maxiter, eps=eps, patnorm=bool(patnorm),
                                x_only=bool(x_only), cost="huber", huber_k=k).run(pa, pb)
        assert np.array_equal(_bits(got.reshape(53, 67, 2)), _bits(c.dense())), (psz, k)
        for ln, level in zip(lines[67 * 53:], range(lv_f, -1, -1)):
            tok = ln.split()
            assert [int(t) for t in tok[1:7]] == [level] + np.bincount(c.level(level)[2].ravel(), minlength=5).tolist()
            d = np.array([float.fromhex(t) for t in tok[7:]], np.float32)
            assert np.array_equal(_bits(d), _bits(c.level(level)[1]).ravel()), level


# ---------------------------------------------------------------- the stereo pipeline and the CLI
def _same(got, want):
    assert got[1].tobytes() == want[1].tobytes()
    assert got[0].tobytes() == want[0].tobytes()


def test_window_with_the_huber_cost(tmp_path):
    from invcompcamtrack_amd import run_stereo_track as RS
    from invcompcamtrack_amd import stereotrack as S
    from test_gpu_c2frgb import _colour_stereo_frames
    left, right = ([np.ascontiguousarray(f[..., 0]) for f in side] for side in _colour_stereo_frames())
    kw = dict(step=4, psz=8, lv_f=2)

    def window(**extra):
        t = S.StereoPointTracker(96, 64, 4, **kw, **extra)
        for a, b in zip(left, right):
            t.push_frames(a, b)
        return t, t.window()

    t, got = window(keep_grids=True, flow="c2f", cost="huber", huber_k=2.5)
    assert t.cost == "huber" and t.huber_k == 2.5
    assert len(t.flows) == 4 and all(c.cost == "huber" and c.huber_k == 2.5 for f in t.flows for c in f.values())
    want = S.stereo_track_window_host(*RS.dense_fields_of(t))
    _same(got, want)
    assert len(want[1]) > 100
    # an object's field is the stage's on that pair's pyramids, and not the L2 stage's
    pl, pr = ic.Pyramid(left[1], 2, 8, True), ic.Pyramid(right[1], 2, 8, True)
    assert np.array_equal(_bits(pf.c2f_flow(pl, pr, 4, 8, 2, cost="huber", huber_k=2.5)), _bits(t.flows[1]["lr"].dense()))
    assert not np.array_equal(_bits(pf.c2f_flow(pl, pr, 4, 8, 2)), _bits(t.flows[1]["lr"].dense()))
    t1, got1 = window(keep_grids=True, flow="c2f-1d", cost="huber", patnorm=True, refine=dict(n_outer=1, n_sor=2))
    assert t1.huber_k == 5.0 and t1.flows[1]["lr"].x_only and t1.flows[1]["lr"].cost == "huber"
    _same(got1, S.stereo_track_window_host(*RS.dense_fields_of(t1)))
    _, l2 = window(flow="c2f")
    print("survivors of", 96 * 64, "start points: L2", len(l2[1]), "Huber k = 2.5", len(got[1]))
    assert len(l2[1]) > 100 and got[0].tobytes() != l2[0].tobytes()
    # the CLI, on the device and with --host
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        for k, (a, b) in enumerate(zip(left, right)):
            np.save(str(tmp_path / f"l{k}.npy"), a)
            np.save(str(tmp_path / f"r{k}.npy"), b)
            f.write(f"{tmp_path / f'l{k}.npy'} {tmp_path / f'r{k}.npy'}\n")
    base = [lst, str(tmp_path / "o.npz"), "--bsize", "4", "--psz", "8", "--lv_f", "2"]
    for extra in ([], ["--host"]):
        assert RS.main(base + ["--flow", "c2f", "--cost", "huber", "--huber-k", "2.5"] + extra) == 0
        with np.load(base[1]) as zf:
            _same((zf["xy_t"], zf["rows"]), want)
        assert RS.main(base + ["--flow", "c2f-1d", "--cost", "huber", "--patnorm", "--refine", "16,13,4.5,1,2"] + extra) == 0
        with np.load(base[1]) as zf:
            _same((zf["xy_t"], zf["rows"]), got1)
        assert RS.main(base + ["--flow", "c2f", "--cost", "l2"] + extra) == 0
        with np.load(base[1]) as zf:
            _same((zf["xy_t"], zf["rows"]), l2)
    with pytest.raises(SystemExit):
        RS.main(base + ["--cost", "huber"])
    with pytest.raises(ValueError, match="cost='huber' needs flow='c2f'"):
        S.StereoPointTracker(96, 64, 4, flow="grid", cost="huber")


# ---------------------------------------------------------------- refusals
def test_refusals_say_why_and_change_nothing():
    case = K.TABLE[1]
    pa, pb = pyramids(case)
    c = _flow(case, huber_k=2.0)
    L = _lib.load()
    cost, k = C.c_int(), C.c_float()

    def state():
        assert L.ictr_c2fflow_get_cost(c._h, C.byref(cost), C.byref(k)) == 0
        return cost.value, k.value

    assert state() == (pf.C2F_COST_HUBER, 2.0)
    assert L.ictr_c2fflow_set_cost(c._h, 1, 2.0) != 0
    msg = L.ictr_last_error()
    assert b"L1" in msg and b"not built" in msg and b"no scale" in msg and b"huber_k" in msg
    for bad in (3, -1, 4, 256):
        assert L.ictr_c2fflow_set_cost(c._h, bad, 2.0) != 0 and b"0: L2, or 2: Huber" in L.ictr_last_error()
    for code in (pf.C2F_COST_HUBER, pf.C2F_COST_L2):
        for bad in (0.0, -0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            assert L.ictr_c2fflow_set_cost(c._h, code, bad) != 0 and b"finite and > 0" in L.ictr_last_error()
    assert L.ictr_c2fflow_set_cost(None, 0, 1.0) != 0
    assert L.ictr_c2fflow_get_cost(c._h, None, C.byref(k)) != 0 and L.ictr_c2fflow_get_cost(c._h, C.byref(cost), None) != 0
    assert state() == (pf.C2F_COST_HUBER, 2.0)  # no failing call changed it
    for call, why in ((lambda: c.set_cost("l1"), "L1.*not built"), (lambda: c.set_cost("huber", 0.0), "finite and > 0"),
                      (lambda: c.set_cost("median"), "cost is 'median'")):
        with pytest.raises(ValueError, match=why):
            call()
    assert (c.cost, c.huber_k) == ("huber", 2.0)
    want = _flow(case, huber_k=2.0).run(pa, pb).dense()
    assert np.array_equal(_bits(c.run(pa, pb).dense()), _bits(want))  # and the run is the one that was set
    fresh = pf.CoarseToFineFlow(67, 53, 2)
    assert (fresh.cost, fresh.huber_k) == ("l2", 5.0)
    with pytest.raises(ValueError, match="L1.*not built"):
        pf.CoarseToFineFlow(67, 53, 2, cost=1)
    with pytest.raises(ValueError, match="finite and > 0"):
        pf.c2f_flow(pa, pb, 4, 8, 2, cost="huber", huber_k=float("nan"))
