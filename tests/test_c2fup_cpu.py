"""A finest level above 0 of the coarse-to-fine dense flow without a GPU: the definitions (patchflow.upsample_flow_host,
c2f_flow_host(lv_l=...)), their exact properties, the f32 restatement of k_flow_upsample (c2fup_f32.py) against the
definition within its derived bound, the usefulness figures on the host functions alone, and the refusals.

Every figure that c2fup_cases.py records is measured again here and printed; a figure above its record fails, and so does one
below half of it (the record is stale)."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import c2fflow_cases as CC
import c2fup_cases as UC
import c2fup_f32 as R
import flowrefine_cases as FC
from invcompcamtrack_amd import patchflow as pf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = (("definition", pf.upsample_flow_host), ("restatement", R.upsample))


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):  # the host pyramids are the oracle's
    return oracle


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _clamped(n, nl, s):
    return np.clip((np.arange(n) + 0.5) / s - 0.5, 0.0, nl - 1.0)


# ---------------------------------------------------------------- exactness, derived, no tolerance
def test_level_sizes_are_the_pyramids():
    from oracle import oracle as O
    for w, h, lv in UC.SHAPES + ((1920, 1080, 3), (53, 67, 2)):
        assert pf.pyramid_level_size(w, h, lv) == tuple(O.level_size(w, h, lv)), (w, h, lv)
    assert pf.pyramid_level_size(67, 53, 1) == (34, 26) and pf.pyramid_level_size(67, 53, 2) == (17, 13)
    assert pf.pyramid_level_size(3, 2, 1) == (2, 1) and pf.pyramid_level_size(9, 7, 1) == (4, 4)


@pytest.mark.parametrize("name,up", BOTH)
def test_a_constant_field_is_scaled_exactly(name, up):
    for w, h, lv in UC.SHAPES:
        wl, hl = UC.level_size(w, h, lv)
        f = np.empty((hl, wl, 2), np.float32)
        f[...] = (1.5, -0.75)
        want = np.empty((h, w, 2), np.float32)
        want[...] = (1.5 * (1 << lv), -0.75 * (1 << lv))
        assert np.array_equal(_bits(up(f, w, h, lv)), _bits(want)), (name, w, h, lv)


@pytest.mark.parametrize("name,up", BOTH)
def test_a_ramp_pins_the_centres_the_clamp_and_the_factor(name, up):
    """u = x / 4 and v = y / 4 on the level: the output is exactly s fx / 4, s fy / 4 with the clamped fx, fy (every
    product and sum is exact: multiples of 2^-(lv + 3) below 2^11)."""
    for w, h, lv in UC.SHAPES:
        wl, hl = UC.level_size(w, h, lv)
        s = float(1 << lv)
        f = np.empty((hl, wl, 2), np.float32)
        f[..., 0] = np.arange(wl)[None, :] / 4.0
        f[..., 1] = np.arange(hl)[:, None] / 4.0
        got = up(f, w, h, lv)
        want = np.empty((h, w, 2), np.float32)
        want[..., 0] = (s * _clamped(w, wl, s) / 4)[None, :]
        want[..., 1] = (s * _clamped(h, hl, s) / 4)[:, None]
        assert np.array_equal(_bits(got), _bits(want)), (name, w, h, lv)
        assert got[0, 0, 0] == 0 and got[0, -1, 0] <= s * (wl - 1) / 4  # clamped on the left, and never past the right


@pytest.mark.parametrize("name,up", BOTH)
def test_x_only_reads_no_v_and_writes_plus_zero(name, up):
    for w, h, lv in UC.SHAPES[:5]:
        f = UC.field(w, h, lv).copy()
        want = up(f, w, h, lv)[..., 0]
        for v in (-0.0, np.nan, np.inf):
            f[..., 1] = v
            got = up(f, w, h, lv, True)
            assert not _bits(got[..., 1]).any(), (name, w, h, lv, v)
            assert np.array_equal(_bits(got[..., 0]), _bits(want))


def test_lv_l_0_returns_the_bits_of_before_and_the_stages_are_the_leading_ones():
    for case in (CC.TABLE[4], CC.TABLE[3]):
        frame, psz, lv_f, maxiter, eps, _, step = case
        pa, pb = CC.host_pyramids(frame, CC.pad_of(case))
        want, stages = CC.host_run(case)
        st0 = []
        got = pf.c2f_flow_host(pa, pb, step, psz, lv_f, maxiter, eps, refine=CC.refine_of(case), _stages=st0, lv_l=0)
        assert np.array_equal(_bits(got), _bits(want)) and len(st0) == lv_f + 1
        w, h = CC.frame_size(frame)
        for lv_l in (1, 2):
            st = []
            out = pf.c2f_flow_host(pa, pb, step, psz, lv_f, maxiter, eps, refine=CC.refine_of(case), _stages=st, lv_l=lv_l)
            assert [s["level"] for s in st] == list(range(lv_f, lv_l - 1, -1))
            for s, s0 in zip(st, stages):
                assert s["level"] == s0["level"] and np.array_equal(s["status"], s0["status"])
                for k in ("init", "d", "field"):
                    assert np.array_equal(_bits(s[k]), _bits(s0[k]), ), (case, lv_l, k)
            assert out.shape == (h, w, 2) and out.dtype == np.float32
            assert np.array_equal(_bits(out), _bits(pf.upsample_flow_host(st[-1]["field"], w, h, lv_l)))
            assert not np.array_equal(_bits(out), _bits(want))


def test_lv_l_with_x_only_keeps_v_at_plus_zero():
    case = CC.TABLE[4]
    frame, psz, lv_f, maxiter, eps, _, step = case
    pa, pb = CC.host_pyramids(frame, CC.pad_of(case))
    out = pf.c2f_flow_host(pa, pb, step, psz, lv_f, maxiter, eps, x_only=True, lv_l=1)
    assert out[..., 0].any() and not _bits(out[..., 1]).any()


def test_the_restated_run_is_the_stages_of_before_and_their_upsampling():
    case, lv_l, patnorm, x_only = UC.STAGE_CASES[0]
    out, st = UC.restated_run(case, lv_l, patnorm, x_only)
    field0, st0 = CC.restated(case)
    assert [s[0] for s in st] == list(range(case[2], lv_l - 1, -1))
    for s, s0 in zip(st, st0):
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(s[1:], s0[1:]))
    w, h = CC.frame_size(case[0])
    assert np.array_equal(_bits(out), _bits(R.upsample(st[-1][1], w, h, lv_l)))
    assert np.array_equal(_bits(R.run(*CC.host_pyramids(case[0], CC.pad_of(case)), case[6], case[1], case[2], 0, case[3],
                                      case[4])), _bits(field0))


# ---------------------------------------------------------------- restatement against definition
def test_restatement_is_within_its_bound_of_the_definition():
    worst = 0.0
    for w, h, lv in UC.SHAPES:
        for x_only in (False, True):
            for seed in (0, 1):
                f = UC.field(w, h, lv, seed)
                assert np.abs(f).max() <= UC.M and f.min() < 0 < f.max()
                want = pf.upsample_flow_host(f, w, h, lv, x_only)
                got = R.upsample(f, w, h, lv, x_only) if seed else UC.restated(w, h, lv, x_only)
                diff = float(np.abs(got.astype(np.float64) - want).max())
                print(f"{w}x{h} lv {lv} x_only {x_only} seed {seed}: worst |restatement - definition| {diff:.3g}, "
                      f"bound {UC.bound(lv):.3g}")
                assert diff <= UC.bound(lv), (w, h, lv, x_only, seed, diff)
                worst = max(worst, diff / UC.bound(lv))
    print("worst difference over its bound:", f"{worst:.4f}")
    assert UC.WORST_OVER_BOUND / 2 <= worst <= UC.WORST_OVER_BOUND, worst


# ---------------------------------------------------------------- usefulness, on the host functions alone
def test_lv_l_1_holds_its_bar_on_large_relative_motion_and_the_tables_are_recorded():
    ratios = []
    for refined in (False, True):
        for kind in UC.KINDS:
            got = [UC.useful_errors(kind, seed, refined) for seed in FC.SEEDS]
            for k, lv_l in enumerate(UC.LV_LS):
                row = [g[k] for g in got]
                print(f"{kind}{' refined' if refined else ''} lv_l {lv_l}:", " / ".join(f"{v:.3f}" for v in row), "px")
                assert np.allclose(row, UC.RECORDED[kind, refined][k], rtol=0, atol=UC.RECORDED_TOL), (kind, refined, lv_l, row)
    for seed in FC.SEEDS:
        base, at1 = UC.baseline_error("big", seed), UC.useful_errors("big", seed)[1]
        print(f"big seed {seed}: whole-pyramid grid {base:.3f} px -> lv_l 1 {at1:.3f} px, ratio {at1 / base:.3f}")
        assert at1 <= UC.useful_bar() * base, (seed, base, at1)
        ratios.append(at1 / base)
    assert UC.USEFUL_LVL1 / 2 <= max(ratios) <= UC.USEFUL_LVL1 + 5e-4, (ratios, UC.USEFUL_LVL1)
    for kind in ("layers", "rotzoom"):
        print(kind, "whole-pyramid grid:", " / ".join(f"{UC.baseline_error(kind, s):.3f}" for s in FC.SEEDS), "px")


def test_a_run_with_lv_l_returns_the_fields_the_figures_are_taken_on():
    from oracle import oracle as O
    fields, (a, b, _, _) = UC.useful_fields("big", 0)
    pa, pb = O.Pyramid(a, CC.USEFUL_LV, CC.USEFUL_PSZ), O.Pyramid(b, CC.USEFUL_LV, CC.USEFUL_PSZ)
    for lv_l in (1, 2):
        out = pf.c2f_flow_host(pa, pb, CC.STEP, CC.USEFUL_PSZ, CC.USEFUL_LV, lv_l=lv_l)
        assert np.array_equal(_bits(out), _bits(fields[lv_l]))


def test_refining_the_upsampled_field_at_level_0_is_recorded():
    """refine_flow_host on the up-sampled lv_l = 1 field: the combination FlowRefiner.run(src=c2f) gives. No bar."""
    for kind in UC.KINDS:
        fields, (a, b, truth, mask) = UC.useful_fields(kind, 0)
        before = FC.epe(fields[1], truth, mask)
        after = FC.epe(pf.refine_flow_host(a, b, fields[1], **CC.USEFUL_REFINE), truth, mask)
        print(f"{kind} seed 0, lv_l 1: {before:.3f} px -> refined at level 0 {after:.3f} px")
        assert abs(after - UC.REFINED_AFTER[kind]) <= UC.RECORDED_TOL, (kind, after)


# ---------------------------------------------------------------- refusals and the surface
def test_refusals():
    case = CC.TABLE[4]
    frame, psz, lv_f, maxiter, eps, _, step = case
    pa, pb = CC.host_pyramids(frame, CC.pad_of(case))
    for bad in (-1, lv_f + 1, 1.5):
        with pytest.raises(ValueError, match="lv_l"):
            pf.c2f_flow_host(pa, pb, step, psz, lv_f, lv_l=bad)
    f = UC.field(67, 53, 1)
    for up in (pf.upsample_flow_host, pf.upsample_flow):  # the device wrapper refuses before it loads anything
        with pytest.raises(ValueError, match="level 1 of 66 x 53"):
            up(f, 66, 53, 1)
        with pytest.raises(ValueError, match="level 2 of 67 x 53"):
            up(f, 67, 53, 2)
        with pytest.raises(ValueError, match="the field is"):
            up(f[..., 0], 67, 53, 1)
        for lv in (0, 16):
            with pytest.raises(ValueError, match="lv is"):
                up(f, 67, 53, lv)
        with pytest.raises(ValueError, match="empty"):
            up(np.zeros((0, 0, 2), np.float32), 1, 1, 1)


def test_size_rules_hold_for_the_levels_that_run():
    """A coarse level that breaks a rule is refused at any lv_l: 20 x 18 at step 9 has no node at level 2 (5 x 4). A level
    below lv_l is not looked at: frames of 20 x 18 and 21 x 18 differ at level 0 and agree at level 1 (10 x 9), and the
    host function, which reads no plane below lv_l, runs them at lv_l = 1 and refuses them at lv_l = 0."""
    from oracle import oracle as O
    rng = np.random.default_rng(0)
    a = rng.uniform(0, 255, (18, 21)).astype(np.float32)
    p2 = O.Pyramid(a[:, :20], 2, 9)
    for lv_l in (0, 1, 2):
        with pytest.raises(ValueError, match="level 2 .* has no node"):
            pf.c2f_flow_host(p2, p2, 9, 8, 2, lv_l=lv_l)
    pa, pb = O.Pyramid(np.ascontiguousarray(a[:, :20]), 1, 8), O.Pyramid(a, 1, 8)
    with pytest.raises(ValueError, match="differ in size at level 0"):
        pf.c2f_flow_host(pa, pb, 4, 8, 1)
    out = pf.c2f_flow_host(pa, pb, 4, 8, 1, lv_l=1)
    assert out.shape == (18, 20, 2) and np.isfinite(out).all()


def test_the_shapes_overshoot_and_undershoot_the_frame_along_both_axes():
    over_x = {(w, h, lv) for w, h, lv in UC.SHAPES if UC.level_size(w, h, lv)[0] << lv > w}
    under_x = {(w, h, lv) for w, h, lv in UC.SHAPES if UC.level_size(w, h, lv)[0] << lv < w}
    over_y = {(w, h, lv) for w, h, lv in UC.SHAPES if UC.level_size(w, h, lv)[1] << lv > h}
    under_y = {(w, h, lv) for w, h, lv in UC.SHAPES if UC.level_size(w, h, lv)[1] << lv < h}
    assert over_x and under_x and over_y and under_y
    assert (67, 53, 1) in over_x & under_y and (9, 7, 1) in under_x & over_y and UC.level_size(3, 2, 1)[1] == 1


def test_the_library_exports_the_option():
    """The symbols declared in include/ictr.h's text, in the ctypes table with their signatures, and in the library."""
    from invcompcamtrack_amd import _lib
    want = ["ictr_c2fflow_create_lvl", "ictr_c2fflow_get_lv_l", "ictr_c2fflow_get_upsample_ms", "ictr_flow_upsample"]
    i, vp = C.c_int, C.c_void_p
    sigs = {"ictr_c2fflow_create_lvl": (i, [C.POINTER(vp), i, i, i, i, i, i]),
            "ictr_c2fflow_get_lv_l": (i, [vp, C.POINTER(i)]),
            "ictr_c2fflow_get_upsample_ms": (i, [vp, C.POINTER(C.c_float)]),
            "ictr_flow_upsample": (i, [vp, i, i, i, vp, i, i, i, i, vp])}
    assert sorted(sigs) == want
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ictr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ictr_[a-z0-9_]+)\s*\(", txt))
    assert all(n in declared for n in want)
    assert {n: _lib.SIGNATURES[n] for n in want} == sigs
    import __graft_entry__ as g
    g.build()
    raw = C.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, n) for n in want)


def test_the_c_entry_points_check_their_arguments_before_they_ask_for_a_device():
    import invcompcamtrack_amd as ic
    from invcompcamtrack_amd import _lib
    L = _lib.load()
    f, out, h = UC.field(67, 53, 1), np.zeros((53, 67, 2), np.float32), C.c_void_p()
    bad = ((pf.fp(f), 34, 26, 1, pf.fp(out), 66, 53), (pf.fp(f), 34, 26, 0, pf.fp(out), 67, 53),
           (pf.fp(f), 34, 26, 16, pf.fp(out), 67, 53), (None, 34, 26, 1, pf.fp(out), 67, 53), (pf.fp(f), 34, 26, 1, None, 67, 53),
           (pf.fp(f), 0, 0, 1, pf.fp(out), 1, 1))
    for args in bad:
        assert L.ictr_flow_upsample(*args, 0, 0, None) == 1, args  # ICTR_ERR_INVALID
        assert b"flow_upsample" in L.ictr_last_error()
    for lv_l in (-1, 3):
        assert L.ictr_c2fflow_create_lvl(C.byref(h), 67, 53, 2, lv_l, 4, 8) == 1 and not h.value
        assert b"lv_l is" in L.ictr_last_error()
    if ic.device_count() < 1:  # no fall-back: a valid call fails loudly without a device
        with pytest.raises(_lib.IctrError, match="no usable HIP device"):
            pf.upsample_flow(f, 67, 53, 1)
        with pytest.raises(_lib.IctrError, match="no usable HIP device"):
            pf.CoarseToFineFlow(67, 53, 2, lv_l=1)


def test_the_stereo_tracker_and_the_cli_refuse_lv_l_with_the_grid_flow():
    from invcompcamtrack_amd import run_stereo_track as RS
    from invcompcamtrack_amd import stereotrack as S
    with pytest.raises(ValueError, match="lv_l > 0 needs flow='c2f'"):
        S.StereoPointTracker(96, 64, 4, lv_l=1)
    with pytest.raises(SystemExit):
        RS.main(["-", "o.npz", "--lv-l", "1"])
    with pytest.raises(SystemExit):
        RS.main(["-", "o.npz", "--flow", "grid", "--lv-l", "1"])
