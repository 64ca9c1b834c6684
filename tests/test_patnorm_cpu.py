"""Patch-mean normalisation of the coarse-to-fine dense flow without a GPU: the definition
(patchflow.c2f_flow_host(patnorm=True) with _c2f_search_host, _c2f_bias_host and densify_flow_host's bias), the f32
restatement of the MEAN kernels (patnorm_f32.py) against it over the case table, level by level from the same starts, the
injectable defects, the exact properties of the rule, the offset invariance and the usefulness bar.

Every figure that patnorm_cases.py records is measured again here and printed; a figure above its record fails, and so does
one below half of it (the record is stale)."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import c2fflow_cases as CC
import c2fflow_f32 as R0
import flowrefine_cases as FC
import patnorm_cases as PN
import patnorm_f32 as R
from invcompcamtrack_amd import patchflow as pf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATUS8 = PN.STATUS_CASES[0]
VOTE_CASE = PN.TABLE[0]


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):  # the host pyramids are the oracle's
    return oracle


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- the table
def test_the_table_covers_what_it_names():
    assert {R0.form_shape(c[1]) for c in PN.TABLE} == {(1, 1), (4, 1), (8, 2)}
    assert {R0.form_shape(c[1]) for c in PN.TABLE if c[4] == 0.0} == {(1, 1), (4, 1), (8, 2)}
    assert {c[7] for c in PN.TABLE} == {"+20", "ramp", "gain", "none"}
    assert {PN.pad_of(c) - c[1] for c in PN.TABLE} == set(PN.PAD_EXTRA)
    assert sum(1 for c in PN.TABLE if c[5]) == 1 and any(c[6] == 3 for c in PN.TABLE) and any(c[2] == 1 for c in PN.TABLE)
    assert {R0.form_shape(c[1]) for c in PN.STATUS_CASES} == {(1, 1), (4, 1), (8, 2)}


@pytest.mark.parametrize("case", PN.STATUS_CASES, ids=lambda c: f"psz{c[1]}")
def test_the_status_pair_holds_stopped_nodes_in_every_form(case):
    """A condition on the input: over the three levels of the definition's and of the restatement's run the recorded
    status values occur, nodes stopped by the conditioning test (2) and by the view test (3) among them in every form."""
    for name, levels in (("definition", [s["status"] for s in PN.host_run(case)[1]]),
                         ("restatement", [s[3] for s in PN.restated(case)[1]])):
        seen = np.zeros(5, int)
        for status in levels:
            seen += np.bincount(status.ravel(), minlength=5)
        print("psz", case[1], name, "status counts over the levels:", seen.tolist())
        assert len(levels) == 3 and tuple(np.nonzero(seen)[0]) == PN.STATUS_REACHED[case[1]], seen
        assert seen[2] > 0 and seen[3] > 0


def test_restatement_differences_are_within_their_records():
    worst_d, worst_b = {}, {}
    left, field = (0.0, None), 0.0
    for case in PN.TABLE:
        for level, nodes, out, same, diff, bdiff in PN.level_differences(case):
            assert same, (case, level, "a status differs on a node whose decisions all have their margins")
            worst_d[level] = max(worst_d.get(level, 0.0), diff)
            worst_b[level] = max(worst_b.get(level, 0.0), bdiff)
            if nodes >= CC.LEFT_OUT_MIN_NODES:
                assert out <= CC.LEFT_OUT_CAP * nodes, (case, level, out, nodes, "take another frame or seed")
                if out / nodes > left[0]:
                    left = (out / nodes, (case[0], case[1], case[6], level))
        if case[4] == 0.0:
            field = max(field, float(np.abs(PN.restated(case)[0].astype(np.float64) - PN.host_run(case)[0]).max()))
    print("worst |d - definition| per level:", {l: float(f"{v:.3g}") for l, v in worst_d.items()},
          "worst |beta - definition| per level:", {l: float(f"{v:.3g}") for l, v in worst_b.items()},
          "final field over eps = 0:", f"{field:.3g}", "worst share left out:", f"{left[0]:.4f}", left[1])
    for level in PN.D_DIFF:
        assert PN.D_DIFF[level] / 2 <= worst_d[level] <= PN.D_DIFF[level], (level, worst_d[level])
        assert PN.BIAS_DIFF[level] / 2 <= worst_b[level] <= PN.BIAS_DIFF[level], (level, worst_b[level])
    assert PN.FIELD_DIFF / 2 <= field <= PN.FIELD_DIFF, (field, PN.FIELD_DIFF)
    assert left[1] == PN.LEFT_OUT[1] and PN.LEFT_OUT[0] / 2 <= left[0] <= PN.LEFT_OUT[0], (left, PN.LEFT_OUT)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_defect_is_seen(defect):
    """By the bits of a whole run (what the GPU tests compare), and by the comparison with the definition."""
    case = VOTE_CASE if defect == "vote ignores beta" else STATUS8
    good, bad = PN.restated(case), PN.restated(case, defect)
    assert not np.array_equal(_bits(good[0]), _bits(bad[0])), "the final field keeps its bits"
    if defect == "vote ignores beta":  # the search and the bias are right: the fields of the levels differ
        assert all(np.array_equal(_bits(g[4]), _bits(b[4])) for g, b in zip(good[1][:1], bad[1][:1]))
        assert any(not np.array_equal(_bits(g[1]), _bits(b[1])) for g, b in zip(good[1], bad[1]))
        assert case[4] == 0.0
        assert float(np.abs(bad[0].astype(np.float64) - PN.host_run(case)[0]).max()) > PN.FIELD_DIFF
        return
    assert any(not np.array_equal(_bits(g[2]), _bits(b[2])) or not np.array_equal(g[3], b[3])
               or not np.array_equal(_bits(g[4]), _bits(b[4])) for g, b in zip(good[1], bad[1]))
    res = PN.level_differences(case, defect)
    assert any(not same or diff > PN.D_DIFF[level] or bdiff > PN.BIAS_DIFF[level]
               for level, _, _, same, diff, bdiff in res), res


# ---------------------------------------------------------------- exact properties
def test_patnorm_off_and_no_bias_are_the_operations_of_before():
    case = CC.TABLE[0]
    frame, psz, lv_f, maxiter, eps, _, step = case
    pa, pb = CC.host_pyramids(frame, CC.pad_of(case))
    st = []
    off = pf.c2f_flow_host(pa, pb, step, psz, lv_f, maxiter, eps, patnorm=False, _stages=st)
    assert np.array_equal(_bits(off), _bits(CC.host_run(case)[0]))
    assert all(s["bias"] is None for s in st)
    s0 = st[-1]
    lost = s0["status"] == pf.C2F_LOST
    A, B = R0.plane(pa, 0), R0.plane(pb, 0)
    d = np.where(lost[..., None], np.float32(0), s0["d"])
    plain = pf.densify_flow_host(A, B, d, lost, step, psz)
    assert np.array_equal(_bits(pf.densify_flow_host(A, B, d, lost, step, psz, bias=None)), _bits(plain))
    assert np.array_equal(_bits(plain), _bits(s0["field"]))
    # a zero bias takes nothing off a residual
    assert np.array_equal(_bits(pf.densify_flow_host(A, B, d, lost, step, psz, bias=np.zeros(lost.shape))), _bits(plain))
    with pytest.raises(ValueError, match="bias"):
        pf.densify_flow_host(A, B, d, lost, step, psz, bias=np.zeros((2, 2)))


def test_lost_nodes_and_finals_out_of_view_have_a_bias_of_plus_zero():
    out_of_view = 0
    for case in PN.STATUS_CASES:
        step = case[6]
        levels = ([(s["d"], s["status"], np.asarray(s["bias"], np.float32)) for s in PN.host_run(case)[1]],
                  [(d, status, bias) for _, _, d, status, bias in PN.restated(case)[1]])
        for which in levels:
            for (d, status, bias), s in zip(which, PN.host_run(case)[1]):
                h, w = s["field"].shape[:2]
                xs, ys = np.meshgrid(np.arange(step // 2, w, step), np.arange(step // 2, h, step))
                fx, fy = xs + d[..., 0].astype(np.float64), ys + d[..., 1].astype(np.float64)
                far = np.minimum(np.minimum(fx, w - fx), np.minimum(fy, h - fy))
                lost = status == pf.C2F_LOST
                gone = ~lost & (far < -CC.MARGIN_PX)
                out_of_view += int(gone.sum())
                assert not _bits(bias[lost | gone]).any()
                assert (bias[~lost & (far > CC.MARGIN_PX)] != 0).any()
    assert out_of_view > 0


def test_maxiter_0_gives_zeros_at_every_level():
    case = STATUS8
    frame, psz, lv_f, _, eps, _, step, _ = case
    pa, pb = PN.pyramids_of(case)
    st, rs = [], []
    pf.c2f_flow_host(pa, pb, step, psz, lv_f, 0, eps, _stages=st, patnorm=True)
    R.run(pa, pb, step, psz, lv_f, 0, eps, stages=rs)
    for d, status, field in [(s["d"], s["status"], s["field"]) for s in st] + [(d, status, f) for _, f, d, status, _ in rs]:
        assert not _bits(field).any() and not _bits(d).any()
        assert np.isin(status, (pf.C2F_TRACKED, pf.C2F_HELD_COND)).all()


def test_a_held_nodes_d_has_its_starts_bits():
    case = STATUS8
    step = case[6]
    for which in ([(s["d"], s["status"], s["field"]) for s in PN.host_run(case)[1]],
                  [(d, status, f) for _, f, d, status, _ in PN.restated(case)[1]]):
        coarse, held_seen = None, 0
        for d, status, field in which:
            h, w = field.shape[:2]
            init = R0.init_of(coarse, w, h, step)
            held = status >= pf.C2F_HELD_COND
            held_seen += int(held.sum())
            assert np.array_equal(_bits(d[held]), _bits(init[held]))
            coarse = field
        assert held_seen > 0


def test_the_library_exports_the_option():
    """The two symbols declared in include/ictr.h's text, in the ctypes table with their signatures, and in the library."""
    from invcompcamtrack_amd import _lib
    want = ["ictr_c2fflow_read_level_bias", "ictr_c2fflow_set_patnorm"]
    sigs = {"ictr_c2fflow_set_patnorm": (C.c_int, [C.c_void_p, C.c_int]),
            "ictr_c2fflow_read_level_bias": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)])}
    assert sorted(sigs) == want
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ictr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ictr_[a-z0-9_]+)\s*\(", txt))
    assert all(n in declared for n in want)
    assert {n: _lib.SIGNATURES[n] for n in want} == sigs
    import __graft_entry__ as g
    g.build()
    raw = C.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, n) for n in want)


def test_the_stereo_tracker_refuses_patnorm_on_flow_grids():
    from invcompcamtrack_amd import stereotrack as S
    with pytest.raises(ValueError, match="patnorm=True needs flow='c2f'"):
        S.StereoPointTracker(96, 64, 4, flow="grid", patnorm=True)
    with pytest.raises(ValueError, match="patnorm=True needs flow='c2f'"):
        S.StereoPointTracker(96, 64, 4, patnorm=True)


# ---------------------------------------------------------------- offset invariance and usefulness, host definitions alone
def test_an_offset_of_20_grey_levels_leaves_the_field_where_it_was():
    worst = 0.0
    for kind in PN.KINDS:
        for seed in FC.SEEDS:
            diff = float(np.abs(PN.useful_field(kind, seed, "+20", True).astype(np.float64)
                                - PN.useful_field(kind, seed, "none", True)).max())
            print(f"{kind} seed {seed}: worst |field(A, B + 20) - field(A, B)| = {diff:.3g} px")
            worst = max(worst, diff)
    assert PN.OFFSET_DIFF / 2 <= worst <= PN.OFFSET_DIFF, (worst, PN.OFFSET_DIFF)


def test_patnorm_holds_its_bar_under_an_offset_and_its_cost_is_recorded():
    ratios = {}
    for kind in PN.KINDS:
        for seed in FC.SEEDS:
            plain, norm = PN.useful_error(kind, seed, "+20", False), PN.useful_error(kind, seed, "+20", True)
            print(f"{kind} seed {seed}, B + 20: plain {plain:.4f} px -> patnorm {norm:.4f} px, ratio {norm / plain:.3f}")
            ratios[kind, seed] = norm / plain
            assert norm <= PN.useful_bar() * plain, (kind, seed, plain, norm)
    worst = max(ratios, key=ratios.get)
    assert worst == PN.USEFUL_OFFSET[1] and PN.USEFUL_OFFSET[0] / 2 <= ratios[worst] <= PN.USEFUL_OFFSET[0] + 5e-4, ratios
    for kind in PN.KINDS:  # recorded, no bar: the cost on unchanged brightness
        for seed in FC.SEEDS:
            plain, norm = PN.useful_error(kind, seed, "none", False), PN.useful_error(kind, seed, "none", True)
            print(f"{kind} seed {seed}, B: plain {plain:.4f} px -> patnorm {norm:.4f} px, cost ratio {norm / plain:.3f}")
            assert np.isfinite(plain) and np.isfinite(norm)


@pytest.mark.parametrize("change", ("ramp", "gain"))
def test_the_ramp_and_the_gain_are_recorded(change):
    for kind in PN.KINDS:
        plain, norm = PN.useful_error(kind, 0, change, False), PN.useful_error(kind, 0, change, True)
        print(f"{kind} seed 0, {change}: plain {plain:.4f} px -> patnorm {norm:.4f} px")
        assert np.isfinite(plain) and np.isfinite(norm)
