"""Coarse-to-fine dense flow without a GPU: the definition (patchflow.c2f_flow_host), the f32 restatement of the kernel and
its launcher (c2fflow_f32.py) against it over the case table, level by level from the same starts, the injectable defects,
the exact properties of the rule, its refusals and the usefulness bar.

Every figure that c2fflow_cases.py records is measured again here and printed; a figure above its record fails, and so does
one below half of it (the record is stale)."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import c2fflow_cases as CC
import c2fflow_f32 as R
import densify_f32 as DZ
import flowrefine_cases as FC
from invcompcamtrack_amd import patchflow as pf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATUS_CASE = next(c for c in CC.TABLE if c[0] == "status-96x64")
STEP3_CASE = next(c for c in CC.TABLE if c[6] == 3)


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):  # the host pyramids are the oracle's
    return oracle


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- the table
def test_the_table_covers_what_it_names():
    assert {c[0] for c in CC.TABLE} >= {"100x77", "67x53", "farxy-320x64", "farxy-64x320"}
    assert {R.form_shape(c[1]) for c in CC.TABLE} == {(1, 1), (4, 1), (8, 2)}
    assert {c[1] for c in CC.TABLE} == {8, 15, 23, 32} and {c[0] for c in CC.TABLE if c[1] > 15} == {"67x53"}
    assert {c[1] for c in CC.TABLE if c[4] == 0.0} == {8, 15, 23, 32}
    assert any(c[2] == 1 and c[0] == "67x53" for c in CC.TABLE) and any(c[3] == 2 for c in CC.TABLE)
    assert sum(1 for c in CC.TABLE if c[5]) == 1
    assert {CC.pad_of(c) - c[1] for c in CC.TABLE} == set(CC.PAD_EXTRA)
    # every status value occurs on the seeded pair, on the definition
    seen = np.zeros(5, int)
    for s in CC.host_run(STATUS_CASE)[1]:
        seen += np.bincount(s["status"].ravel(), minlength=5)
    print("status counts of the seeded pair over its levels:", seen.tolist())
    assert (seen > 0).all(), seen
    # the clamp row is asked for at step 3: a node in row 52 of 53 over a level of 26 rows
    s0 = CC.host_run(STEP3_CASE)[1][-1]
    assert s0["level"] == 0 and s0["status"].shape[0] == 18 and (1 + 3 * 17) >> 1 == 26 == CC.host_run(STEP3_CASE)[1][-2][
        "field"].shape[0]


@pytest.mark.parametrize("case", CC.STATUS_FORMS, ids=lambda c: f"psz{c[1]}")
def test_the_status_pair_reaches_every_status_in_the_other_forms(case):
    """A condition on the input: over the three levels of the restatement's run, every status value 0..4 occurs."""
    assert R.form_shape(case[1]) == {15: (4, 1), 17: (8, 2)}[case[1]]
    seen = np.zeros(5, int)
    for _, _, _, status in CC.restated(case)[1]:
        seen += np.bincount(status.ravel(), minlength=5)
    print("psz", case[1], "pad", CC.pad_of(case), "status counts over the levels:", seen.tolist())
    assert len(CC.restated(case)[1]) == 3 and (seen > 0).all(), seen


def test_restatement_differences_are_within_their_records():
    worst = {}
    left, field = (0.0, None), 0.0
    for case in CC.TABLE:
        for level, nodes, out, same, diff in CC.level_differences(case):
            assert same, (case, level, "a status differs on a node whose decisions all have their margins")
            worst[level] = max(worst.get(level, 0.0), diff)
            if nodes >= CC.LEFT_OUT_MIN_NODES:
                assert out <= CC.LEFT_OUT_CAP * nodes, (case, level, out, nodes, "take another frame or seed")
                if out / nodes > left[0]:
                    left = (out / nodes, (case[0], case[1], level))
        if case[4] == 0.0:
            field = max(field, float(np.abs(CC.restated(case)[0].astype(np.float64) - CC.host_run(case)[0]).max()))
    print("worst |d - definition| per level:", {l: float(f"{v:.3g}") for l, v in worst.items()},
          "final field over eps = 0:", f"{field:.3g}", "worst share left out:", f"{left[0]:.4f}", left[1])
    for level, rec in CC.D_DIFF.items():
        assert rec / 2 <= worst[level] <= rec, (level, worst[level], rec)
    assert CC.FIELD_DIFF / 2 <= field <= CC.FIELD_DIFF, (field, CC.FIELD_DIFF)
    assert left[1] == CC.LEFT_OUT[1] and CC.LEFT_OUT[0] / 2 <= left[0] <= CC.LEFT_OUT[0], (left, CC.LEFT_OUT)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_defect_is_seen(defect):
    """By the bits of a whole run (what the GPU tests compare), and by the comparison with the definition."""
    case = STEP3_CASE if defect in ("init not doubled", "init row up", "no clamp") else STATUS_CASE
    good, bad = CC.restated(case), CC.restated(case, defect)
    assert not np.array_equal(_bits(good[0]), _bits(bad[0])), "the final field keeps its bits"
    assert any(not np.array_equal(_bits(g[2]), _bits(b[2])) or not np.array_equal(g[3], b[3])
               for g, b in zip(good[1], bad[1])), "every level's d and status keep their bits"
    if case is STEP3_CASE:  # the starts themselves, against the definition's
        stages = CC.host_run(case)[1]
        differs = False
        for coarse, s in zip(stages[:-1], stages[1:]):
            h, w = s["field"].shape[:2]
            assert np.array_equal(_bits(R.init_of(coarse["field"], w, h, case[6])), _bits(s["init"]))
            differs |= not np.array_equal(_bits(R.init_of(coarse["field"], w, h, case[6], defect)), _bits(s["init"]))
        assert differs
    else:  # the search from the definition's starts
        res = CC.level_differences(case, defect)
        assert any(not same or diff > CC.D_DIFF[level] for level, _, _, same, diff in res), res


# ---------------------------------------------------------------- exact properties, definition and restatement
def _runs(case, **over):
    """[(level, init or None, d, status, field)] per level of the definition and of the restatement."""
    frame, psz, lv_f, maxiter, eps, _, step = case
    maxiter = over.get("maxiter", maxiter)
    lv_f = over.get("lv_f", lv_f)
    pa, pb = CC.host_pyramids(frame, CC.pad_of(case))
    st, rs = [], []
    pf.c2f_flow_host(pa, pb, step, psz, lv_f, maxiter, eps, _stages=st)
    R.run(pa, pb, step, psz, lv_f, maxiter, eps, stages=rs)
    return ([(s["level"], s["init"], s["d"], s["status"], s["field"]) for s in st],
            [(l, None, d, status, field) for l, field, d, status in rs])


def test_maxiter_0_gives_zeros_at_every_level():
    for case in (CC.TABLE[0], STATUS_CASE):
        for which in _runs(case, maxiter=0):
            for level, _, d, status, field in which:
                assert not _bits(field).any() and not _bits(d).any(), (case, level)
                assert np.isin(status, (pf.C2F_TRACKED, pf.C2F_HELD_COND)).all()


def test_held_nodes_keep_their_starts_bits_and_lost_ones_start_out_of_view():
    frame, psz, lv_f, maxiter, eps, _, step = STATUS_CASE
    pa, pb = CC.host_pyramids(frame, CC.pad_of(STATUS_CASE))
    definition, restatement = _runs(STATUS_CASE)
    for which in (definition, restatement):
        coarse = None
        for level, _, d, status, field in which:
            h, w = field.shape[:2]
            init = R.init_of(coarse, w, h, step)
            held = status >= pf.C2F_HELD_COND
            assert held.any() or level == lv_f
            assert np.array_equal(_bits(d[held]), _bits(init[held])), level
            xs, ys = np.meshgrid(np.arange(step // 2, w, step), np.arange(step // 2, h, step))
            sx, sy = xs + init[..., 0].astype(np.float64), ys + init[..., 1].astype(np.float64)
            out = ~((sx >= 0) & (sx <= w) & (sy >= 0) & (sy <= h))
            lost = status == pf.C2F_LOST
            assert not (lost & ~out).any(), level               # status 0 only where the start is out of view ...
            far = np.minimum(np.minimum(sx, w - sx), np.minimum(sy, h - sy))
            assert lost[out & (np.abs(far) > 1e-3)].all(), level   # ... and everywhere it clearly is
            coarse = field
    assert any((s == pf.C2F_LOST).any() for _, _, _, s, _ in definition)


def test_one_level_without_held_or_lost_nodes_is_the_densifier_on_the_same_nodes():
    case = next(c for c in CC.TABLE if c[0] == "farxy-320x64" and c[1] == 8)
    frame, psz, _, maxiter, eps, _, step = case
    pa, pb = CC.host_pyramids(frame, CC.pad_of(case))
    A, B = R.plane(pa, 0), R.plane(pb, 0)
    (definition,), (restatement,) = _runs(case, lv_f=0)
    for (_, _, d, status, field), densify in ((definition, lambda d, lost: pf.densify_flow_host(A, B, d, lost, step, psz)),
                                              (restatement, lambda d, lost: DZ.densify(A, B, d, lost, step, psz))):
        assert (status == pf.C2F_TRACKED).all()
        assert np.array_equal(_bits(field), _bits(densify(d, np.zeros(status.shape, bool))))


def test_refusals_say_why():
    pa, pb = CC.host_pyramids("67x53", 9)
    with pytest.raises(ValueError, match="no node"):
        pf.c2f_flow_host(pa, pb, step=40, psz=8, lv_f=2)
    with pytest.raises(ValueError, match="psz is 1 .. 32"):
        pf.c2f_flow_host(pa, pb, psz=33)
    with pytest.raises(ValueError, match="psz is 1 .. 32"):
        pf.c2f_flow_host(pa, pb, psz=0)
    with pytest.raises(ValueError, match="padding must be >= psz"):
        pf.c2f_flow_host(pa, pb, psz=10)
    with pytest.raises(ValueError, match="levels 0 .. 2"):
        pf.c2f_flow_host(pa, pb, lv_f=3)
    from oracle import oracle as O
    a, b = FC.pair("9x7")
    qa, qb = O.Pyramid(a, 2, 8), O.Pyramid(b, 2, 8)     # 9 x 7 -> 4 x 4 -> 2 x 2
    with pytest.raises(ValueError, match="refinement needs 4 x 4"):
        pf.c2f_flow_host(qa, qb, step=2, psz=8, lv_f=2, refine={})
    assert pf.c2f_flow_host(qa, qb, step=2, psz=8, lv_f=2).shape == (7, 9, 2)
    ra, rb = O.Pyramid(a, 3, 8), O.Pyramid(b, 3, 8)     # ... -> 1 x 1
    with pytest.raises(ValueError, match="smaller than 2 px"):
        pf.c2f_flow_host(ra, rb, step=1, psz=8, lv_f=3)


def test_the_library_exports_the_stage():
    """The symbols of the stage in include/ictr.h, in the library and in the ctypes table."""
    from invcompcamtrack_amd import _lib
    want = ["ictr_c2fflow_" + n for n in ("create", "destroy", "set_params", "set_refine", "run", "result", "device_ptr",
                                           "level_dims", "read_level", "set_timing", "get_kernel_ms",
                                           "set_patnorm", "read_level_bias", "set_x_only", "get_x_only", "create_lvl",
                                           "get_lv_l", "get_upsample_ms", "set_channels", "get_channels", "run_rgb",
                                           "read_level_bias_rgb")]
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ictr.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(ictr_c2fflow_[a-z0-9_]+)\s*\(", txt))) == sorted(want)
    assert re.search(r"\bictr_flow_upsample\s*\(", txt)  # the up-sampling of a finest level above 0 is declared with them
    want.append("ictr_flow_upsample")
    import __graft_entry__ as g
    g.build()
    raw = C.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, n) and n in _lib.SIGNATURES for n in want)
    assert [getattr(pf, "C2F_" + n) for n in ("LOST", "TRACKED", "HELD_COND", "HELD_VIEW", "HELD_FAR")] == [
        int(v) for v in re.findall(r"#define\s+ICTR_C2F_[A-Z_]+\s+(\d)", txt)]


# ---------------------------------------------------------------- usefulness
def test_coarse_to_fine_holds_its_bar_on_large_relative_motion():
    ratios = []
    for seed in FC.SEEDS:
        base, c2f = CC.useful_errors("big", seed)
        print(f"big seed {seed}: baseline {base:.3f} px -> coarse-to-fine {c2f:.3f} px, ratio {c2f / base:.3f}")
        ratios.append(c2f / base)
        assert c2f <= CC.useful_bar() * base, (seed, base, c2f)
    assert CC.USEFUL_BIG / 2 <= max(ratios) <= CC.USEFUL_BIG + 5e-4, (ratios, CC.USEFUL_BIG)


@pytest.mark.parametrize("kind", ("layers", "rotzoom"))
def test_no_worse_where_no_gain_is_expected(kind):
    for seed in FC.SEEDS:
        base, c2f = CC.useful_errors(kind, seed)
        print(f"{kind} seed {seed}: baseline {base:.3f} px -> coarse-to-fine {c2f:.3f} px")
        assert c2f <= CC.NO_WORSE * base, (kind, seed, base, c2f)


def test_the_run_with_refinement_is_recorded():
    base, c2f = CC.useful_errors("big", 0, CC.USEFUL_REFINE)
    print(f"big seed 0, both refined: baseline {base:.3f} px -> coarse-to-fine {c2f:.3f} px")
    assert np.isfinite(base) and np.isfinite(c2f)
