"""CPU half of test_gpu_icgn_sums.py: the checks that module makes can fail, and its inputs are well posed.

For every case of icgn_cases.CASES and every level: the f64 oracle's H and b move by many times the bound when the
template region loses one column or one row (so a kernel that drops an edge pixel is caught), no template pixel lands
within 1e-3 px of the in-frame test's thresholds (so f32 and f64 take the same side of the step), the far warp leaves
the stated share of the template outside, and the helper's per-lane load L equals a thread-by-thread count."""
import numpy as np
import pytest

import icgn_cases as IC
from oracle import np_icgn as NI


def _distinct(cases):
    """Cases that share oracle inputs share a record; keep the largest L (the widest bound) per record."""
    seen = {}
    for c in cases:
        for l in IC.LEVELS:
            key = (c.frame, c.model, c.region, c.warp, l)
            L = IC.lane_load(c, l)
            old = seen.get(key, (0, 0))
            seen[key] = (max(old[0], L[0]), max(old[1], L[1]))
    return seen


@pytest.mark.parametrize("frame", list(IC.FRAMES))
def test_one_pixel_edge_moves_the_sums_far_beyond_the_bound(oracle, frame):
    worst_H, worst_b = np.inf, np.inf
    for (fr, model, region, warp, l), (LH, Lb) in _distinct([c for c in IC.CASES if c.frame == frame]).items():
        reg0 = IC.region_px(fr, region)
        M0 = IC.warp_px(fr, model, warp)
        rec = IC.oracle_record(oracle, fr, model, l, reg0, M0)
        tolH, tolb = IC.tolerances(rec, LH, Lb)
        moved_b = live = 0
        for edge, r in IC.trimmed_regions(reg0, l).items():
            cut = IC.oracle_record(oracle, fr, model, l, r, M0)
            assert cut.npx < rec.npx
            rH = (np.abs(cut.H - rec.H) / tolH).max()
            rb = (np.abs(cut.b - rec.b) / tolb).max()
            assert rH >= 100, (model, region, warp, l, edge, rH)
            live += round(rec.inframe * rec.npx) > round(cut.inframe * cut.npx)   # the lost pixels reach the frame
            worst_H = min(worst_H, rH)
            if rb >= 5:
                moved_b += 1
                worst_b = min(worst_b, rb)
        # an edge whose pixels all land outside the current frame adds nothing to b: the far warp pushes the last
        # columns and the first rows out, so two edges are all it can ask for; every other warp keeps all four
        assert live >= (2 if warp == "far" else 4), (model, region, warp, l, live)
        assert moved_b >= min(3, live), (model, region, warp, l, moved_b)
    print(f"[icgn-sums-cpu] {frame}: smallest move of H {worst_H:.0f} x tol, of b {worst_b:.1f} x tol")


@pytest.mark.parametrize("frame", list(IC.FRAMES))
def test_inputs_stay_clear_of_the_in_frame_step(oracle, frame):
    for (fr, model, region, warp, l) in _distinct([c for c in IC.CASES if c.frame == frame]):
        rec = IC.oracle_record(oracle, fr, model, l, IC.region_px(fr, region), IC.warp_px(fr, model, warp))
        assert rec.margin >= 1e-3, (model, region, warp, l, rec.margin)
        if warp == "far":
            assert 0.7 <= rec.inframe <= 0.95, (model, region, l, rec.inframe)
        assert np.abs(rec.b).max() > 0 and rec.npx >= 100


def test_bands_partition_the_region_and_stay_clear_of_the_step(oracle):
    from invcompcamtrack_amd import icgn
    for fr in IC.BAND_FRAMES:
        w, h, _ = IC.frame_size(fr)
        reg0 = IC.region_px(fr, "default")
        assert any((hi - lo) % 4 for world in IC.BAND_SPLITS[fr] for lo, hi in icgn.shard_rows(2, h - 2, world))
        for world, model in [(n, m) for n in IC.BAND_SPLITS[fr] for m in IC.MODELS]:
            bands = icgn.shard_rows(2, h - 2, world)
            M0 = IC.warp_px(fr, model, "far")
            for l in IC.LEVELS:
                whole = IC.oracle_record(oracle, fr, model, l, reg0, M0)
                parts = [IC.oracle_record(oracle, fr, model, l, reg0, M0, rows=b) for b in bands]
                assert sum(p.npx for p in parts) == whole.npx
                assert np.allclose(sum(p.H for p in parts), whole.H, rtol=1e-12, atol=0)
                assert np.allclose(sum(p.b for p in parts), whole.b, rtol=1e-10, atol=1e-9 * np.abs(whole.b).max())
                assert np.allclose(sum(p.majb for p in parts), whole.majb, rtol=1e-12)
                one = IC.oracle_record(oracle, fr, model, l, reg0, M0, rows=IC.ONE_ROW)
                assert one.npx == NI.region_at(reg0, l)[2]
                none = IC.oracle_record(oracle, fr, model, l, reg0, M0, rows=IC.EMPTY)
                assert none.npx == 0 and not none.H.any() and not none.b.any()


def test_level_sizes_and_forms_of_the_case_table(oracle):
    for fr, (w, h, pad, _) in IC.FRAMES.items():
        for l in IC.LEVELS:
            assert IC.level_size(w, h, l) == oracle.level_size(w, h, l)
    form = {fr: [IC.iter_form(fr, l, "default") for l in IC.LEVELS] for fr in IC.FRAMES}
    assert form["75x51p4"] == ["scalar"] * 3 and form["70x46p2"] == ["scalar"] * 3
    assert form["76x52p4"] == ["vector", "scalar", "scalar"]
    assert form["96x40p16"][:2] == ["vector", "vector"] and form["300x20p4"][0] == form["288x24p16"][0] == "vector"
    assert (96 + 32) % 32 == 0 and (48 + 32) % 32 != 0 and (288 + 32) % 32 == 0      # 32-float and 4-float starts
    # the LDS window: theta = 0.01 is staged everywhere, theta = 0.2 on the 96-wide frame is not
    for c in IC.CASES:
        if c.form == "lds" and c.warp in ("rot001", "near"):
            assert IC.lds_rows(c.frame, c.model, c.warp, 0, c.region) <= IC.LDS_H, c
    assert IC.lds_rows("96x40p16", "se2", "rot02", 0, "default") > IC.LDS_H
    # every path of the issue's list is reached by some case
    have = {(c.frame, c.form, c.gridx) for c in IC.CASES}
    for fr in IC.FRAMES:
        assert {(fr, "default", None), (fr, "default", 1), (fr, "default", 3)} <= have
    for fr in IC.VECTOR_FRAMES:
        assert {(fr, "lds", None), (fr, "scalar", None), (fr, "lds", 3), (fr, "scalar", 1)} <= have
    assert len({IC.case_id(c) for c in IC.CASES}) == len(IC.CASES)


@pytest.mark.parametrize("frame,region,level,gridx", [("76x52p4", "odd", 0, 3), ("96x40p16", "default", 0, 1),
                                                        ("300x20p4", "odd", 0, 3), ("75x51p4", "default", 2, None)])
def test_lane_load_matches_a_thread_by_thread_count(frame, region, level, gridx):
    w, h, pad = IC.frame_size(frame)
    reg0 = IC.region_px(frame, region)
    sw = IC.level_size(w, h, level)[0] + 2 * pad
    for rows in (None, (18, 33)):
        R = NI.region_at(reg0, level, rows)
        for form in ("default", "lds", "scalar"):
            c = IC.Case(frame, "affine", region, "far", form, gridx, "")
            kind = IC.iter_form(frame, level, form)
            nb_h = IC.grid_blocks(reg0, level, gridx, False)
            nb_i = IC.grid_blocks(reg0, level, gridx, kind != "scalar")
            if gridx is not None:
                assert nb_h <= gridx and nb_i <= gridx
            want = (IC.lane_load_brute("scalar", R, pad, sw, nb_h), IC.lane_load_brute(kind, R, pad, sw, nb_i))
            assert IC.lane_load(c, level, rows) == want, (form, rows)
            if gridx is None and rows is None:
                assert max(want) <= 4
    if gridx == 1 and frame == "96x40p16":   # one workgroup: 4 pixels per tile row, 9 tile rows of the 36-row region
        assert IC.lane_load(IC.Case(frame, "affine", region, "far", "default", 1, ""), 0)[1] == 4 * 9


def test_rank_deficient_oracle_solve(oracle):
    """The lstsq solve the GPU module uses as the oracle of the rank-deficient tails: on vertical stripes it leaves the
    unobservable parameters at exactly zero and finds the shift."""
    a, b = IC.stripes_pair()
    h, w = a.shape
    pa, pb = IC.planes_of(oracle, a, b, IC.STRIPES_PAD)
    assert all(not np.asarray(p[2]).any() for p in pa)          # gy == 0 at every level
    tr = []
    M, it = NI.align(pa, pb, IC.STRIPES_PAD, w, h, 0, IC.LV_F, maxiter=6, trace=tr, solve=IC.lstsq)
    assert all(t[4][1] == 0.0 for t in tr) and M[1, 2] == 0.0 and abs(M[0, 2] - 1.5) < 0.02
    M, it = NI.align(pa, pb, IC.STRIPES_PAD, w, h, 2, IC.LV_F, maxiter=6, solve=IC.lstsq)
    assert np.abs(M[1] - [0.0, 1.0, 0.0]).max() < 1e-12 and np.isfinite(M).all() and abs(M[0, 2] - 1.5) < 0.05
    # the device's solver arithmetic (lu_factor_ws<6> / lu_apply_ws<6>, host build) on the affine system of level 0:
    # the free variables are exactly 0 and the rest is the minimum-norm solution
    import invcompcamtrack_amd as ic
    tr = []
    NI.align(pa, pb, IC.STRIPES_PAD, w, h, 2, 0, maxiter=1, trace=tr, solve=IC.lstsq)
    H, rhs = tr[0][2].astype(np.float32), tr[0][3].astype(np.float32)
    assert not H[1::2].any() and not H[:, 1::2].any() and np.linalg.matrix_rank(H[::2, ::2].astype(np.float64)) == 3
    x = ic.solve6(H, rhs)
    ref = IC.lstsq(H.astype(np.float64), rhs.astype(np.float64))
    assert not x[1::2].any() and x[0] != 0 and np.abs(x - ref).max() <= 1e-4 * np.abs(ref).max()
    with pytest.raises(np.linalg.LinAlgError):
        NI.align(pa, pb, IC.STRIPES_PAD, w, h, 0, IC.LV_F, maxiter=1)   # the default solve refuses a singular H
