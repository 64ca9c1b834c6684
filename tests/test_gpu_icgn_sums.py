"""The raw H and b sums of one launch of the alignment engine (csrc/ictr_icgn.hip) against the f64 oracle, at the shapes
where this kernel family can go wrong: pitches that force the scalar form, levels of one run in different forms, the
32-float row start, two tile columns, short last tile rows, odd regions, bands, batches, grids of 1 and 3 workgroups
and warps that push a fifth of the template out of the frame; then end-to-end runs on those shapes and rank-deficient
systems. Gauss-Newton corrects itself, so converged warps cannot see a wrong H entry or a dropped edge column; the sums
can. The bound is icgn_cases' (24 + L) * 2^-24 * majorant, derived there; test_icgn_sums_cpu.py shows that one lost
edge pixel moves the sums by hundreds of times that bound.

Every check prints its ratio |GPU - oracle| / (2^-24 * majorant) next to the bound 24 + L >= 25, and the module ends
with the worst ratio per kernel form (run with -s). An f32 NumPy restatement of the per-pixel arithmetic gives 2.3 for
H and 0.5 for b on this case table ("Raw sums").
"""
import numpy as np
import pytest

import invcompcamtrack_amd as ic
from invcompcamtrack_amd import icgn

import icgn_cases as IC
from test_gpu_icgn import corner_err

pytestmark = pytest.mark.gpu

_pyr = {}
_worst = {}     # kernel form -> worst ratio in units of 2^-24 * majorant


def pyramids(frame, seed=1234):
    key = (frame, seed)
    if key not in _pyr:
        a, b = IC.pair(frame, seed)
        pad = IC.frame_size(frame)[2]
        _pyr[key] = (ic.Pyramid(a, IC.LV_F, pad), ic.Pyramid(b, IC.LV_F, pad, getgrad=False))
    return _pyr[key]


def set_form(monkeypatch, form, gridx):
    for k in ("ICTR_ICGN_LDS", "ICTR_ICGN_SCALAR", "ICTR_ICGN_GRIDX"):
        monkeypatch.delenv(k, raising=False)
    if form == "lds":
        monkeypatch.setenv("ICTR_ICGN_LDS", "1")
    elif form == "scalar":
        monkeypatch.setenv("ICTR_ICGN_SCALAR", "1")
    if gridx is not None:
        monkeypatch.setenv("ICTR_ICGN_GRIDX", str(gridx))


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for form in sorted(_worst):
        print(f"\n[icgn-sums] worst GPU ratio, {form}: {_worst[form]:.2f} x 2^-24 x majorant")


def note(form, ratio):
    _worst[form] = max(_worst.get(form, 0.0), float(ratio))


def one_launch(eng, red, level, nproblems=1):
    """begin, H of one launch, b of one launch at the initial warp, as f64 arrays (B, 36) and (B, 8)."""
    import torch
    eng.begin()
    eng.hess_accumulate(level)
    torch.cuda.synchronize()
    H = red.cpu().numpy().astype(np.float64).reshape(nproblems, icgn.RED_STRIDE)[:, :36].copy()
    eng.hess_finish(level)
    eng.iter_accumulate(level)
    torch.cuda.synchronize()
    rec = red.cpu().numpy().astype(np.float64).reshape(nproblems, icgn.RED_STRIDE)
    assert not rec[:, :36].any()                    # hess_finish consumed and cleared the H part of the record
    b = rec[:, 36:].copy()
    eng.iter_finish(level)
    torch.cuda.synchronize()
    assert not red.cpu().numpy().any()              # iter_finish cleared b
    return H, b


def check(tag, form, H, b, rec, L):
    """|GPU - oracle| <= (24 + L) 2^-24 majorant, entry by entry; entries the model does not have are exactly zero."""
    nh, n = len(rec.H), len(rec.b)
    tolH, tolb = IC.tolerances(rec, *L)
    assert not H[nh:].any() and not b[n:].any(), tag
    eH, eb = np.abs(H[:nh] - rec.H), np.abs(b[:n] - rec.b)
    if rec.npx == 0:
        assert not H.any() and not b.any(), tag     # an empty band's record is exactly zero
        return
    # (a majorant of 0, e.g. ny == 0 on a one-row band, allows no error at all: the assertions below see to that)
    rH = np.divide(eH, IC.EPS24 * rec.majH, out=np.zeros(nh), where=rec.majH > 0).max()
    rb = np.divide(eb, IC.EPS24 * rec.majb, out=np.zeros(n), where=rec.majb > 0).max()
    note("k_icgn_hess", rH)
    note("iter " + form, rb)
    print(f"[icgn-sums] {tag}: H {rH:.2f} of {IC.K_ROUND + L[0]}, b {rb:.2f} of {IC.K_ROUND + L[1]} ({form})")
    assert (eH <= tolH).all(), (tag, "H", rH, IC.K_ROUND + L[0])
    assert (eb <= tolb).all(), (tag, "b", rb, IC.K_ROUND + L[1])


def engine(c, nproblems=1, seeds=(1234,), warps=None):
    import torch
    w, h, _ = IC.frame_size(c.frame)
    eng = icgn.AlignBatch(c.model, w, h, IC.LV_F, 0, 1, 0.0, IC.region_px(c.frame, c.region), nproblems)
    red = torch.zeros(nproblems * icgn.RED_STRIDE, dtype=torch.float32, device="cuda")
    M0 = []
    for k in range(nproblems):
        eng.set_frames(k, *pyramids(c.frame, seeds[k]))
        M0.append(IC.warp_px(c.frame, c.model, warps[k] if warps else c.warp))
        eng.set_warp(k, M0[k])
    eng.enable_sharding(red.data_ptr())
    return eng, red, M0


@pytest.mark.parametrize("c", IC.CASES, ids=IC.case_id)
def test_sums_of_one_launch_match_oracle(oracle, monkeypatch, c):
    set_form(monkeypatch, c.form, c.gridx)
    eng, red, M0 = engine(c)
    reg0 = IC.region_px(c.frame, c.region)
    for l in IC.LEVELS:
        H, b = one_launch(eng, red, l)
        rec = IC.oracle_record(oracle, c.frame, c.model, l, reg0, M0[0])
        check(f"{IC.case_id(c)} level {l}", IC.iter_form(c.frame, l, c.form), H[0], b[0], rec, IC.lane_load(c, l))


@pytest.mark.parametrize("model", IC.MODELS)
@pytest.mark.parametrize("frame,world,form", [("75x51p4", 3, "default"), ("76x52p4", 3, "default"),
                                              ("76x52p4", 5, "default"), ("76x52p4", 5, "lds")])
def test_row_bands(oracle, monkeypatch, frame, world, form, model):
    """Row bands of the default region (set_rows): counts that are no multiple of four, a one-row band, an empty one.
    Each band against NpEngine(rows=...) to its own bound; the bands' sum against the whole-frame record."""
    c = IC.Case(frame, model, "default", "far", form, None, "row bands")
    set_form(monkeypatch, form, None)
    eng, red, M0 = engine(c)
    w, h, _ = IC.frame_size(frame)
    reg0 = IC.region_px(frame, "default")
    bands = icgn.shard_rows(2, h - 2, world)
    for l in IC.LEVELS:
        kind = IC.iter_form(frame, l, form)
        sumH, sumb, tolH, tolb = 0.0, 0.0, 0.0, 0.0
        for rows in bands + [IC.ONE_ROW, IC.EMPTY]:
            eng.set_rows(*rows)
            H, b = one_launch(eng, red, l)
            rec = IC.oracle_record(oracle, frame, model, l, reg0, M0[0], rows=rows)
            L = IC.lane_load(c, l, rows)
            check(f"{frame} {model} rows {rows} level {l}", kind, H[0], b[0], rec, L)
            if rows in bands:
                t = IC.tolerances(rec, *L)
                sumH, sumb, tolH, tolb = sumH + H[0], sumb + b[0], tolH + t[0], tolb + t[1]
        eng.set_rows(0, h)
        H, b = one_launch(eng, red, l)
        whole = IC.oracle_record(oracle, frame, model, l, reg0, M0[0])
        L = IC.lane_load(c, l)
        check(f"{frame} {model} whole level {l}", kind, H[0], b[0], whole, L)
        nh, n = len(whole.H), len(whole.b)
        assert (np.abs(sumH[:nh] - whole.H) <= tolH).all() and (np.abs(sumb[:n] - whole.b) <= tolb).all()
        t = IC.tolerances(whole, *L)
        assert (np.abs(sumH[:nh] - H[0][:nh]) <= tolH + t[0]).all() and (np.abs(sumb[:n] - b[0][:n]) <= tolb + t[1]).all()


@pytest.mark.parametrize("model", IC.MODELS)
@pytest.mark.parametrize("frame,form,gridx", [("76x52p4", "default", None), ("76x52p4", "default", 3),
                                              ("300x20p4", "lds", 3), ("75x51p4", "default", None)])
def test_batch_of_three_different_problems(oracle, monkeypatch, frame, form, gridx, model):
    """B = 3 problems with different frames and warps on one engine, each against its own oracle: catches a wrong
    blockIdx.y / nblk indexing of the partials."""
    c = IC.Case(frame, model, "odd", None, form, gridx, "batch")
    set_form(monkeypatch, form, gridx)
    eng, red, M0 = engine(c, 3, IC.BATCH_SEEDS, IC.BATCH_WARPS)
    reg0 = IC.region_px(frame, "odd")
    for l in IC.LEVELS:
        H, b = one_launch(eng, red, l, 3)
        recs = [IC.oracle_record(oracle, frame, model, l, reg0, M0[k], seed=IC.BATCH_SEEDS[k]) for k in range(3)]
        assert np.abs(recs[0].H - recs[1].H).max() > 1e-3 * np.abs(recs[0].H).max()      # the problems do differ
        for k in range(3):
            check(f"{frame} {model} batch {k} level {l}", IC.iter_form(frame, l, form), H[k], b[k], recs[k],
                  IC.lane_load(c, l, nproblems=3))


# ---------------------------------------------------------------- end to end where it has never run
@pytest.mark.parametrize("model", IC.MODELS)
@pytest.mark.parametrize("frame", ["76x52p4", "75x51p4"])
def test_end_to_end_on_mixed_forms_and_with_a_last_level(oracle, frame, model):
    """run_async against the oracle's align on frames whose levels take different forms (76x52) or only the scalar
    form (75x51), down to level 0 and down to level 1 only."""
    from oracle import np_icgn as NI
    w, h, pad = IC.frame_size(frame)
    ga, gb = pyramids(frame)
    pa, pb = IC.oracle_planes(oracle, frame)
    out = {}
    for lv_l in (0, 1):
        eng = icgn.AlignBatch(model, w, h, IC.LV_F, lv_l, 8, 0.0, None, 1)
        eng.set_frames(0, ga, gb)
        eng.run_async()
        M, it, _ = eng.results()
        Mo, ito = NI.align(pa, pb, pad, w, h, IC.MODEL_ID[model], IC.LV_F, lv_l, maxiter=8)
        err = corner_err(M[0], Mo, w, h)
        print(f"[icgn-e2e] {frame} {model} lv_l={lv_l}: corner error vs oracle {err:.2e} px, {it[0]} iterations")
        assert it[0] == ito == 8 * (IC.LV_F + 1 - lv_l)
        assert err < 2e-3
        out[lv_l] = M[0]
    assert not np.array_equal(out[0], out[1])


# ---------------------------------------------------------------- rank-deficient systems
def _stripes_engine(model, maxiter, b=None, M0=None):
    a, cur = IC.stripes_pair()
    cur = cur if b is None else b
    ga = ic.Pyramid(a, IC.LV_F, IC.STRIPES_PAD)
    gb = ic.Pyramid(cur, IC.LV_F, IC.STRIPES_PAD, getgrad=False)
    eng = icgn.AlignBatch(model, IC.STRIPES_W, IC.STRIPES_H, IC.LV_F, 0, maxiter, 0.0, None, 1)
    eng.set_frames(0, ga, gb)
    if M0 is not None:
        eng.set_warp(0, M0)
    return eng, a, cur


def _phase_run(eng, maxiter):
    """The sharded loop on one rank, reading dp after every iteration; returns the list of dp."""
    import torch
    red = torch.zeros(icgn.RED_STRIDE, dtype=torch.float32, device="cuda")
    eng.enable_sharding(red.data_ptr())
    dps = []
    eng.begin()
    for l in range(IC.LV_F, -1, -1):
        eng.hess_accumulate(l)
        eng.hess_finish(l)
        for _ in range(maxiter):
            eng.iter_accumulate(l)
            eng.iter_finish(l)
            dps.append(eng.results()[2][0].copy())
    return dps


def test_rank_deficient_translation_on_stripes(oracle):
    """Vertical stripes: gy == 0, H = [[sum gx^2, 0], [0, 0]]. Both tails take the rank-deficient branch: the free
    parameter stays exactly 0 at every iteration, in the one-launch-chain form and in the phase form."""
    from oracle import np_icgn as NI
    maxiter = 6
    eng, a, cur = _stripes_engine("translation", maxiter)
    eng.run_async()
    M, it, dp = eng.results()
    assert np.isfinite(M).all() and np.isfinite(dp).all()
    assert dp[0][1] == 0.0 and M[0][1, 2] == 0.0
    assert abs(M[0][0, 2] - IC.STRIPES_SHIFT) < 0.02
    eng2, _, _ = _stripes_engine("translation", maxiter)
    dps = _phase_run(eng2, maxiter)
    assert len(dps) == maxiter * (IC.LV_F + 1) and all(np.isfinite(d).all() and d[1] == 0.0 for d in dps)
    assert any(d[0] != 0.0 for d in dps)
    assert np.array_equal(eng2.results()[0], M)      # one band: the phase form sees the same floats
    pa, pb = IC.planes_of(oracle, a, cur, IC.STRIPES_PAD)
    Mo, _ = NI.align(pa, pb, IC.STRIPES_PAD, IC.STRIPES_W, IC.STRIPES_H, 0, IC.LV_F, maxiter=maxiter, solve=IC.lstsq)
    assert corner_err(M[0], Mo, IC.STRIPES_W, IC.STRIPES_H) < 2e-3


def test_rank_deficient_affine_on_stripes(oracle):
    """H has zero rows and columns 1, 3, 5 (rank 3): the second row of the warp stays exactly (0, 1, 0), the first row
    agrees with the minimum-norm oracle."""
    from oracle import np_icgn as NI
    maxiter = 6
    eng, a, cur = _stripes_engine("affine", maxiter)
    eng.run_async()
    M, it, dp = eng.results()
    assert np.isfinite(M).all() and np.isfinite(dp).all()
    assert np.array_equal(M[0][1], [0.0, 1.0, 0.0]) and np.array_equal(M[0][2], [0.0, 0.0, 1.0])
    assert dp[0][1] == dp[0][3] == dp[0][5] == 0.0
    pa, pb = IC.planes_of(oracle, a, cur, IC.STRIPES_PAD)
    Mo, _ = NI.align(pa, pb, IC.STRIPES_PAD, IC.STRIPES_W, IC.STRIPES_H, 2, IC.LV_F, maxiter=maxiter, solve=IC.lstsq)
    print(f"[icgn-rank] affine on stripes: first row GPU {M[0][0]}, oracle {Mo[0]}")
    assert corner_err(M[0], Mo, IC.STRIPES_W, IC.STRIPES_H) < 2e-3


@pytest.mark.parametrize("model", IC.MODELS)
def test_constant_template_leaves_the_warp_alone(model):
    """H == 0 and b == 0 whatever the current frame holds: dp == 0, one iteration per level, the warp keeps its bits."""
    _, cur = IC.pair("76x52p4")
    M0 = np.array([[1.0, 0.0, 0.75], [0.0, 1.0, -1.25], [0.0, 0.0, 1.0]])
    a = np.full((IC.STRIPES_H, IC.STRIPES_W), 100.0, np.float32)
    cur = np.ascontiguousarray(cur[:IC.STRIPES_H, :IC.STRIPES_W])
    ga = ic.Pyramid(a, IC.LV_F, IC.STRIPES_PAD)
    gb = ic.Pyramid(cur, IC.LV_F, IC.STRIPES_PAD, getgrad=False)
    eng = icgn.AlignBatch(model, IC.STRIPES_W, IC.STRIPES_H, IC.LV_F, 0, 5, 0.0, None, 1)
    eng.set_frames(0, ga, gb)
    eng.set_warp(0, M0)
    eng.begin()
    Mstart = eng.results()[0].copy()
    assert np.abs(Mstart[0] - M0).max() < 1e-6
    eng.run_async()
    M, it, dp = eng.results()
    assert np.array_equal(M, Mstart)
    assert not dp.any()
    assert it[0] == IC.LV_F + 1
