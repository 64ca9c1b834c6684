"""Variational refinement without a GPU: the definition (patchflow.refine_flow_host), the f32 restatement of the kernels
(flowrefine_f32.py) against it over the case table, the injectable defects, and the usefulness bars.

Every figure that flowrefine_cases.py records is measured again here and printed; a figure above its record fails. The
edge-shape table (flowrefine_cases.EDGE) and the weights off their defaults (PARAMS) have records of their own, and the
condition under which EDGE leaves no pixel out is checked here."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import flowrefine_cases as FC
import flowrefine_f32 as R
from invcompcamtrack_amd import patchflow as pf


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):  # the "dense" inputs are tracked by the host oracle
    return oracle


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- the definition
@pytest.mark.parametrize("frame", FC.FRAMES)
@pytest.mark.parametrize("x_only", (False, True))
def test_host_identity_returns_zeros(frame, x_only):
    a, _ = FC.pair(frame)
    out = pf.refine_flow_host(a, a, np.zeros(a.shape + (2,), np.float32), x_only=x_only)
    assert out.dtype == np.float32 and not out.any()


@pytest.mark.parametrize("frame,kind", FC.TABLE)
def test_host_n_outer_0_and_x_only_keep_bits(frame, kind):
    a, b = FC.pair(frame)
    f = FC.f0(frame, kind)
    assert np.array_equal(_bits(pf.refine_flow_host(a, b, f, n_outer=0)), _bits(f))
    out = pf.refine_flow_host(a, b, f, x_only=True)
    assert np.array_equal(_bits(out[..., 1]), _bits(f[..., 1]))
    assert not np.array_equal(out[..., 0], f[..., 0])


def test_host_keeps_special_bits_of_v():
    a, b = FC.pair("67x53")
    f = FC.f0("67x53", "smooth").copy()
    f[3, 4, 1], f[5, 6, 1], f[7, 8, 1] = -0.0, np.float32(1e-42), np.float32(-3.25)  # -0, a subnormal
    assert np.array_equal(_bits(pf.refine_flow_host(a, b, f, x_only=True)[..., 1]), _bits(f[..., 1]))
    assert np.array_equal(_bits(pf.refine_flow_host(a, b, f, n_outer=0)), _bits(f))


def test_host_refuses():
    a, b = FC.pair("67x53")
    f = FC.f0("67x53", "smooth")
    with pytest.raises(ValueError):
        pf.refine_flow_host(a, b, f, omega=2.0)
    with pytest.raises(ValueError):
        pf.refine_flow_host(a, b, f, alpha=-1.0)
    with pytest.raises(ValueError, match="alpha"):  # no coupling, and 0 / 0 at every pixel without data
        pf.refine_flow_host(a, b, f, alpha=0.0)
    assert np.isfinite(pf.refine_flow_host(a, b, f, n_outer=1, gamma=0.0, delta=0.0)).all()  # these stay legal
    from oracle import oracle as O
    pa, pb = O.Pyramid(a, 1, 8), O.Pyramid(b, 1, 8)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="alpha"):  # refused before the first level is searched
            pf.c2f_flow_host(pa, pb, lv_f=1, refine=dict(alpha=bad))


def test_alpha_0_was_0_by_0():
    """What the refusal is for: with alpha = 0 a pixel without data (outside: w0 = wg = 0) has a11 + sw = 0."""
    frame, kind = "edge-33x18", "edge"
    a, b = FC.pair(frame)
    f = FC.f0(frame, kind)
    h, w = a.shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    bw, inside = pf._fr_warp(b.astype(np.float64), xx + f[..., 0], yy + f[..., 1])
    a11, _, _, _, _, wr, wd = pf._fr_coef(a.astype(np.float64), bw, inside, f[..., 0].astype(np.float64),
                                          f[..., 1].astype(np.float64), 0.0, 13.0, 4.5)
    assert (inside == 0).any() and not wr.any() and not wd.any() and not a11[inside == 0].any()
    with pytest.raises(ValueError):
        pf.refine_flow_host(a, b, f[:-1])
    with pytest.raises(ValueError):
        pf.refine_flow_host(a[:3, :3], b[:3, :3], f[:3, :3])


def test_host_flow_that_leaves_the_frame_stays_finite():
    """Positions far outside, and a NaN: no index depends on them; the NaN stays where the rule carries it."""
    a, b = FC.pair("67x53")
    f = FC.f0("67x53", "smooth").copy()
    f[:6] += 400.0
    f[-6:] -= 1e6
    out = pf.refine_flow_host(a, b, f, n_outer=2)
    assert np.isfinite(out).all()
    f[20, 20, 0] = np.nan
    assert np.isnan(pf.refine_flow_host(a, b, f, n_outer=1)[20, 20, 0])
    assert np.isnan(R.refine(a, b, f, n_outer=1)[20, 20, 0])


# ---------------------------------------------------------------- the restatement against the definition
@functools.lru_cache(maxsize=None)
def _restated_stage(frame, kind, x_only, defect=None):
    a, b = FC.pair(frame)
    tr = []
    R.refine(a, b, FC.f0(frame, kind), n_outer=FC.STAGE_RUN[0], n_sor=FC.STAGE_RUN[1], omega=FC.STAGE_RUN[2],
             x_only=x_only, defect=defect, trace=tr)
    return tr[0]


def _restated_sweep(frame, kind, colour, x_only, defect=None):
    p = {k: v.copy() for k, v in FC.sweep_inputs(frame, kind).items()}
    R.half_sweep(colour, 1.6, x_only, p["u"], p["v"], p["du"], p["dv"], *[p[k] for k in FC.COEF_PLANES], defect=defect)
    return p["du"], p["dv"]


def test_restatement_warp_within_the_derived_bound():
    for frame, kind in FC.TABLE:
        err, bound = FC.warp_error(frame, kind, _restated_stage(frame, kind, False)["bw"])
        print(f"warp {frame} {kind}: {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (frame, kind)


def test_restatement_stage_differences_are_within_their_records():
    worst = {}
    for frame, kind in FC.TABLE:
        for x_only in (False, True):
            t = _restated_stage(frame, kind, x_only)
            planes = {k: t[k] for k in FC.STAGE_DIFF if k != "sweep"}
            for k, e in FC.stage_errors(frame, kind, x_only, planes).items():
                worst[k] = max(worst.get(k, 0.0), e)
            for colour in (0, 1):
                e = FC.sweep_error(frame, kind, colour, x_only, *_restated_sweep(frame, kind, colour, x_only))
                worst["sweep"] = max(worst.get("sweep", 0.0), e)
            assert np.array_equal(_bits(t["u"]), _bits(FC.f0(frame, kind)[..., 0]))
    print("stage differences:", {k: float(f"{v:.3g}") for k, v in worst.items()})
    for k, rec in FC.STAGE_DIFF.items():
        assert worst[k] <= rec, (k, worst[k], rec)
        assert worst[k] >= rec / 2, (k, "the record is stale", worst[k], rec)


@pytest.mark.parametrize("run", FC.RUNS)
@pytest.mark.parametrize("x_only", (False, True))
def test_restatement_full_run_differences_are_within_their_records(run, x_only):
    worst = 0.0
    for frame, kind in FC.TABLE:
        a, b = FC.pair(frame)
        got = R.refine(a, b, FC.f0(frame, kind), n_outer=run[0], n_sor=run[1], omega=run[2], x_only=x_only)
        worst = max(worst, FC.full_error(frame, kind, *run, x_only, got))
        if x_only:
            assert np.array_equal(_bits(got[..., 1]), _bits(FC.f0(frame, kind)[..., 1]))
    rec = FC.FULL_DIFF[run + (x_only,)]
    print(f"full run {run} x_only={x_only}: {worst:.3e} (record {rec:.3e})")
    assert worst <= rec
    assert worst >= rec / 2, "the record is stale"


def test_restatement_exact_cases():
    a, b = FC.pair("100x77")
    f = FC.f0("100x77", "dense")
    assert not R.refine(a, a, np.zeros_like(f)).any()
    assert np.array_equal(_bits(R.refine(a, b, f, n_outer=0)), _bits(f))


# ---------------------------------------------------------------- every injectable defect is seen
DEFECT_CASES = (("100x77", "dense"), ("67x53", "smooth"))


def _checks(defect):
    """{check: passed} of the checks that the GPU module applies to the device, applied to the restatement."""
    out = {}
    for frame, kind in DEFECT_CASES:
        t = _restated_stage(frame, kind, False, defect)
        err, bound = FC.warp_error(frame, kind, t["bw"])
        out[f"warp {frame}"] = err <= bound
        errs = FC.stage_errors(frame, kind, False, {k: t[k] for k in FC.STAGE_DIFF if k != "sweep"})
        out[f"coef {frame}"] = all(errs[k] <= FC.MARGIN * FC.STAGE_DIFF[k] for k in FC.COEF_PLANES)
        out[f"du dv {frame}"] = all(errs[k] <= FC.MARGIN * FC.STAGE_DIFF[k] for k in ("du", "dv"))
        out[f"sweep {frame}"] = all(
            FC.sweep_error(frame, kind, c, False, *_restated_sweep(frame, kind, c, False, defect))
            <= FC.MARGIN * FC.STAGE_DIFF["sweep"] for c in (0, 1))
        a, b = FC.pair(frame)
        run = FC.RUNS[1]
        got = R.refine(a, b, FC.f0(frame, kind), n_outer=run[0], n_sor=run[1], omega=run[2], defect=defect)
        out[f"full {frame}"] = FC.full_error(frame, kind, *run, False, got) <= FC.MARGIN * FC.FULL_DIFF[run + (False,)]
    return out


def test_the_checks_pass_without_a_defect():
    res = _checks(None)
    assert all(res.values()), res


@pytest.mark.parametrize("defect", R.DEFECTS[:6])
def test_each_defect_is_seen(defect):
    res = _checks(defect)
    seen = sorted(k for k, ok in res.items() if not ok)
    print(defect, "seen by", seen)
    assert seen, (defect, "no check sees it")


@pytest.mark.parametrize("defect", R.DEFECTS[6:])
def test_a_defect_within_the_tolerances_changes_bits(defect):
    """"fused" and "border2": which of the tolerance checks see them is printed (DESIGN.md states the outcome); whatever
    they do, the defective restatement's stage planes differ in bits from the clean one's on the table and on EDGE."""
    seen = sorted(k for k, ok in _checks(defect).items() if not ok)
    print(defect, "seen by the tolerance checks:", seen or "none")
    differ = {}
    for name, cases in (("TABLE", DEFECT_CASES), ("EDGE", FC.EDGE)):
        differ[name] = []
        for frame, kind in cases:
            bad = _restated_stage(frame, kind, False, defect)
            good = FC.restated(frame, kind, *FC.STAGE_RUN, False)[1][0]
            planes = [k for k in R.STAGES if not np.array_equal(_bits(bad[k]), _bits(good[k]))]
            if planes:
                differ[name].append((frame, planes))
        print(defect, name, "bits differ on", len(differ[name]), "of", len(cases), differ[name])
    assert differ["TABLE"] and differ["EDGE"]


# ---------------------------------------------------------------- the edge-shape table
@pytest.mark.parametrize("frame,kind", FC.EDGE)
def test_edge_entries_meet_their_condition(frame, kind):
    """Part of F0 is outside on at least two sides, and no warped position of the definition comes near the inside
    boundary in any outer iteration of any run that a test uses: nothing is left out on these frames."""
    f = FC.f0(frame, kind)
    h, w = f.shape[:2]
    assert (np.arange(w) + f[0, :, 0] >= 0).any() and (f[0, :, 1] < 0).all()  # the first row is above the frame
    assert (np.arange(h) + f[:, -1, 1] >= 0).any() and (f[:, -1, 0] > 0).all()  # the last column right of it
    share = FC.outside_share(frame, kind)
    print(f"{frame}: {100 * share:.1f} % of F0 outside, pyramids padded by psz + {FC.pad_extra(frame)}")
    assert FC.EDGE_OUTSIDE[0] <= share <= FC.EDGE_OUTSIDE[1]
    for n_outer, n_sor, omega, x_only, weights in FC.edge_runs(frame, kind):
        out, tr, near = FC.host_run(frame, kind, n_outer, n_sor, omega, x_only, weights)
        assert len(tr) == n_outer and not near.any(), (n_outer, n_sor, omega, x_only, weights, int(near.sum()))
        assert np.isfinite(out).all()
    assert sorted({FC.pad_extra(fr) for fr, _ in FC.EDGE}) == [0, 1, 5]


def test_restatement_edge_stage_differences_are_within_their_records():
    worst = {}
    for frame, kind in FC.EDGE:
        for x_only in (False, True):
            t = FC.restated(frame, kind, *FC.STAGE_RUN, x_only)[1][0]
            planes = {k: t[k] for k in FC.EDGE_STAGE_DIFF if k != "sweep"}
            for k, e in FC.stage_errors(frame, kind, x_only, planes).items():
                worst[k] = max(worst.get(k, (0.0, None)), (e, frame))
            for colour in (0, 1):
                e = FC.sweep_error(frame, kind, colour, x_only, *_restated_sweep(frame, kind, colour, x_only))
                worst["sweep"] = max(worst.get("sweep", (0.0, None)), (e, frame))
            assert np.array_equal(_bits(t["u"]), _bits(FC.f0(frame, kind)[..., 0]))
            assert np.array_equal(_bits(t["v"]), _bits(FC.f0(frame, kind)[..., 1]))
    print("edge stage differences:", {k: (float(f"{v[0]:.3g}"), v[1]) for k, v in worst.items()})
    for k, rec in FC.EDGE_STAGE_DIFF.items():
        assert worst[k][0] <= rec, (k, worst[k], rec)
        assert worst[k][0] >= rec / 2, (k, "the record is stale", worst[k], rec)


def test_restatement_edge_warp_within_the_derived_bound():
    for frame, kind in FC.EDGE:
        err, bound = FC.warp_error(frame, kind, FC.restated(frame, kind, *FC.STAGE_RUN, False)[1][0]["bw"])
        print(f"warp {frame}: {err:.3e} (bound {bound:.3e})")
        assert err <= bound, frame


@pytest.mark.parametrize("run", FC.EDGE_RUNS)
@pytest.mark.parametrize("x_only", (False, True))
def test_restatement_edge_full_run_differences_are_within_their_records(run, x_only):
    worst = (0.0, None)
    for frame, kind in FC.EDGE:
        got = FC.restated(frame, kind, *run, x_only)[0]
        worst = max(worst, (FC.full_error(frame, kind, *run, x_only, got), frame))
        if x_only:
            assert np.array_equal(_bits(got[..., 1]), _bits(FC.f0(frame, kind)[..., 1]))
    rec = FC.EDGE_FULL_DIFF[run + (x_only,)]
    print(f"edge full run {run} x_only={x_only}: {worst[0]:.3e} at {worst[1]} (record {rec:.3e})")
    assert worst[0] <= rec
    assert worst[0] >= rec / 2, "the record is stale"


@pytest.mark.parametrize("params", FC.PARAMS)
def test_restatement_differences_at_other_weights_are_within_their_records(params):
    """alpha, gamma, delta, omega off their defaults (gamma = 0: wg = 0; delta = 0: w0 = 0; both: a11 = a12 = a22 = 0)."""
    worst = (0.0, None)
    run = (3, 5, params[3])
    for frame, kind in FC.PARAM_CASES:
        for x_only in (False, True):
            got, tr = FC.restated(frame, kind, *run, x_only, params[:3])
            assert np.isfinite(got).all()
            worst = max(worst, (FC.full_error(frame, kind, *run, x_only, got, params[:3]), frame, x_only))
            if params[1] == 0 and params[2] == 0:
                assert not any(t[k].any() for t in tr for k in ("a11", "a12", "a22", "b1", "b2"))
            else:
                assert all(t["a11"].any() for t in tr)
    rec = FC.PARAM_DIFF[params]
    print(f"weights {params}: {worst[0]:.3e} at {worst[1:]} (record {rec:.3e})")
    assert worst[0] <= rec
    assert worst[0] >= rec / 2, "the record is stale"


@pytest.mark.parametrize("frame,kind", (("67x53", "smooth"), ("edge-18x33", "edge")))
def test_restatement_and_definition_carry_a_nan_alike(frame, kind):
    """The far field stays finite in both; a NaN at one pixel of it is a NaN at the same pixels of both results after
    (1, 5, 1.6): the device is compared with the restatement there, so the restatement has to be right about it."""
    a, b = FC.pair(frame)
    f = FC.far_field(frame, kind)
    assert np.isfinite(pf.refine_flow_host(a, b, f, n_outer=3)).all()
    assert np.isfinite(R.refine(a, b, f, n_outer=3)).all()
    f[FC.NAN_AT[1], FC.NAN_AT[0], 0] = np.nan
    for x_only in (False, True):
        want = np.isnan(pf.refine_flow_host(a, b, f, n_outer=1, x_only=x_only))
        got = np.isnan(R.refine(a, b, f, n_outer=1, x_only=x_only))
        print(frame, x_only, int(want.sum()), "NaN floats")
        assert want[FC.NAN_AT[1], FC.NAN_AT[0], 0] and not want.all()
        assert np.array_equal(got, want)


# ---------------------------------------------------------------- usefulness, on the definition alone
@pytest.mark.parametrize("kind", sorted(FC.USEFUL))
def test_host_usefulness(kind):
    n_outer, ratio = FC.USEFUL[kind]
    worst = 0.0
    for seed in FC.SEEDS:
        a, b, f, truth, mask = FC.scene(kind, seed)
        out = pf.refine_flow_host(a, b, f, n_outer=n_outer)
        before, after = FC.epe(f, truth, mask), FC.epe(out, truth, mask)
        print(f"{kind} seed {seed}: {before:.4f} -> {after:.4f} px ({after / before:.3f}), bar {FC.useful_bar(kind):.3f}")
        assert after <= FC.useful_bar(kind) * before
        worst = max(worst, after / before)
    assert ratio - 0.01 <= worst <= ratio, ("the recorded ratio is not the measured one", worst, ratio)
