"""Variational refinement without a GPU: the definition (patchflow.refine_flow_host), the f32 restatement of the kernels
(flowrefine_f32.py) against it over the case table, the injectable defects, and the usefulness bars.

Every figure that flowrefine_cases.py records is measured again here and printed; a figure above its record fails."""
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


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_each_defect_is_seen(defect):
    res = _checks(defect)
    seen = sorted(k for k, ok in res.items() if not ok)
    print(defect, "seen by", seen)
    assert seen, (defect, "no check sees it")


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
