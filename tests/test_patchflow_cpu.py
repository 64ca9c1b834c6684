"""The patch-flow oracle (oracle/np_patchflow.py) and the case table (patchflow_cases.py) on the CPU: an f32 restatement
of the kernel in each launch form's summation shape stays inside one_step's derived bound, six injected defects each leave
it, every decision of the oracle over the table has the margin that lets the GPU module demand equal status and iters,
the padding of the pyramid does not move a result, and the final rescale is 2^lv_l."""
import numpy as np
import pytest

import patchflow_cases as PC
import patchflow_f32 as F32
from oracle import np_patchflow as NP

GROUPS = (0, 1, 2)


@pytest.fixture(scope="module")
def O(oracle):
    return oracle


def _shape(job):
    f = PC.form(job)
    return f // 10, f % 10


def _restate(O, job, shape="form", defect=None):
    pa, pb = PC.oracle_pyramids(O, job.frame, job.pad)
    return F32.track_points(pa, pb, job.pts, job.psz, job.lv_f, job.lv_l, job.maxiter, PC.EPS, PC.MIN_DET,
                            shape=_shape(job) if shape == "form" else shape, defect=defect)


def test_dispatch_table_matches_the_launcher():
    """GROUP_FORM is launch_patchflow's choice (restated in np_patchflow.form_of), every form is in the table, and the
    boundary sizes sit where the issue of this table says: 8 -> 1 pixel per lane, 9 -> first with 2, 16 -> exactly 4,
    17 -> first two-wave size, 32 -> every lane full."""
    for g in GROUPS:
        for psz, f in PC.GROUP_FORM[g].items():
            npl, wpp = NP.form_of(psz, g)
            assert npl * 10 + wpp == f, (g, psz)
            assert NP.lane_pixels(psz, wpp) <= npl
    assert {f for g in GROUPS for f in PC.GROUP_FORM[g].values()} == {11, 41, 161, 82}
    assert [NP.lane_pixels(p, 1) for p in (8, 9, 16, 17, 32)] == [1, 2, 4, 5, 16]
    assert NP.lane_pixels(32, 2) == 8 and NP.lane_pixels(17, 2) == 3 and NP.lane_pixels(8, 2) == 1


def test_oracle_sampling_is_np_oracle_patches(O):
    """np_patchflow._sample (slices) against np_oracle.patches (gathers), which defines the sampling: the same bits, on
    a plane padded by psz and through the view of a plane padded by more."""
    from oracle import np_oracle as N
    for frame in PC.SIZES:
        pts = np.concatenate([PC.interior(frame), PC.special(frame)[:3]])
        for psz, pad in ((1, 1), (8, 8), (15, 20), (32, 33)):
            pa, _ = PC.oracle_pyramids(O, frame, pad)
            ref_pyr, _ = PC.oracle_pyramids(O, frame, psz)
            for plane, ref_plane in ((pa.img[0], ref_pyr.img[0]), (pa.dy[0], ref_pyr.dy[0])):
                want = N.patches(ref_plane, pts[:, 0].copy(), pts[:, 1].copy(), psz)
                for k, (x, y) in enumerate(pts):
                    got, maj = NP._sample(plane, x, y, psz, pad)
                    assert np.array_equal(got, want[k].astype(np.float64)), (frame, psz, pad, k)
                    assert np.all(maj >= np.abs(got) * (1 - 1e-6))


def test_interior_points_are_well_conditioned(O):
    """det > 0.01 tr^2 for every interior point, patch size above 1 and level: a condition on the inputs."""
    for frame in PC.SIZES:
        pa, pb = PC.oracle_pyramids(O, frame, 32)
        for psz in sorted({p for g in GROUPS for p in PC.GROUP_PSZ[g]} - {1}):
            for l in range(PC.LV + 1):
                _, _, cond = NP.one_step(pa, pb, PC.interior(frame), psz, l, 1)
                assert np.all(cond > PC.INTERIOR_COND), ("pick another seed", frame, psz, l, cond.min())


@pytest.mark.parametrize("group", GROUPS)
def test_restatement_stays_within_the_one_step_bound(O, group):
    """Every 'step' job: the kernel's arithmetic in f32, in the form's summation shape and as one serial sum, against
    the f64 step. The worst ratios are printed (-s) and recorded in DESIGN.md."""
    worst = {}
    for job in PC.jobs(group).values():
        if job.kind != "step":
            continue
        for shape in ("form", None):
            new, ok, it = _restate(O, job, shape)
            r = PC.compare_step(job, new, ok, it, O)
            key = (PC.form(job), "form" if shape else "serial")
            worst[key] = max(worst.get(key, 0.0), r)
    print("one-step restatement / bound:", worst)
    assert worst and max(worst.values()) <= 1.0


@pytest.mark.parametrize("group", GROUPS)
def test_margins_hold_and_full_runs_stay_within_the_factor(O, group):
    """Every job that runs to convergence: the oracle's decisions have their margins (check_margins inside compare_full),
    the restatement takes the same decisions, and its final positions are within FULL_FACTOR of bound-sum + u |new|."""
    worst = {}
    for job in PC.jobs(group).values():
        if job.kind not in ("full", "pad"):
            continue
        new, ok, it = _restate(O, job)
        r = PC.compare_full(job, new, ok, it, O)
        worst[PC.form(job)] = max(worst.get(PC.form(job), 0.0), r)
    print("full-run restatement / (bound sum + u |new|):", worst)
    assert max(worst.values()) <= PC.FULL_FACTOR


@pytest.mark.parametrize("group", GROUPS)
def test_status_cases(O, group):
    """Textureless frames are lost exactly (tr = 0, or hyy = hxy = 0), psz 1 is lost everywhere, maxiter = 0 returns the
    input; the leaving points do leave."""
    for job in PC.jobs(group).values():
        if job.kind == "lost":
            pa, pb = PC.oracle_pyramids(O, job.frame, job.pad)
            _, _, cond = NP.one_step(pa, pb, job.pts, job.psz, job.lv_f, 1)
            if job.frame.startswith("flat"):
                assert np.isnan(cond).all(), job.key           # tr == 0: no ratio
            else:
                assert np.all(cond == 0.0), job.key            # det == 0 exactly
            new, ok, it, _ = PC.oracle_full(O, job)
            assert not ok.any() and np.all(it == 0) and np.isnan(new).all(), job.key
            new, ok, it = _restate(O, job)
            assert not ok.any() and np.all(it == 0), job.key
        elif job.kind == "maxiter0":
            new, ok, it, _ = PC.oracle_full(O, job)
            n = PC.N_INTERIOR
            assert ok[:n].all() and np.array_equal(new[ok], job.pts[ok]) and np.all(it == 0), job.key
            assert ok[n] and not ok[-6:].any(), job.key   # the corner (0, 0) lives, the last six are lost
        elif job.key.split("-")[1] == "leave" and job.psz > 1:
            new, ok, it, det = PC.oracle_full(O, job)
            assert (~ok & (it > 0)).sum() >= 3, (job.key, ok, it)   # lost after iterating: they left the view
        elif job.psz == 1 and job.kind == "full":
            _, ok, it, _ = PC.oracle_full(O, job)
            assert not ok.any() and np.all(it == 0), job.key


# ---------------------------------------------------------------- injected defects
DEFECT_JOBS = {  # defect -> (group, key of a 'step' job); "half of P-1" needs an even P, "omit second wave" two waves
    "drop last column": (0, "g0-step-100x77-p15-l0"),
    "drop last row": (0, "g0-step-100x77-p15-l0"),
    "swap w1 w2": (0, "g0-step-100x77-p15-l0"),
    "half of P-1": (0, "g0-step-100x77-p16-l0"),
    "omit second wave": (0, "g0-step-100x77-p31-l0"),
}


@pytest.mark.parametrize("defect", sorted(DEFECT_JOBS))
def test_injected_defect_exceeds_the_bound(O, defect):
    group, key = DEFECT_JOBS[defect]
    job = PC.jobs(group)[key]
    new, ok, it = _restate(O, job, defect=defect)
    step, bound, _ = PC.oracle_step(O, job)
    live = np.isfinite(step[:, 0]) & ok
    live[PC.N_INTERIOR:] = False
    assert live[:PC.N_INTERIOR].all()
    if defect == "swap w1 w2":
        live[:2] = False          # integer and half-pixel coordinates: w1 == w2, nothing to swap
    got = (new[live].astype(np.float64) - job.pts[live]) / 2.0 ** job.lv_f
    tol = bound[live] + PC.U * np.abs(new[live].astype(np.float64)) / 2.0 ** job.lv_f
    ratio = (np.abs(got - step[live]) / tol).max(axis=1)
    print(f"defect {defect!r}: error / bound per interior point, smallest {ratio.min():.1f}, largest {ratio.max():.1f}")
    assert np.all(ratio > 1.0), (defect, ratio)


def test_injected_rescale_defect_exceeds_the_tolerance(O):
    """The final rescale taken from lv_f instead of lv_l, on the (2, 1) range."""
    job = PC.jobs(0)["g0-full-100x77-p15-21"]
    new, ok, it = _restate(O, job, defect="rescale by lv_f")
    new_o, ok_o, _, det = PC.oracle_full(O, job)
    live = ok_o.copy()
    live[PC.N_INTERIOR:] = False
    assert np.array_equal(ok, ok_o) and live.sum() == PC.N_INTERIOR
    err = np.abs(new[live].astype(np.float64) - new_o[live]).max(axis=1)
    ratio = err / PC.full_tolerance(new_o, det)[live]
    print(f"defect 'rescale by lv_f': error / tolerance per interior point, smallest {ratio.min():.1f}")
    assert np.all(ratio > 1.0), ratio


# ---------------------------------------------------------------- padding, final rescale
@pytest.mark.parametrize("group", GROUPS)
def test_padding_does_not_move_the_result(O, group):
    """pad = psz, psz + 1, psz + 5: the same patches, hence the same bits."""
    for psz in PC.GROUP_FORM_PSZ[group]:
        ref = PC.oracle_full(O, PC.jobs(group)[f"g{group}-pad0-p{psz}"])
        assert ref[1].all()
        for extra in PC.PAD_EXTRA[1:]:
            got = PC.oracle_full(O, PC.jobs(group)[f"g{group}-pad{extra}-p{psz}"])
            for a, b in zip(ref[:3], got[:3]):
                assert np.array_equal(a, b), (psz, extra, np.abs(a.astype(float) - b).max())
            new, ok, it = _restate(O, PC.jobs(group)[f"g{group}-pad{extra}-p{psz}"])
            ref32 = _restate(O, PC.jobs(group)[f"g{group}-pad0-p{psz}"])
            assert np.array_equal(new, ref32[0]) and np.array_equal(it, ref32[2])


def test_lv_l_1_equals_the_hand_rolled_sequence(O):
    """track_points(lv_f=2, lv_l=1) = level 2, p * 2, level 1, then exactly * 2 back to level-0 pixels."""
    psz, f32 = 15, np.float32
    pa, pb = PC.oracle_pyramids(O, "100x77", psz)
    pts = PC.interior("100x77")
    new, ok, it = NP.track_points(pa, pb, pts, psz, 2, 1, PC.MAXITER, PC.EPS)
    assert ok.all()
    for k, (x0, y0) in enumerate(pts):
        p = np.zeros(2, f32)
        n = 0
        for l in (2, 1):
            p = p * f32(2) if l == 1 else p
            xl, yl = f32(x0 * f32(0.5 ** l)), f32(y0 * f32(0.5 ** l))
            t = NP._Template(pa, l, xl, yl, psz, 1)
            for _ in range(PC.MAXITER):
                (dx, dy), _ = t.step(pb.img[l], pb.pad, f32(xl + p[0]), f32(yl + p[1]), psz)
                p = (p + np.array([dx, dy])).astype(f32)
                n += 1
                if dx * dx + dy * dy < PC.EPS ** 2:
                    break
        assert np.array_equal(new[k], np.array([x0 + p[0] * f32(2), y0 + p[1] * f32(2)], f32)) and it[k] == n
    # and it is not the lv_l = 0 result
    new0, _, _ = NP.track_points(pa, pb, pts, psz, 2, 0, PC.MAXITER, PC.EPS)
    assert not np.array_equal(new0, new)


@pytest.mark.parametrize("l", range(PC.LV + 1))
def test_one_iteration_at_one_level_is_one_step(O, l):
    """lv_f = lv_l = l, maxiter = 1: (out - pts) / 2^l is one_step's step up to the two f32 roundings of the output."""
    for psz in (8, 17):
        pa, pb = PC.oracle_pyramids(O, "67x53", psz)
        pts = PC.interior("67x53")
        new, ok, it = NP.track_points(pa, pb, pts, psz, l, l, 1, PC.EPS)
        step, bound, _ = NP.one_step(pa, pb, pts, psz, l, 1)
        assert ok.all() and np.all(it == 1)
        got = (new.astype(np.float64) - pts) / 2.0 ** l
        # p = f32(step) (u |step|), out = f32(x0 + p * 2^l) (u |out|)
        assert np.all(np.abs(got - step) <= PC.U * (np.abs(step) + np.abs(new) / 2.0 ** l))
        assert np.abs(step).max() > 0.02
