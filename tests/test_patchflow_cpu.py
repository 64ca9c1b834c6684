"""The patch-flow oracle (oracle/np_patchflow.py) and the case table (patchflow_cases.py) on the CPU: an f32 restatement
of the kernel in each launch form's summation shape stays inside one_step's derived bound, six injected defects each leave
it, every decision of the oracle over the table has the margin that lets the GPU module demand equal status and iters,
the padding of the pyramid does not move a result, and the final rescale is 2^lv_l. The far frames (coordinates of 256 and
more, a displacement known in advance) hold the tap rule: truth, continuity across an integer, the plane's own pixels at
integer centres, the flow grid, and the two ways a rounded-up first tap fails, injected and seen."""
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
    """np_patchflow._sample (slices) against np_oracle.patches (gathers), the reference's util_getPatch: the same bits,
    on a plane padded by psz and through the view of a plane padded by more, at points below 256 with two-decimal
    fractions, where the two first-tap rules (floor(x) + 1 here, ceil(x + 1e-5f) there) choose the same taps.
    np_oracle.patches no longer defines the patch-flow sampling: where the rules differ, _sample is held by
    test_integer_centres_sample_the_planes_own_pixels below, which also shows what np_oracle.patches returns there."""
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


# ---------------------------------------------------------------- the far frames: coordinates of 256 and more
def _far_fulls(group):
    return [j for j in PC.far_jobs(group).values() if j.kind == "full"]


def test_far_points_and_jobs():
    """The triples are one ulp apart around the integers the tap rule needs, there are half-pixel and two-decimal points
    on both sides of 256, every point is the first of its candidates' kind, and the far jobs reach all four forms."""
    for frame in PC.FAR:
        pts, axis = PC.far_points(frame), PC.far_axis(frame)
        w, h = PC.frame_size(frame)
        assert np.all(pts >= 0) and np.all(pts[:, 0] <= w) and np.all(pts[:, 1] <= h)
        ns = [n for n, _ in PC.far_triples(frame)]
        assert set(ns) >= ({512, 514} if max(w, h) == 576 else {24, 63, 64, 100, 255, 256, 257, 300})
        for n, ks in PC.far_triples(frame):
            a = pts[ks, axis]
            assert a[1] == n and np.nextafter(a[0], np.float32(np.inf)) == a[1] == np.nextafter(a[2], np.float32(-np.inf))
            assert len(set(pts[ks, 1 - axis].tolist())) == 1
            if n in PC.FAR_INTEGER:
                assert pts[ks[1], 1 - axis] == np.floor(pts[ks[1], 1 - axis])
        more = pts[3 * len(ns):, axis]
        mid = 512 if max(w, h) == 576 else 256
        assert (more < mid).sum() >= 2 and (more > mid).sum() >= 2
        assert (more % 1 == 0.5).sum() >= 2 and ((more * 100) % 50 != 0).sum() >= 2
        low = PC.far_low(frame)
        assert low.sum() >= (1 if max(w, h) == 576 else 10) and (~low).sum() >= 6
    forms = {PC.form(j) for g in GROUPS for j in PC.far_jobs(g).values()}
    assert forms == {11, 41, 82, 161}
    assert sum(len(PC.far_jobs(g)) for g in GROUPS) == 5 * (3 * 6 + 4)
    for g in GROUPS:
        assert not set(PC.far_jobs(g)) & set(PC.jobs(g))
        big = [j for j in PC.far_jobs(g).values() if j.frame == "farx-576x64"]
        assert {(j.lv_f, j.lv_l) for j in big if j.kind == "full"} == {(1, 1), (2, 0)}
    assert not set(PC.FAR) & set(PC.SIZES)


@pytest.mark.parametrize("group", GROUPS)
def test_far_restatement_stays_within_the_one_step_bound(O, group):
    worst = {}
    for job in PC.far_jobs(group).values():
        if job.kind != "step":
            continue
        for shape in ("form", None):
            new, ok, it = _restate(O, job, shape)
            assert ok.all(), job.key
            key = (PC.form(job), "form" if shape else "serial")
            worst[key] = max(worst.get(key, 0.0), PC.compare_step(job, new, ok, it, O))
    print("far frames, one-step restatement / bound:", worst)
    assert worst and max(worst.values()) <= 1.0


@pytest.mark.parametrize("group", GROUPS)
def test_far_full_runs_truth_and_continuity(O, group):
    """Every full far job, on the oracle and on the restatement: margins, equal decisions and positions (compare_full,
    FULL_FACTOR as for the old table once one spacing of the returned f32 position is taken off, see compare_full), every
    point within the bar of the known shift, every triple continuous. The ratio with that spacing left in is printed with
    its job: it is what exceeds FULL_FACTOR on these frames, and it is exactly one spacing wherever it does."""
    worst, raw, truth, cont = {}, (0.0, None), {}, 0.0
    for job in _far_fulls(group):
        new_o, ok_o, it_o, det = PC.oracle_full(O, job)
        new, ok, it = _restate(O, job)
        f = PC.form(job)
        worst[f] = max(worst.get(f, 0.0), PC.compare_full(job, new, ok, it, O))
        err = np.abs(new.astype(np.float64) - new_o).max(axis=1)
        base = det["bound"] + PC.U * np.abs(new_o).max(axis=1)
        k = int(np.argmax(err / base))
        if err[k] / base[k] > raw[0]:
            raw = (float(err[k] / base[k]), (job.key, job.pts[k].tolist()))
        over = err > PC.FULL_FACTOR * base
        assert np.array_equal(err[over], PC.out_ulp(new_o)[over]), (job.key, "an excess that is not one spacing of f32")
        for res in ((new_o, ok_o, it_o), (new, ok, it)):
            truth[job.psz] = max(truth.get(job.psz, 0.0), PC.check_truth(job, res[0], res[1]))
            cont = max(cont, PC.check_continuity(job, *res, O))
    print(f"far frames, group {group}: full-run restatement / (bound sum + u |new|) beyond one spacing: {worst}; with the "
          f"spacing left in: {raw[0]:.4f} at {raw[1]}; worst truth error per psz {truth} (bars {PC.TRUTH_BAR}); largest "
          f"difference inside a triple {cont:.2e} px")
    assert max(worst.values()) <= PC.FULL_FACTOR


def test_truth_bars_are_twice_the_oracles_error_below_255(O):
    """TRUTH_BAR[psz] = 2 x the f64 oracle's worst |new - pts - shift| over the far jobs' points with every level-0
    coordinate below 255 (and not one ulp below an integer), rounded up to 0.001 px; at most 0.25 px."""
    worst = {}
    for group in GROUPS:
        for job in _far_fulls(group):
            low = PC.far_low(job.frame)
            new_o, ok_o, _, _ = PC.oracle_full(O, job)
            assert ok_o.all()
            worst[job.psz] = max(worst.get(job.psz, 0.0), float(PC.truth_error(job, new_o)[low].max()))
    print("far frames: oracle's worst truth error below 255, per psz:", {k: round(v, 4) for k, v in worst.items()})
    assert set(worst) == set(PC.TRUTH_BAR)
    for psz, bar in PC.TRUTH_BAR.items():
        assert 2 * worst[psz] <= bar <= 2 * worst[psz] + 0.001 and bar <= 0.25, (psz, worst[psz], bar)


INTEGER_CENTRES = (40, 255, 256, 300)


@pytest.mark.parametrize("frame", ("farx-320x64", "fary-64x320"))
def test_integer_centres_sample_the_planes_own_pixels(O, frame):
    """At an integer centre the fraction is 0 and the patch is the plane's own pixels, bit for bit, from row
    y - (P - P/2) and column x - (P - P/2) of the image on (util_getPatch's window, test_oracle_kats.py; P/2 for an even
    P): in the oracle, in the restatement, on a plane padded by psz and by more. np_oracle.patches, the reference's rule,
    gives the same below 256 and the window one pixel back along the long axis from 256 on: the defect this rule
    does not have."""
    from oracle import np_oracle as N
    img = PC.pair(frame)[0]
    axis = PC.far_axis(frame)
    for psz, pad in ((1, 1), (8, 8), (15, 15), (15, 19), (31, 31), (32, 32)):
        pa, _ = PC.oracle_pyramids(O, frame, pad)
        assert np.array_equal(pa.img[0][pad:-pad, pad:-pad], img)
        sh = pad - psz
        view = pa.img[0][sh:, sh:] if sh else pa.img[0]
        for n in INTEGER_CENTRES:
            x, y = (n, 32) if axis == 0 else (32, n)
            r0, c0 = y - (psz - psz // 2), x - (psz - psz // 2)
            own = np.pad(img, psz, mode="edge")[r0 + psz:r0 + 2 * psz, c0 + psz:c0 + 2 * psz]
            assert own.shape == (psz, psz)
            if psz <= 15:
                assert np.array_equal(own, img[r0:r0 + psz, c0:c0 + psz])      # (inside the image: no padding read)
            got, _ = NP._sample(pa.img[0], x, y, psz, pad)
            assert np.array_equal(got, own.astype(np.float64)), (psz, pad, n)
            assert np.array_equal(F32._fetch(view, F32._taps(x, y, psz, None), psz), own.ravel()), (psz, pad, n)
            if pad == psz:
                ref = N.patches(pa.img[0], np.array([x], np.float32), np.array([y], np.float32), psz)[0].reshape(psz, psz)
                back = np.pad(img, psz + 1, mode="edge")
                back = back[r0 + psz + (axis == 0 or n < 256):, c0 + psz + (axis == 1 or n < 256):][:psz, :psz]
                assert np.array_equal(ref, back), (psz, n)
                assert np.array_equal(ref, own) == (n < 256), (psz, n)


def _where(job, level):
    """The coordinate along the long axis at a level, f32 as the kernel forms it."""
    return (job.pts[:, PC.far_axis(job.frame)] * np.float32(0.5 ** level)).astype(np.float32)


def _is_large_integer(job, level):
    a = _where(job, level)
    return (a == np.floor(a)) & (a >= 256)


def _is_just_below_small_integer(job, level):
    a = _where(job, level)
    up = np.nextafter(a, np.float32(np.inf))
    return (up == np.floor(up)) & (up <= 64) & (a != np.floor(a))


def _fails(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("group", GROUPS)
def test_tap_pair_one_back_at_large_integers_is_seen_by_truth_and_continuity(O, group):
    """The first tap of ceil(x + 1e-5f) at an integer x >= 256, injected into the restatement: the truth check fails at
    exactly the points whose coordinate at the run's last level is such an integer, the continuity check at exactly
    their triples; everywhere else the results are the sound restatement's bits."""
    defect = "tap pair one back at large integers"
    seen = 0
    for job in _far_fulls(group):
        new, ok, it = _restate(O, job, defect=defect)
        ref = _restate(O, job)
        hit = np.zeros(len(job.pts), bool)
        for l in range(job.lv_l, job.lv_f + 1):
            hit |= _is_large_integer(job, l)
        assert np.array_equal(new[~hit], ref[0][~hit]) and np.array_equal(it[~hit], ref[2][~hit]), job.key
        last = _is_large_integer(job, job.lv_l)
        assert ok.all()
        bad = ~(PC.truth_error(job, new) <= PC.TRUTH_BAR[job.psz])
        assert np.array_equal(bad, last), (job.key, np.nonzero(bad)[0], np.nonzero(last)[0])
        assert _fails(PC.check_truth, job, new, ok) == bool(last.any()), job.key
        broken = {b[0] for b in PC.discontinuous(job, new, ok, it, O)[0]}
        assert broken == {n for n, ks in PC.far_triples(job.frame) if last[ks].any()}, (job.key, broken)
        assert _fails(PC.check_continuity, job, new, ok, it, O) == bool(last.any()), job.key
        seen += int(last.sum())
        if last.any():
            e = PC.truth_error(job, new)[last]
            # one pixel of the run's last level, as the parent reports it
            assert np.all(np.abs(e - 2.0 ** job.lv_l) <= PC.TRUTH_BAR[job.psz]), (job.key, e)
    assert seen >= 3


@pytest.mark.parametrize("group", GROUPS)
def test_tap_pair_one_ahead_just_below_small_integers_is_seen_by_continuity(O, group):
    """The first tap of ceil(x + 1e-5f) one ulp below an integer n <= 64, injected: the continuity check fails at
    exactly the triples whose lower point is such a value at a level of the run (100 - 1 ulp is one at level 2 only: 25
    - 1 ulp), and the points that are no such value at any level keep the sound restatement's bits."""
    defect = "tap pair one ahead just below small integers"
    seen, coarse = 0, 0
    for job in _far_fulls(group):
        new, ok, it = _restate(O, job, defect=defect)
        ref = _restate(O, job)
        hit = np.zeros(len(job.pts), bool)
        for l in range(job.lv_l, job.lv_f + 1):
            hit |= _is_just_below_small_integer(job, l)
        assert np.array_equal(new[~hit], ref[0][~hit], equal_nan=True) and np.array_equal(it[~hit], ref[2][~hit]), job.key
        last = _is_just_below_small_integer(job, job.lv_l)
        broken = {b[0] for b in PC.discontinuous(job, new, ok, it, O)[0]}
        assert _fails(PC.check_continuity, job, new, ok, it, O) == bool(broken), job.key
        assert broken == {n for n, ks in PC.far_triples(job.frame) if hit[ks].any()}, (job.key, broken)
        seen += sum(bool(last[ks].any()) for _, ks in PC.far_triples(job.frame))
        coarse += sum(bool(hit[ks].any() and not last[ks].any()) for _, ks in PC.far_triples(job.frame))
    assert seen >= 4 * len(PC.GROUP_FORM_PSZ[group]) and coarse >= len(PC.GROUP_FORM_PSZ[group])


@pytest.mark.parametrize("frame", ("farx-320x64", "fary-64x320"))
def test_flow_grid_on_a_far_pair_on_the_oracle(O, frame):
    """dense_flow (the definition of FlowGrid.compute's field) with the oracle tracking the nodes: check_grid."""
    from invcompcamtrack_amd import patchflow as pf
    pa, pb = PC.oracle_pyramids(O, frame, PC.GRID_PSZ)
    kept = {}

    def track(a, b, pts, psz, lv_f, maxiter, eps):
        out = NP.track_points(a, b, pts, psz, lv_f, 0, maxiter, eps)
        kept["ok"] = out[1]
        return out

    field = pf.dense_flow(pa, pb, PC.GRID_STEP, PC.GRID_PSZ, PC.GRID_LV, _track=track)
    xy, _ = PC.grid_nodes(frame)
    got = PC.check_grid(frame, field, ~kept["ok"].reshape(xy.shape[:2]), PC.TRUTH_BAR[PC.GRID_PSZ])
    print(f"{frame}: oracle grid, largest interior error {got[0]:.4f} px, median below 256 {got[1]:.4f}, from 256 on {got[2]:.4f}")
