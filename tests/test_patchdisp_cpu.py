"""The 1-D patch search on the CPU: the f64 oracle (patchdisp_np.py), the f32 restatement of k_patchdisp
(patchdisp_f32.py) and the case table (patchdisp_cases.py). The chosen points have their margins, the restatement stays
within the derived one-step bound in every form's summation shape and within FULL_FACTOR over full runs, every injected
defect is seen, the exact cases (rows, columns, textureless, the rolled pair) come out as the rule says, and on the
tilted-grating scene the 1-D oracle is right where the 2-D oracle is wrong."""
import numpy as np
import pytest

import patchdisp_cases as DC
import patchdisp_f32 as F32
import patchdisp_np as DN
from oracle import np_patchflow as NP


@pytest.fixture(scope="module")
def O(oracle):
    return oracle


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _shape(job):
    f = DC.form(job)
    return f // 10, f % 10


def _restate(O, job, shape="form", defect=None):
    pa, pb = DC.oracle_pyramids(O, job.frame, job.pad)
    return F32.track_disparity(pa, pb, job.pts, job.psz, job.lv_f, job.lv_l, job.maxiter, DC.EPS, DC.MIN_HX,
                               shape=_shape(job) if shape == "form" else shape, defect=defect)


def test_dispatch_table_matches_the_launcher():
    """FORM is launch_patchdisp's choice (restated in patchdisp_np.form_of): three forms, by the patch size alone."""
    for psz, f in DC.FORM.items():
        npl, wpp = DN.form_of(psz)
        assert npl * 10 + wpp == f, psz
        assert NP.lane_pixels(psz, wpp) <= npl
    assert set(DC.FORM.values()) == {11, 41, 82}
    assert all(DN.form_of(p)[0] * 10 + DN.form_of(p)[1] in (11, 41, 82) for p in range(1, 33))


def test_point_sets():
    for frame in DC.INTERIOR:
        w, h = DC.PC.frame_size(frame)
        p = DC.interior(frame)
        assert len(p) >= DC.N_INTERIOR and np.all(p >= 8) and np.all(p[:, 0] <= w - 8) and np.all(p[:, 1] <= h - 8)


def test_restatement_stays_within_the_one_step_bound(O):
    """Every 'step' job: the kernel's arithmetic in f32, in the form's summation shape and as one serial sum, against
    the f64 step. The worst ratios are printed (-s) and recorded in DESIGN.md."""
    worst = {}
    for job in DC.jobs().values():
        if job.kind != "step":
            continue
        for shape in ("form", None):
            new, ok, it = _restate(O, job, shape)
            r = DC.compare_step(job, new, ok, it, O)
            key = (DC.form(job), "form" if shape else "serial")
            worst[key] = max(worst.get(key, 0.0), r)
    print("one-step restatement / bound:", worst)
    assert len(worst) == 6 and max(worst.values()) <= 1.0


def test_margins_hold_and_full_runs_stay_within_the_factor(O):
    """Every job that runs to convergence: the oracle's decisions have their margins (check_margins inside compare_full)
    for every point, none left out; the restatement takes the same decisions, and its x is within FULL_FACTOR of bound
    sum + u |new_x|. FULL_FACTOR is this module's measurement, never the device's."""
    worst = {}
    for job in DC.jobs().values():
        if job.kind not in ("full", "pad", "rows"):
            continue
        new, ok, it = _restate(O, job)
        r = DC.compare_full(job, new, ok, it, O)
        worst[DC.form(job)] = max(worst.get(DC.form(job), 0.0), r)
    print("full-run restatement / (bound sum + u |new_x|):", worst)
    assert len(worst) == 3 and max(worst.values()) <= DC.FULL_FACTOR


# ---------------------------------------------------------------- injected defects
STEP_DEFECTS = {  # defect -> key of a 'step' job; "half of P-1" needs an even P, "omit second wave" two waves
    "drop last column": "step-100x77-p15-l0",
    "drop last row": "step-100x77-p15-l0",
    "swap w1 w2": "step-100x77-p15-l0",
    "half of P-1": "step-100x77-p16-l0",
    "omit second wave": "step-100x77-p31-l0",
    "solve by tr": "step-100x77-p15-l0",
}
# these act only from the second step or the second level on: seen by the full-run check
FULL_DEFECTS = {"rescale by lv_f": "full-100x77-p15-21", "no doubling": "full-100x77-p15-20", "y follows x": "full-100x77-p15-20"}


def test_every_defect_has_a_test():
    assert set(STEP_DEFECTS) | set(FULL_DEFECTS) == set(F32.DEFECTS)


@pytest.mark.parametrize("defect", sorted(STEP_DEFECTS))
def test_injected_defect_exceeds_the_bound(O, defect):
    job = DC.jobs()[STEP_DEFECTS[defect]]
    new, ok, it = _restate(O, job, defect=defect)
    step, bound, _ = DC.oracle_step(O, job)
    live = np.isfinite(step) & ok
    live[DC.N_INTERIOR:] = False
    assert live[:DC.N_INTERIOR].all()
    if defect == "swap w1 w2":
        with np.errstate(invalid="ignore"):
            r0, r1 = job.pts[:, 0] - np.floor(job.pts[:, 0]), job.pts[:, 1] - np.floor(job.pts[:, 1])
        live &= r0 != r1          # equal fractions: w1 == w2, nothing to swap
        assert live.sum() >= 8
    got = (new[live, 0].astype(np.float64) - job.pts[live, 0]) / 2.0 ** job.lv_f
    tol = bound[live] + DC.U * np.abs(new[live, 0].astype(np.float64)) / 2.0 ** job.lv_f
    ratio = np.abs(got - step[live]) / tol
    print(f"defect {defect!r}: error / bound per interior point, smallest {ratio.min():.1f}, largest {ratio.max():.1f}")
    assert np.all(ratio > 1.0), (defect, ratio)
    with pytest.raises(AssertionError):
        DC.compare_step(job, new, ok, it, O)


@pytest.mark.parametrize("defect", sorted(FULL_DEFECTS))
def test_injected_defect_exceeds_the_full_run_tolerance(O, defect):
    job = DC.jobs()[FULL_DEFECTS[defect]]
    new, ok, it = _restate(O, job, defect=defect)
    with pytest.raises(AssertionError):
        DC.compare_full(job, new, ok, it, O)
    new_o, ok_o, _, det = DC.oracle_full(O, job)
    live = ok_o & ok
    live[DC.N_INTERIOR:] = False
    err = np.abs(new[live, 0].astype(np.float64) - new_o[live, 0])
    ratio = err / DC.full_tolerance(new_o, det)[live]
    print(f"defect {defect!r}: error / tolerance per interior point, smallest {ratio.min():.1f}, largest {ratio.max():.1f}")
    assert ratio.max() > 1.0


# ---------------------------------------------------------------- exact cases
@pytest.mark.parametrize("psz", (1, 8, 15, 31))
def test_rows_frame_is_kept_where_the_2d_rule_loses_it(O, psz):
    """rows-100x77 (A = B, vertical structure alone in rows 8..h-8): the 1-D oracle keeps all 10 interior points, returns
    pts' bits, and iterates once per level (r = 0: dx = 0 < eps). The 2-D oracle loses points there."""
    pts = DC.interior("100x77")
    for lv_f, lv_l in ((0, 0), (2, 0), (2, 1)):
        job = DC.jobs()[f"rows-p{psz}-{lv_f}{lv_l}"]
        new, ok, it, _ = DC.oracle_full(O, job)
        assert ok.all() and np.array_equal(_bits(new), _bits(pts)) and np.all(it == lv_f - lv_l + 1), (psz, lv_f, lv_l)
        new, ok, it = _restate(O, job)
        assert ok.all() and np.array_equal(_bits(new), _bits(pts)) and np.all(it == lv_f - lv_l + 1), (psz, lv_f, lv_l)
    pa, pb = DC.oracle_pyramids(O, "rows-100x77", psz)
    _, ok2, _ = NP.track_points(pa, pb, pts, psz, 2, 0, DC.MAXITER, DC.EPS)
    print(f"rows-100x77 psz {psz}: the 2-D oracle keeps {int(ok2.sum())} of {len(pts)}, the 1-D oracle all")
    assert not ok2.all()


def test_columns_and_textureless_frames_are_lost(O):
    """A patch without x gradient (columns all equal: hxx = 0 exactly; constant: tr = 0) is lost with 0 iterations."""
    seen = 0
    for job in DC.jobs().values():
        if job.kind != "lost":
            continue
        pa, pb = DC.oracle_pyramids(O, job.frame, job.pad)
        for k, (x, y) in enumerate(job.pts):
            sc = np.float32(0.5 ** job.lv_f)
            gx, _ = NP._sample(pa.dx[job.lv_f], np.float32(x * sc), np.float32(y * sc), job.psz, job.pad)
            assert np.all(gx == 0.0), (job.key, k)          # the premise: the patch holds no x gradient
        _, _, cond = DN.one_step(pa, pb, job.pts, job.psz, job.lv_f, 1)
        if job.frame.startswith("flat"):
            assert np.isnan(cond).all(), job.key            # tr == 0: no ratio
        else:
            assert np.all(cond == 0.0), job.key             # hxx == 0 exactly, hyy > 0
        for new, ok, it in (DC.oracle_full(O, job)[:3], _restate(O, job)):
            assert not ok.any() and np.all(it == 0) and np.isnan(new).all(), job.key
        seen += 1
    assert seen >= 16


def test_maxiter0_special_and_leaving_points(O):
    for job in DC.jobs().values():
        if job.kind == "maxiter0":
            new, ok, it, _ = DC.oracle_full(O, job)
            n = DC.N_INTERIOR
            assert ok[:n].all() and np.array_equal(_bits(new[ok]), _bits(job.pts[ok])) and np.all(it == 0), job.key
            assert not ok[-6:].any() and np.isnan(new[~ok]).all(), job.key
        elif job.key.startswith("leave") and job.psz > 1:
            _, ok, it, _ = DC.oracle_full(O, job)
            assert (~ok & (it > 0)).sum() >= 3, (job.key, ok, it)   # lost after iterating: they left the view in x


def test_rolled_pair_recovers_the_shift(O):
    """B = A rolled by 6 px: away from the wrap B(x + 6) = A(x) exactly, so p = 6 has zero residual and is a fixed point
    of the iteration; Gauss-Newton on a zero-residual problem contracts faster than linearly, so when the last step is
    below eps the distance left is below eps too."""
    job = DC.jobs()["roll-p15-20"]
    new, ok, it, _ = DC.oracle_full(O, job)
    assert ok.all() and np.all(job.pts[:, 0] + DC.ROLL + 8 < 100)
    d = new[:, 0].astype(np.float64) - job.pts[:, 0]
    print(f"roll-100x77 psz 15: recovered shift {d.min():.4f} .. {d.max():.4f}")
    assert np.all(np.abs(d - DC.ROLL) <= DC.EPS)
    assert np.array_equal(_bits(new[:, 1]), _bits(job.pts[:, 1]))


def test_padding_does_not_move_the_result(O):
    for psz in DC.FORM_PSZ:
        ref = DC.oracle_full(O, DC.jobs()[f"pad0-p{psz}"])
        ref32 = _restate(O, DC.jobs()[f"pad0-p{psz}"])
        assert ref[1].all()
        for extra in DC.PAD_EXTRA[1:]:
            got = DC.oracle_full(O, DC.jobs()[f"pad{extra}-p{psz}"])
            for a, b in zip(ref[:3], got[:3]):
                assert np.array_equal(a, b), (psz, extra)
            new, ok, it = _restate(O, DC.jobs()[f"pad{extra}-p{psz}"])
            assert np.array_equal(new, ref32[0]) and np.array_equal(it, ref32[2])


# ---------------------------------------------------------------- usefulness
@pytest.mark.parametrize("tilt", DC.SCENE_TILTS)
@pytest.mark.parametrize("seed", DC.SCENE_SEEDS)
def test_usefulness_on_the_oracle(O, tilt, seed):
    """Gratings near one direction, shifted along x: the 2-D step moves along the gradient and its x is not the
    disparity (the aperture problem); the 1-D search keeps every node and finds the shift."""
    a, b = DC.scene(tilt, seed)
    pa, pb = O.Pyramid(a, DC.SCENE_LV, DC.SCENE_PSZ), O.Pyramid(b, DC.SCENE_LV, DC.SCENE_PSZ)
    nodes = DC.scene_nodes()
    assert len(nodes) == 98
    new1, ok1, _ = DN.track_disparity(pa, pb, nodes, DC.SCENE_PSZ, DC.SCENE_LV)
    new2, ok2, _ = NP.track_points(pa, pb, nodes, DC.SCENE_PSZ, DC.SCENE_LV)
    k1, med1, max1 = DC.scene_errors(new1, ok1)
    k2, med2, _ = DC.scene_errors(new2, ok2)
    print(f"tilt {tilt} seed {seed}: 1-D kept {k1}, median {med1:.4f} max {max1:.4f} px; 2-D kept {k2}, median {med2:.4f} px")
    assert k1 == 98 and med1 <= DC.BAR_1D
    assert med2 >= DC.BAR_2D


# ---------------------------------------------------------------- the far frame: x of 256 and more
def _far_fulls():
    return [j for j in DC.far_jobs().values() if j.kind == "full"]


def test_far_jobs_are_the_2d_tests_frame_and_points():
    jobs = DC.far_jobs()
    assert not set(jobs) & set(DC.jobs()) and len(jobs) == 3 * 6
    assert {DC.form(j) for j in jobs.values()} == {11, 41, 82}
    for j in jobs.values():
        assert j.frame == DC.FAR_FRAME and np.array_equal(j.pts, DC.PC.far_points(DC.FAR_FRAME))
    assert {(j.lv_f, j.lv_l) for j in _far_fulls()} == set(DC.PC.FAR_RANGES)


def test_far_restatement_stays_within_the_one_step_bound(O):
    worst = {}
    for job in DC.far_jobs().values():
        if job.kind != "step":
            continue
        for shape in ("form", None):
            new, ok, it = _restate(O, job, shape)
            assert ok.all(), job.key
            key = (DC.form(job), "form" if shape else "serial")
            worst[key] = max(worst.get(key, 0.0), DC.compare_step(job, new, ok, it, O))
    print("far frame, one-step restatement / bound:", worst)
    assert len(worst) == 6 and max(worst.values()) <= 1.0


def test_far_full_runs_truth_and_continuity(O):
    """Every full far job, on the oracle and on the restatement: margins, equal decisions and x (compare_full, FULL_FACTOR
    as for the old table once one spacing of the returned f32 x is taken off), every point within the bar of the known
    shift, every triple continuous. An excess over FULL_FACTOR with the spacing left in is exactly one spacing."""
    worst, raw, truth, cont = {}, (0.0, None), {}, 0.0
    for job in _far_fulls():
        new_o, ok_o, it_o, det = DC.oracle_full(O, job)
        new, ok, it = _restate(O, job)
        f = DC.form(job)
        worst[f] = max(worst.get(f, 0.0), DC.compare_full(job, new, ok, it, O))
        err = np.abs(new[:, 0].astype(np.float64) - new_o[:, 0])
        base = DC.base_tolerance(new_o, det)
        k = int(np.argmax(err / base))
        if err[k] / base[k] > raw[0]:
            raw = (float(err[k] / base[k]), (job.key, job.pts[k].tolist()))
        over = err > DC.FULL_FACTOR * base
        assert np.array_equal(err[over], DC.out_ulp(new_o)[over]), (job.key, "an excess that is not one spacing of f32")
        for res in ((new_o, ok_o, it_o), (new, ok, it)):
            truth[job.psz] = max(truth.get(job.psz, 0.0), DC.check_truth(job, res[0], res[1]))
            cont = max(cont, DC.check_continuity(job, *res, O))
    print(f"far frame: full-run restatement / (bound sum + u |new_x|) beyond one spacing: {worst}; with the spacing left "
          f"in: {raw[0]:.4f} at {raw[1]}; worst truth error per psz {truth} (bars {DC.TRUTH_BAR}); largest difference "
          f"inside a triple {cont:.2e} px")
    assert len(worst) == 3 and max(worst.values()) <= DC.FULL_FACTOR


def test_truth_bars_are_twice_the_oracles_error_below_255(O):
    worst = {}
    low = DC.PC.far_low(DC.FAR_FRAME)
    for job in _far_fulls():
        new_o, ok_o, _, _ = DC.oracle_full(O, job)
        assert ok_o.all()
        worst[job.psz] = max(worst.get(job.psz, 0.0), float(DC.truth_error(job, new_o)[low].max()))
    print("far frame: oracle's worst truth error below 255, per psz:", {k: round(v, 4) for k, v in worst.items()})
    assert set(worst) == set(DC.TRUTH_BAR)
    for psz, bar in DC.TRUTH_BAR.items():
        assert 2 * worst[psz] <= bar <= 2 * worst[psz] + 0.001 and bar <= 0.25, (psz, worst[psz], bar)


def _hits(job, level, large):
    a = (job.pts[:, 0] * np.float32(0.5 ** level)).astype(np.float32)
    if large:
        return (a == np.floor(a)) & (a >= 256)
    up = np.nextafter(a, np.float32(np.inf))
    return (up == np.floor(up)) & (up <= 64) & (a != np.floor(a))


@pytest.mark.parametrize("defect", F32.TAP_DEFECTS)
def test_tap_defects_are_seen(O, defect):
    """The two failure forms of a first tap at ceil(x + 1e-5f), injected (they act in x and in y; on this frame the y are
    below 64 and none is one ulp below an integer). At integers >= 256: the truth check fails at exactly the points that
    are one at the run's last level, by one pixel of that level, and the continuity check at their triples. One ulp
    below an integer <= 64: the continuity check fails at exactly the triples that hold such a value at a level of the
    run. Every other point keeps the sound restatement's bits."""
    large = defect == F32.TAP_DEFECTS[0]
    seen = 0
    for job in _far_fulls():
        new, ok, it = _restate(O, job, defect=defect)
        ref = _restate(O, job)
        hit = np.zeros(len(job.pts), bool)
        for l in range(job.lv_l, job.lv_f + 1):
            hit |= _hits(job, l, large)
        assert ok.all()
        assert np.array_equal(new[~hit], ref[0][~hit]) and np.array_equal(it[~hit], ref[2][~hit]), job.key
        last = _hits(job, job.lv_l, large)
        triples = DC.PC.far_triples(job.frame)
        broken = {b[0] for b in DC.discontinuous(job, new, ok, it, O)[0]}
        if large:
            e = DC.truth_error(job, new)
            assert np.array_equal(~(e <= DC.TRUTH_BAR[job.psz]), last), (job.key, e)
            assert np.all(np.abs(e[last] - 2.0 ** job.lv_l) <= DC.TRUTH_BAR[job.psz]), (job.key, e[last])
            assert broken == {n for n, ks in triples if last[ks].any()}, (job.key, broken)
            if last.any():
                with pytest.raises(AssertionError):
                    DC.check_truth(job, new, ok)
            else:
                DC.check_truth(job, new, ok)
        else:
            assert broken == {n for n, ks in triples if hit[ks].any()}, (job.key, broken)
        if broken:
            with pytest.raises(AssertionError):
                DC.check_continuity(job, new, ok, it, O)
        else:
            DC.check_continuity(job, new, ok, it, O)
        seen += int(last.sum())
    assert seen >= 9


def test_flow_grid_compute_x_on_the_far_pair_on_the_oracle(O):
    """dense_disparity's host path (the definition of FlowGrid.compute_x's field) with the 1-D oracle tracking the nodes."""
    from invcompcamtrack_amd import patchflow as pf
    PC = DC.PC
    pa, pb = DC.oracle_pyramids(O, DC.FAR_FRAME, PC.GRID_PSZ)
    kept = {}

    def track(a, b, pts, psz, lv_f, maxiter, eps):
        out = DN.track_disparity(a, b, pts, psz, lv_f, 0, maxiter, eps)
        kept["ok"] = out[1]
        return out

    field = pf.dense_flow(pa, pb, PC.GRID_STEP, PC.GRID_PSZ, PC.GRID_LV, _track=track)
    assert not field[..., 1].any()
    xy, _ = PC.grid_nodes(DC.FAR_FRAME)
    got = PC.check_grid(DC.FAR_FRAME, field, ~kept["ok"].reshape(xy.shape[:2]), DC.TRUTH_BAR[PC.GRID_PSZ])
    print(f"oracle grid (x only), largest interior error {got[0]:.4f} px, median below 256 {got[1]:.4f}, from 256 on {got[2]:.4f}")
