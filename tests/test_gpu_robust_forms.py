"""The robustness options (set_robust: clean_invisible, compositional, huber_k) in every kernel that carries a copy of
their code, each launch form on its own.

Any option routes a tracking to the any-size kernels, so two families hold the option code: the one-launch tracker
k_track1<TL> (ictr_track1.hip; TL: templates in LDS, or re-read from global memory) and the per-iteration launches
k_ref_any / k_iter_any (ictr_kernels.hip), replayed as one hipGraph or issued as plain launches; the compose branch of the
update (ictr_devfn.h) is shared by the tails of both. Every case below names its form, asserts through path_name() that
this form ran, and holds every record of the device trace to the serial solver turn (parity_util.check_solver_turns).

Judge: oracle/np_oracle.py's track with the same options, itself pinned to the C oracle on the CPU with the options off
(tests/test_oracle_kats.py: visibility masks, patch normalisation, loop rule). It runs with the C oracle's exp map, whose
bits are the host build's (tests/test_abi_cpu.py), so that projections and patches are comparable bit for bit.

Bars, all taken from tests/test_gpu_parity.py (none from the device's output):
  patches T/Gx/Gy of the points in the reference view: bit-equal to NumPy; patches and sd coefficients bit-equal
  between the forms; first-iteration H within SUM_TOL, b within SUM_TOL (1e-5 where points are out of view, the bar of
  test_points_out_of_view_and_stale_state_across_frames); first dp within DP_TOL; final pose within POSE_TOL; poses of
  two forms within 5e-6 (test_one_launch_tracker_equals_per_iteration_launches). Frames are 256 x 224: trajectories are
  comparable step by step below 256 px only (module docstring of test_gpu_parity.py).
Each test prints the worst differences it saw (pytest -s); DESIGN.md's parity-status section records them."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import invcompcamtrack_amd as ic
from parity_util import Pair, check_solver_turns, rel, same_bits, scene
from test_gpu_parity import DP_TOL, POSE_TOL, SUM_TOL
from test_gpu_robust import _compose
from test_gpu_solver import SE3_K

gpu = pytest.mark.gpu

B_TOL_VIEW = 1e-5   # first b with points out of view (test_points_out_of_view_and_stale_state_across_frames)
FORM_POSE_TOL = 5e-6  # poses of two launch forms (test_one_launch_tracker_equals_per_iteration_launches)
HUBER_K = 6.0
W, H_ = 256, 224

FORMS = {  # name -> (selection bits, what path_name() must say, what it must not say)
    "k_track1": (ic.VARIANT_ONE_LAUNCH | ic.VARIANT_NO_TEAMS, "k_track1", "workgroups per problem"),
    "graph": (ic.VARIANT_LAUNCHES, "hipGraph", "k_track1"),
    "plain": (ic.VARIANT_LAUNCHES | ic.VARIANT_NO_GRAPH, "k_iter", "hipGraph"),
}
FLAG_SETS = ["clean", "compose", "huber", "clean+compose", "clean+huber", "compose+huber", "clean+compose+huber"]


def _robust(flags):
    f = set(flags.split("+")) if flags else set()
    assert f <= {"clean", "compose", "huber"}
    return dict(clean_invisible="clean" in f, compositional="compose" in f, huber_k=HUBER_K if "huber" in f else 0.0)


def _assert_form(form, name):
    _, want, never = FORMS[form]
    assert want in name and never not in name, (form, name)


# ------------------------------------------------------------------------------------------------------------ scenes
@functools.lru_cache(maxsize=None)
def _view_scene(npts, margin):
    """A third of the points outside the reference view: the start pose is p_a moved by 4.3 along x (every projection
    moves by 4.3 fx / depth = 86 px of 256). A true motion of ~6 px lets points cross the border between iterations too,
    so the new-view mask is not the reference-view mask."""
    sc = scene(W, H_, npts, seed=12, margin=margin, dp_gt=np.array([0.3, -0.18, 0.04, 0.004, -0.003, 0.005]))
    p0 = sc["p_a"].copy()
    p0[0] += 4.3
    return sc, p0


@functools.lru_cache(maxsize=None)
def _plain_scene():
    sc = scene(W, H_, 150, seed=21, margin=40.0)
    return sc, sc["p_a"].copy()


@functools.lru_cache(maxsize=None)
def _occluded_scene():
    """The scene of test_options_match_numpy_oracle with a block of frame B replaced by noise: outliers."""
    sc = dict(scene(W, H_, 150, seed=21, margin=40.0))
    img_b = sc["img_b"].copy()
    img_b[60:130, 70:150] = np.random.default_rng(1).uniform(0, 255, (70, 80)).astype(np.float32)
    sc["img_b"] = img_b
    return sc, sc["p_a"].copy()


def _shape(psz):
    return (40, 40.0) if psz == 16 else (150, 2.0)


# --------------------------------------------------------------------------------------------- the NumPy side, cached
_NP = {}


def _numpy_run(oracle, key, sc, p0, psz, flags, lv_f=2, lv_l=0, maxiter=5, dpn=0, swap=False):
    """np_oracle.track with the options of `flags`, once per key."""
    k = (key, psz, flags, lv_f, lv_l, maxiter, dpn, swap)
    if k not in _NP:
        from oracle import np_oracle as N
        rb = _robust(flags)
        pa, pb = oracle.Pyramid(sc["img_a"], lv_f, psz), oracle.Pyramid(sc["img_b"], lv_f, psz)
        if swap:
            pa, pb = pb, pa
        n = sc["pts3d"].shape[1]
        cam = oracle.Tracker(oracle.make_op(lv_f, lv_l, psz, maxiter, 0.0, 0, dpn, n), sc["fc"], sc["cc"], sc["wh"])
        detail = {}
        p, trace = N.track(sc["pts3d"], p0, pa, pb, cam.cam_get, lv_f, lv_l, psz, maxiter, oracle.solve6,
                           compose=_compose(oracle) if rb["compositional"] else None, huber_k=rb["huber_k"],
                           clean_invisible=rb["clean_invisible"], dopatchnorm=bool(dpn), exp=oracle.se3_exp, detail=detail)
        _NP[k] = SimpleNamespace(pose=p.astype(np.float64), trace=trace, detail=detail)
    return _NP[k]


# ------------------------------------------------------------------------------------------------ the device side
def _device_run(oracle, sc, p0, form, psz, flags, lv_f=2, lv_l=0, maxiter=5, ratio=0.0, donorm=0, dpn=0, extra=0,
                robust=None, chain=None):
    """One tracking in one form, trace-checked. chain: (p_first, swap) tracks a first pair from p_first before the pair
    that is returned, without Set3Dpoints in between (run_track_nposes.cpp:232-258)."""
    pr = Pair(oracle, sc, lv_f, lv_l, psz, maxiter, ratio, donorm, dpn, variant=FORMS[form][0] | extra)
    rb = _robust(flags) if robust is None else robust
    if any(rb.values()):
        pr.odo.set_robust(**rb)
    pr.odo.Set3Dpoints(np.ascontiguousarray(sc["pts3d"].copy()))
    compose = None
    if rb.get("compositional"):
        e, l = ic.util_SE3_coeff_to_group, ic.util_SE3_group_to_coeff
        compose = (SE3_K, e, l, e, l)
    first = None
    if chain is not None:
        pr.odo.SetPose(chain, pr.gpa, pr.gpb)
        first = pr.odo.TrackPose()
        p0 = p0(first)
        pr.odo.SetPose(p0, pr.gpb, pr.gpa)
    else:
        pr.odo.SetPose(p0, pr.gpa, pr.gpb)
    p_start = pr.pose.state()[0]
    pg = pr.odo.TrackPose()
    _assert_form(form, pr.odo.path_name())
    tr = check_solver_turns(pr.odo, p_start, pr.op, p_final=pg, compose=compose)
    nv, n = pr.op.novals, pr.n
    bufs = [pr.odo.read_buffer(w, nv * n).reshape(n, -1) for w in (0, 1, 2)]
    return SimpleNamespace(pr=pr, pose=pg, trace=tr, bufs=bufs, coef=pr.odo.read_buffer(7, 16 * n), first=first, p0=p0)


_DEV = {}


def _cached_device_run(oracle, key, sc, p0, form, psz, flags, **kw):
    k = (key, form, psz, flags, tuple(sorted(kw.items())))
    if k not in _DEV:
        _DEV[k] = _device_run(oracle, sc, p0, form, psz, flags, **kw)
    return _DEV[k]


def _seq(trace):
    return [(r["level"], r["iter"]) for r in trace]


def _against_numpy(dev, ref, lv_l, b_tol, label):
    """The bars of (a) between one device run and the NumPy run of the same options. Returns the observed figures."""
    vr = ref.detail[lv_l]["vis_ref"]
    n = len(vr)
    for w, key in ((0, "T"), (1, "Gx"), (2, "Gy")):
        want = ref.detail[lv_l][key].reshape(n, -1)
        assert np.array_equal(dev.bufs[w][vr], want[vr]), (label, key, "patches of the points in the reference view")
    assert _seq(dev.trace) == _seq(ref.trace), label
    a, b = ref.trace[0], dev.trace[0]
    fig = dict(H=rel(a["H"], b["H"]), b=rel(a["b"], b["b"]),
               dp=np.abs(a["dp"] - b["dp"]).max() / np.abs(a["dp"]).max(), pose=np.abs(dev.pose - ref.pose).max())
    print(f"[{label}] vs NumPy: H {fig['H']:.2e} (bar {SUM_TOL:.0e})  b {fig['b']:.2e} (bar {b_tol:.0e})  "
          f"first dp {fig['dp']:.2e} (bar {DP_TOL:.0e})  pose {fig['pose']:.2e} (bar {POSE_TOL:.0e})")
    assert fig["H"] <= SUM_TOL, (label, "first H", fig)
    assert fig["b"] <= b_tol, (label, "first b", fig)
    assert fig["dp"] <= DP_TOL, (label, "first dp", fig)
    assert fig["pose"] <= POSE_TOL, (label, "final pose", fig)
    return fig


def _between_forms(one, other, label):
    for w in range(3):
        assert np.array_equal(one.bufs[w], other.bufs[w]), (label, "patch buffer", w)
    assert np.array_equal(one.coef, other.coef), (label, "sd coefficients")
    assert _seq(one.trace) == _seq(other.trace), (label, "iteration counts")
    d = np.abs(one.pose - other.pose).max()
    print(f"[{label}] between forms: pose {d:.2e} (bar {FORM_POSE_TOL:.0e})")
    assert d <= FORM_POSE_TOL, (label, d)


def _same_tracking(a, b, label, bufs=True):
    """Bit for bit: pose, records (H, b, dp, p) and, with bufs, the patch and coefficient buffers."""
    assert np.array_equal(a.pose, b.pose), (label, "pose", np.abs(a.pose - b.pose).max())
    assert _seq(a.trace) == _seq(b.trace), (label, "iteration counts")
    for ra, rb in zip(a.trace, b.trace):
        for k in ("H", "b", "dp", "p"):
            assert same_bits(ra[k], rb[k]), (label, k, ra["level"], ra["iter"])
    if bufs:
        for w in range(3):
            assert np.array_equal(a.bufs[w], b.bufs[w]), (label, "patch buffer", w)
        assert np.array_equal(a.coef, b.coef), (label, "sd coefficients")


# ------------------------------------------------------------- (a) each flag set in each form against NumPy
CASES_A = [(8, f) for f in FLAG_SETS] + [(p, f) for p in (4, 5, 16) for f in ("huber", "clean+compose+huber")]


def _case_a(oracle, psz, flags, form):
    npts, margin = _shape(psz)
    sc, p0 = _view_scene(npts, margin)
    key = ("view", npts, margin)
    ref = _numpy_run(oracle, key, sc, p0, psz, flags)
    out = 1.0 - ref.detail[0]["vis_ref"].mean()
    assert 0.15 < out < 0.6, out
    assert any(not np.array_equal(r["vis_new"], ref.detail[r["level"]]["vis_ref"]) for r in ref.trace) or psz == 16
    if "huber" in flags:
        assert ref.trace[0]["over"] > 0.01  # the weight branch fires
    return ref, _cached_device_run(oracle, key, sc, p0, form, psz, flags)


def _forms_of(psz):  # psz 4, 5, 16 run in the one-launch and the graph form
    return list(FORMS) if psz == 8 else ["k_track1", "graph"]


@gpu
@pytest.mark.parametrize("psz,flags,form", [(p, f, form) for p, f in CASES_A for form in _forms_of(p)])
def test_each_option_set_in_each_form_matches_numpy(oracle, psz, flags, form):
    """A third of the points outside the reference view, the rest tracked with the options of `flags`."""
    ref, dev = _case_a(oracle, psz, flags, form)
    _against_numpy(dev, ref, 0, B_TOL_VIEW, f"a/{form}/psz{psz}/{flags}")


@gpu
@pytest.mark.parametrize("psz,flags", CASES_A)
def test_each_option_set_gives_the_same_tracking_in_every_form(oracle, psz, flags):
    forms = _forms_of(psz)
    runs = [_case_a(oracle, psz, flags, f)[1] for f in forms]
    for f, r in zip(forms[1:], runs[1:]):
        _between_forms(runs[0], r, f"a/{forms[0]}~{f}/psz{psz}/{flags}")


# --------------------------------------------------------------------------- (b) Huber on inputs with outliers
@gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("psz", [8, 4])
def test_huber_weights_do_their_job_on_outliers(oracle, psz, form):
    """A 70 x 80 block of frame B is noise. The weighted device run follows the weighted NumPy run, and the option does
    what it is for: |p_huber - p_b|inf < 0.25 |p_default - p_b|inf on the device and, before that, in NumPy (measured
    with NumPy alone: psz 8 default 4.1e-2, k=6 2.6e-3, ratio 0.063; psz 4 0.26, 8.3e-3, 0.032: the bar leaves a factor
    of 4)."""
    sc, p0 = _occluded_scene()
    ref = _numpy_run(oracle, "occluded", sc, p0, psz, "huber")
    ref0 = _numpy_run(oracle, "occluded", sc, p0, psz, "")
    assert 0.05 < ref.trace[0]["over"] < 0.6, ref.trace[0]["over"]
    err = lambda p: np.abs(np.asarray(p, np.float64) - sc["p_b"]).max()
    assert err(ref.pose) < 0.25 * err(ref0.pose), ("the NumPy restatement's own ratio", err(ref.pose), err(ref0.pose))
    dev = _device_run(oracle, sc, p0, form, psz, "huber")
    dev0 = _device_run(oracle, sc, p0, form, psz, "")
    d = np.abs(dev.pose - ref.pose).max()
    print(f"[b/{form}/psz{psz}] pose vs NumPy {d:.2e} (bar {POSE_TOL:.0e}); error default {err(dev0.pose):.2e}, k=6 "
          f"{err(dev.pose):.2e}, ratio {err(dev.pose) / err(dev0.pose):.3f} (bar 0.25; NumPy "
          f"{err(ref.pose) / err(ref0.pose):.3f}); residuals above k at the first iteration {ref.trace[0]['over']:.2f}")
    assert _seq(dev.trace) == _seq(ref.trace)
    assert d <= POSE_TOL
    assert err(dev.pose) < 0.25 * err(dev0.pose)


# ------------------------------------------------------------------------------- (c) metamorphic identities
@gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_a_huber_threshold_never_reached_is_the_any_size_run(oracle, form):
    """huber_k = 1e30: the weight branch never fires; poses, records and buffers are those of the same form without an
    option and with VARIANT_ANY_SIZE, bit for bit."""
    sc, p0 = _plain_scene()
    a = _device_run(oracle, sc, p0, form, 8, "", robust=dict(huber_k=1e30))
    b = _device_run(oracle, sc, p0, form, 8, "", extra=ic.VARIANT_ANY_SIZE)
    _same_tracking(a, b, f"c/{form}/huber 1e30")
    c = _device_run(oracle, sc, p0, form, 8, "huber")
    assert not np.array_equal(a.pose, c.pose)  # (and k = 6 is not that run)


@gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("view", ["all_in_view", "third_out_of_view"])
def test_clean_invisible_on_a_first_pair_is_the_any_size_run(oracle, form, view):
    """Every point in view: nothing to clean. A third outside the reference view on a fresh engine: what the default
    keeps for them are the zeros of Set3Dpoints, so clean_invisible changes no bit either."""
    sc, p0 = _plain_scene() if view == "all_in_view" else _view_scene(150, 2.0)
    a = _device_run(oracle, sc, p0, form, 8, "clean")
    b = _device_run(oracle, sc, p0, form, 8, "", extra=ic.VARIANT_ANY_SIZE)
    _same_tracking(a, b, f"c/{form}/clean/{view}")
    vis = np.abs(a.coef.reshape(-1, 16)[:, :12]).sum(1) > 0  # points that were in the reference view at some level
    assert vis.all() if view == "all_in_view" else 0.15 < 1.0 - vis.mean() < 0.6


@gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_clean_invisible_chained_equals_a_fresh_engine(oracle, form):
    """Two frame pairs without Set3Dpoints; in the second one a third of the points are outside the reference view and
    carry the first pair's patches and coefficients. With clean_invisible their Gx, Gy are zeroed, every term they add to
    H and b is an exact zero added at the same place of the same sum, and the chained engine equals a fresh engine that
    never saw pair 1, bit for bit, in the same form. Without the option it does not."""
    sc, _ = _plain_scene()
    shift = lambda p1: p1 + np.array([4.3, 0, 0, 0, 0, 0])
    chained = _device_run(oracle, sc, shift, form, 8, "clean", chain=sc["p_a"])
    p2 = chained.p0
    fresh = _device_run(oracle, dict(sc, img_a=sc["img_b"], img_b=sc["img_a"]), p2, form, 8, "clean")
    _same_tracking(chained, fresh, f"c/{form}/clean chained", bufs=False)
    ref = _numpy_run(oracle, ("chained", form, tuple(p2)), sc, p2, 8, "clean", swap=True)
    vr = ref.detail[0]["vis_ref"]
    assert 0.15 < 1.0 - vr.mean() < 0.6
    for w in (1, 2):
        assert np.array_equal(chained.bufs[w], fresh.bufs[w]), ("Gx / Gy", w)
        assert not chained.bufs[w][~vr].any()
    assert np.array_equal(chained.bufs[0][vr], fresh.bufs[0][vr])
    assert chained.bufs[0][~vr].any() and not fresh.bufs[0][~vr].any()  # the stale T is still there, and weighs nothing
    _against_numpy(chained, ref, 0, B_TOL_VIEW, f"c/{form}/clean chained, pair 2")
    quirk = _device_run(oracle, sc, shift, form, 8, "", chain=sc["p_a"], extra=ic.VARIANT_ANY_SIZE)
    assert np.array_equal(quirk.first, chained.first)
    assert rel(quirk.trace[0]["H"], chained.trace[0]["H"]) > 1e-3  # the stale patches are in the default's H


@gpu
def test_options_with_cloud_normalisation_and_a_coarse_last_level(oracle):
    """donorm = 1, lv_l = 1, {compose, huber}: the one-launch tracker against the graph form (no NumPy judge: the
    restatement has no cloud normalisation), both trace-checked."""
    sc, p0 = _plain_scene()
    runs = [_device_run(oracle, sc, p0, f, 8, "compose+huber", lv_l=1, donorm=1) for f in ("k_track1", "graph")]
    assert {lv for lv, _ in _seq(runs[0].trace)} == {2, 1}
    _between_forms(runs[0], runs[1], "c/k_track1~graph/donorm, lv_l=1/compose+huber")


# ------------------------------------------------------------------- (d) k_track1<false>: templates in global memory
@gpu
def test_one_launch_tracker_with_templates_in_global_memory(oracle):
    """900 points of 8x8 patches do not fit the LDS: k_track1<false> re-reads T, Gx, Gy from the patch buffers."""
    sc, p0 = _view_scene(900, 2.0)
    key = ("view", 900, 2.0)
    ref = _numpy_run(oracle, key, sc, p0, 8, "clean+huber")
    assert 0.15 < 1.0 - ref.detail[0]["vis_ref"].mean() < 0.6
    one = _device_run(oracle, sc, p0, "k_track1", 8, "clean+huber")
    assert "k_track1" in one.pr.odo.path_name()
    many = _device_run(oracle, sc, p0, "graph", 8, "clean+huber")
    _between_forms(one, many, "d/k_track1~graph/900 points/clean+huber")
    _against_numpy(one, ref, 0, B_TOL_VIEW, "d/k_track1/900 points/clean+huber")


# ----------------------------------------------------------------------------------------------------- (e) batches
def _batch(cam, op, variant, probs, pa, pb, which):
    e = ic.TrackBatch(cam, op, len(which))
    e.set_variant(variant)
    e.set_robust(**_robust("clean+compose+huber"))
    for k, j in enumerate(which):
        pts, p0 = probs[j]
        e.Set3Dpoints(k, np.ascontiguousarray(pts.copy()), pts.shape[1])
        e.SetPose(k, p0, pa, pb)
    e.track_async()
    return e, e.poses().copy(), e.iterations().copy()


@gpu
@pytest.mark.parametrize("form", ["k_track1", "graph"])
def test_batch_of_ragged_problems_with_every_option(oracle, form):
    """Five problems of 150, 1, 0, 97 and 150 points with distinct start poses, {clean, compose, huber} and patch
    normalisation. One-launch form: a problem gives the same bits whatever shares its launch (ictr_host.hip, "Always the
    same workgroup shape"). Graph form: the grid follows the largest problem, so sums to tolerance."""
    sc, p0 = _view_scene(150, 2.0)
    counts = [150, 1, 0, 97, 150]
    rng = np.random.default_rng(5)
    k1 = int(np.flatnonzero((sc["px_a"][:, 0] < 100) & (np.abs(sc["px_a"][:, 1] - 112) < 60))[0])  # stays in view
    first = {150: 0, 97: 0, 1: k1, 0: 0}
    probs = [(sc["pts3d"][:, first[c]:first[c] + c], p0 + rng.normal(0, 2e-3, 6)) for c in counts]
    op = ic.optparam(2, 0, 8, 5, 0.0, 0, 1, 150)
    cam = ic.CamClass(3, sc["fc"], sc["cc"], sc["wh"], 8)
    pa, pb = ic.Pyramid(sc["img_a"], 2, 8), ic.Pyramid(sc["img_b"], 2, 8)
    e, poses, iters = _batch(cam, op, FORMS[form][0], probs, pa, pb, range(5))
    _assert_form(form, e.path_name())
    assert np.isfinite(poses).all()
    assert np.array_equal(poses[2], np.asarray(probs[2][1], np.float32).astype(np.float64))  # no points: the start pose
    assert not np.array_equal(poses[0], poses[4])
    worst = 0.0
    for j in (0, 1, 3, 4):
        e1, p1, it1 = _batch(cam, op, FORMS[form][0], probs, pa, pb, [j])
        _assert_form(form, e1.path_name())
        if form == "k_track1":
            assert np.array_equal(poses[j], p1[0]) and iters[j] == it1[0], (j, np.abs(poses[j] - p1[0]).max())
        elif counts[j] > 1:
            worst = max(worst, np.abs(poses[j] - p1[0]).max())
            assert np.abs(poses[j] - p1[0]).max() <= FORM_POSE_TOL and iters[j] == it1[0], j
    print(f"[e/{form}] batch against the problems alone: pose {worst:.2e} (bar {FORM_POSE_TOL:.0e})")
    # the one-point problem is rank deficient: its last record (the problem's device state) solves its own H and b
    st = e.read_buffer(1, 8, 116)
    Hs, bs, dps = st[18:54].reshape(6, 6), st[104:110], st[110:116]
    assert Hs.any() and same_bits(dps, ic.solve6(Hs, bs)), (dps, ic.solve6(Hs, bs))
    # ... and so does every record of the same problem alone
    pts1, p01 = probs[1]
    one = _device_run(oracle, dict(sc, pts3d=np.ascontiguousarray(pts1)), p01, form, 8, "clean+compose+huber", dpn=1)
    assert np.isfinite(one.pose).all() and len(one.trace) >= 3 and one.trace[0]["H"].any()


# ---------------------------------------------------------------------------------------------------- (f) refusals
@gpu
@pytest.mark.parametrize("bad", [float("nan"), -1.0, float("-inf")])
def test_bad_huber_thresholds_are_refused(bad):
    sc = scene(128, 96, 20, seed=3)
    op = ic.optparam(1, 0, 8, 3, 0.0, 0, 0, 20)
    cam = ic.CamClass(2, sc["fc"], sc["cc"], sc["wh"], 8)
    for eng in (ic.TrackBatch(cam, op, 1), ic.OdometerClass(ic.PoseClass(cam, op), op)):
        with pytest.raises(ic.IctrError, match="Huber threshold"):
            eng.set_robust(huber_k=bad)
        eng.set_robust(huber_k=0.0)  # 0 is "off"


@gpu
@pytest.mark.parametrize("flags", ["clean", "compose", "huber"])
def test_image_only_reference_pyramids_refuse_the_options(flags):
    """getgrad = 2 pyramids hold no gradient planes; only the 8x8 setup kernel forms gradients on the fly, and it carries
    no option code."""
    sc = scene(W, H_, 60, seed=3, margin=16.0)
    op = ic.optparam(2, 0, 8, 3, 0.0, 0, 0, 60)
    cam = ic.CamClass(3, sc["fc"], sc["cc"], sc["wh"], 8)
    e = ic.TrackBatch(cam, op, 1)
    e.set_robust(**_robust(flags))
    e.Set3Dpoints(0, sc["pts3d"].copy())
    e.SetPose(0, sc["p_a"], ic.Pyramid(sc["img_a"], 2, 8, getgrad=2), ic.Pyramid(sc["img_b"], 2, 8, getgrad=0))
    with pytest.raises(ic.IctrError, match="on the fly"):
        e.track_async()
