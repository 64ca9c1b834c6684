"""The solver turn of the device (WaveSolver, ictr_devfn.h) against the serial full-pivot LU, bit for bit.

Layer 1: ws_factor / ws_apply (and the ws_store_factor / ws_load_factor round trip through ProbState) alone, on a corpus
  of crafted symmetric 6x6 systems (parity_util.solver_corpus), through ictr_debug_wave_solve. Judges: ic.solve6 (the
  host build of lu_factor_ws<6> / lu_apply_ws<6>), oracle.solve6 (the independent C restatement of Eigen's FullPivLU)
  and parity_util.lu6_np (NumPy f32; it also yields rank, nonzero, the composed permutations and the factors). x is
  compared as raw 32-bit patterns, any NaN equal to any NaN. A truth anchor that belongs to none of the three:
  |x - numpy.linalg.solve(H64, b64)|inf <= 8 cond2 eps32 |x|inf for the well-conditioned finite full-rank systems
  (the serial host solver's worst ratio err / (cond2 eps32 |x|inf) over such a corpus is 1.3, so 8 leaves the
  reference a margin of six and fails a solver that loses more than three bits beyond what conditioning explains).
  The device builds of se3_exp<float> / se3_log<float> (ictr_debug_se3) are held to the f64 instantiation on the host,
  per sample: |dev - f64|inf <= SE3_K max(|host_f32 - f64|inf, eps32 max(1, |value|inf)).
Layer 2: every launch form's trace solves its own H and b with those bits (parity_util.check_solver_turns), on scenes
  that drive the solver where the usual parity scenes do not: 1, 2, 3 points, stripes (an exactly zero row of H), a
  constant image, far points, and caller-made systems through the sharded phase API.
The tests without the gpu mark check the judges themselves on the CPU."""
import numpy as np
import pytest

import invcompcamtrack_amd as ic
import parity_util as pu
from parity_util import Pair, check_solver_turns, same_bits, scene

gpu = pytest.mark.gpu

# |dev - f64|inf / max(|host_f32 - f64|inf, eps32 max(1, |value|inf)), largest over the corpus as measured on the MI355X:
# exp 1.105 (293 of 299 samples bit-equal to the host f32 build), log 2.090 (268 of 290 bit-equal; the largest at a
# rotation by pi - 1e-3). Twice the larger, rounded up to a power of two:
SE3_K = 8.0

LAUNCHES, ONE_LAUNCH = ic.VARIANT_LAUNCHES, ic.VARIANT_ONE_LAUNCH
FORMS = {  # name -> (kernel-selection bits, team form of the one-launch tracker)
    "one_workgroup": (ONE_LAUNCH | ic.VARIANT_NO_TEAMS, None),
    "teams16": (ONE_LAUNCH, (16, 0, 1 << 30)),
    "graph": (LAUNCHES, None),
    "no_graph": (LAUNCHES | ic.VARIANT_NO_GRAPH, None),
    "any_size": (LAUNCHES | ic.VARIANT_ANY_SIZE, None),
    "h_by_setup": (LAUNCHES | ic.VARIANT_H_BY_SETUP, None),
}


@pytest.fixture(scope="module")
def corpus():
    return pu.solver_corpus()


# ------------------------------------------------------------------------------------------------ the judges, on the CPU
def test_numpy_restatement_reproduces_the_host_solver(oracle, corpus):
    """lu6_np / lu6_apply_np (the judge of rank, nonzero, rowmap, colmap and the factors below) give ic.solve6's and
    oracle.solve6's bits on every system of the corpus, the non-finite classes included."""
    bad = []
    for name, H, b in corpus:
        assert same_bits(H, H.T), name
        x = pu.lu6_apply_np(pu.lu6_np(H), b)
        if not (same_bits(x, ic.solve6(H, b)) and same_bits(x, oracle.solve6(H, b))):
            bad.append(name)
    assert not bad, bad
    assert 2000 <= len(corpus) <= 5000


def test_corpus_reaches_every_pivot_pattern(corpus):
    """The corpus is only as good as the decisions it forces: every rank and non-zero-pivot count, every row / column
    swap pattern at every step, swaps that undo earlier ones, and thresholds that decide."""
    seen, ranks, nonzeros, undo = set(), set(), set(), 0
    for name, H, b in corpus:
        if name.startswith("nonfinite"):
            continue
        f = pu.lu6_np(H)
        ranks.add(f["rank"])
        nonzeros.add(f["nonzero"])
        for k in range(min(f["nonzero"], 5)):
            seen.add((k, f["rowsw"][k] == k, f["colsw"][k] == k))
        rs = [f["rowsw"][k] for k in range(f["nonzero"]) if f["rowsw"][k] != k]
        undo += any(b2 == b1 for b1, b2 in zip(rs, rs[1:]))
        if name.startswith("threshold-"):
            d = np.abs(np.diag(f["lu"]))
            k = int((d > d.max() * 1e-5).sum())  # pivots well above the threshold
            assert f["nonzero"] == 6 and 1 <= k <= 5
            assert f["rank"] == (6 if "above" in name else k), (name, f["rank"], k)
        if name.startswith("rank") and name.endswith("zeroed"):
            assert f["nonzero"] == f["rank"] == int(name[4]), name
        if name.endswith("-dup"):
            assert f["rank"] <= int(name[4]) < 6, name
    assert ranks == set(range(7)) and nonzeros == set(range(7))
    # (step 0 of a symmetric matrix cannot keep its row and change its column: the scan meets |H[c][0]| before |H[0][c]|)
    assert seen == {(k, r, c) for k in range(5) for r in (False, True) for c in (False, True)} - {(0, True, False)}
    assert undo > 20


def _normal_entries(H):
    """finite, and every entry a normal f32 number or an exact zero"""
    H64 = H.astype(np.float64)
    return bool(np.isfinite(H64).all() and (np.abs(H64[H64 != 0.0]) >= np.finfo(np.float32).tiny).all())


def _truth_anchor(corpus, X):
    """Returns (number of systems checked, worst err / (cond2 eps32 |x|inf), failures)."""
    worst, n, bad = 0.0, 0, []
    for (name, H, b), x in zip(corpus, X):
        if name.startswith("nonfinite") or not _normal_entries(H) or not np.isfinite(b).all():
            continue
        H64, b64 = H.astype(np.float64), b.astype(np.float64)
        keep = np.arange(6)
        if name.startswith("rank") and name.endswith("zeroed"):
            keep = np.flatnonzero(np.abs(H64).sum(0) != 0.0)
            free = np.setdiff1d(np.arange(6), keep)
            if not np.array_equal(x[free].view(np.uint32), np.zeros(len(free), np.uint32)):
                bad.append((name, "free variables not +0", x))
            if len(keep) == 0:
                continue
            H64, b64 = H64[np.ix_(keep, keep)], b64[keep]
        elif pu.lu6_np(H)["rank"] < 6:
            continue
        cond = np.linalg.cond(H64, 2)
        if not cond <= 1e4:
            continue
        ref = np.linalg.solve(H64, b64)
        xs = x[keep].astype(np.float64)
        if not np.isfinite(xs).all():
            if np.abs(ref).max() < 1e38:
                bad.append((name, "not finite", x))
            continue
        ratio = np.abs(xs - ref).max() / (cond * float(pu.EPS32) * np.abs(xs).max())
        worst, n = max(worst, ratio), n + 1
        if not ratio <= 8.0:
            bad.append((name, ratio, cond))
    return n, worst, bad


def test_truth_anchor_holds_for_the_host_solver(corpus):
    """The anchor's own margin: the serial host solver stays below 8 by a factor of about six."""
    n, worst, bad = _truth_anchor(corpus, [ic.solve6(H, b) for _, H, b in corpus])
    print(f"truth anchor, host solver: {n} systems, worst ratio {worst:.3f}")
    assert not bad, bad[:5]
    assert n >= 1000 and worst <= 2.0


def _stripes(horizontal):
    sc = scene(256, 224, 150, seed=7, margin=16.0)
    f = lambda x: 128.0 + 60.0 * np.sin(0.21 * x) + 40.0 * np.sin(0.057 * x + 1.0)
    yy, xx = np.mgrid[0:224, 0:256].astype(np.float64)
    t = yy if horizontal else xx
    sc["img_a"], sc["img_b"] = f(t).astype(np.float32), f(t + 1.3).astype(np.float32)
    return sc


def _check_null_parameter(tr, null):
    zero = np.zeros(6, np.uint32)
    for r in tr:
        H = np.ascontiguousarray(r["H"])
        assert np.array_equal(H[null].view(np.uint32), zero) and np.array_equal(H.T[null].copy().view(np.uint32), zero)
        assert r["dp"][null:null + 1].view(np.uint32)[0] == 0 and np.isfinite(r["dp"]).all()
    assert np.abs(np.delete(tr[0]["dp"], null)).max() > 1e-3  # the other components move


@pytest.mark.parametrize("horizontal", [False, True])
def test_stripes_give_an_exactly_zero_row_in_the_oracle(oracle, horizontal):
    """I(x, y) = f(x): the dy plane is exactly 0 at every level, so row and column 1 (t_y) of H are all-zero bits in any
    summation order, dp[1] == +0 in every record and solve6(H, b) == dp; f(y): the same for parameter 0 (t_x)."""
    sc = _stripes(horizontal)
    oop = oracle.make_op(2, 0, 8, 5, 0.0, 0, 0, 150)
    tr = oracle.Tracker(oop, sc["fc"], sc["cc"], sc["wh"])
    tr.set3dpoints(sc["pts3d"].copy())
    tr.setpose(sc["p_a"], oracle.Pyramid(sc["img_a"], 2, 8), oracle.Pyramid(sc["img_b"], 2, 8))
    tr.trackpose()
    recs = tr.trace()
    assert len(recs) == 15
    _check_null_parameter(recs, 0 if horizontal else 1)
    for r in recs:
        assert same_bits(r["dp"], oracle.solve6(r["H"], r["b"])) and same_bits(r["dp"], ic.solve6(r["H"], r["b"]))


# ------------------------------------------------------------------------------------------------ layer 1 on the device
@pytest.fixture(scope="module")
def device_solves(corpus):
    Hs, bs = np.stack([H for _, H, _ in corpus]), np.stack([b for _, _, b in corpus])
    return [pu.device_wave_solve(Hs, bs, ts) for ts in (0, 1)]


@gpu
@pytest.mark.parametrize("through_state", [0, 1])
def test_wave_solver_gives_the_serial_bits(oracle, corpus, device_solves, through_state):
    """ws_factor -> ws_apply in registers (0) and ws_factor -> ws_store_factor -> second launch -> ws_load_factor ->
    ws_apply (1): x, rank, nonzero, the composed permutations and the 36 factors of every system of the corpus."""
    d = device_solves[through_state]
    bad = {}
    for i, (name, H, b) in enumerate(corpus):
        f = pu.lu6_np(H)
        what = []
        if not same_bits(d["x"][i], ic.solve6(H, b)):
            what.append("x vs ic.solve6")
        if not same_bits(d["x"][i], oracle.solve6(H, b)):
            what.append("x vs oracle.solve6")
        if (d["rank"][i], d["nonzero"][i]) != (f["rank"], f["nonzero"]):
            what.append(f"rank/nonzero {d['rank'][i]}/{d['nonzero'][i]} vs {f['rank']}/{f['nonzero']}")
        if not (np.array_equal(d["rowmap"][i], f["rowmap"]) and np.array_equal(d["colmap"][i], f["colmap"])):
            what.append("rowmap/colmap")
        if not same_bits(d["lu"][i], f["lu"]):
            what.append("LU")
        if what:
            bad.setdefault(name.split("*")[0], []).append((i, name, what))
    report = {k: (len(v), v[0]) for k, v in bad.items()}
    print("classes that differ:", report)
    assert not bad, report


@gpu
def test_wave_solver_is_the_same_through_the_problem_record(device_solves):
    a, b = device_solves
    for k in ("x", "lu"):
        assert same_bits(a[k], b[k]), k
    for k in ("rank", "nonzero", "rowmap", "colmap"):
        assert np.array_equal(a[k], b[k]), k


@gpu
@pytest.mark.parametrize("through_state", [0, 1])
def test_wave_solver_meets_the_truth_anchor(corpus, device_solves, through_state):
    n, worst, bad = _truth_anchor(corpus, device_solves[through_state]["x"])
    print(f"truth anchor, device solver: {n} systems, worst ratio {worst:.3f}")
    assert not bad, bad[:5]
    assert n >= 1000


def _se3_corpus():
    rng = np.random.default_rng(0)
    ps = []
    for _ in range(200):  # the poses of test_abi_cpu.py's loop
        scale = 10.0 ** rng.integers(-6, 1)
        ps.append(rng.normal(0, 1, 6) * np.array([2, 2, 2, scale, scale, scale]))
        rng.normal(size=(12, 6)), rng.normal(size=6)  # (that loop's other draws)
    exp_only = []
    for th in (0.0, 1e-11, 1e-5, 0.99e-4, 1e-4, 1.01e-4, 1.0, np.pi / 2, np.pi - 1e-3, np.pi - 1e-6, 1.5 * np.pi):
        axes = [rng.normal(size=3) for _ in range(6)] + list(np.eye(3))
        for ax in axes:
            p = np.concatenate([rng.normal(0, 1, 3), ax / np.linalg.norm(ax) * th])
            (exp_only if th > np.pi else ps).append(p)
    return np.array(ps).astype(np.float32), np.array(ps + exp_only).astype(np.float32)


@gpu
def test_device_exp_and_log_against_the_f64_build():
    """se3_exp<float> / se3_log<float> as compiled for the device (its sincosf, acosf, tanf are not glibc's) against the
    f64 instantiation on the host (pinned to scipy's expm / logm by the oracle KATs), per sample with the host f32
    build's own error as the yardstick. Bit equality with the host f32 build is recorded, not required."""
    p_log, p_exp = _se3_corpus()
    bad = []
    for kind, inp in (("exp", p_exp), ("log", np.stack([ic.util_SE3_coeff_to_group(p) for p in p_log]))):
        fn = ic.util_SE3_coeff_to_group if kind == "exp" else ic.util_SE3_group_to_coeff
        dev = pu.device_se3(inp, kind == "log")
        worst, equal, outside = (0.0, -1), 0, 0
        for i, a in enumerate(inp):
            ref = np.asarray(fn(a.astype(np.float64)), np.float64).reshape(-1)
            host = np.asarray(fn(a), np.float32).reshape(-1)
            equal += same_bits(host, dev[i])
            if not np.isfinite(ref).all():
                # The rounded matrix lies outside the logarithm's domain: 0.5 (trace - 1) < -1 in f64 (se3_log does
                # not clamp, like the reference). In f32 that argument is the same bits on host and device (plain
                # products and sums, no contraction), so both are NaN together or both landed on -1 exactly; nothing
                # is excluded: where finite, the device is held to the host f32 build itself.
                assert kind == "log" and np.abs(a[0] + a[5] + a[10] + 1.0) < 1e-5, (kind, i, a)
                outside += 1
                ok = np.array_equal(np.isnan(host), np.isnan(dev[i]))
                fin = np.isfinite(host)
                yard = float(pu.EPS32) * max(1.0, np.abs(host[fin]).max()) if fin.any() else 1.0
                ratio = np.abs(dev[i][fin].astype(np.float64) - host[fin]).max() / yard if fin.any() else 0.0
                if not (ok and ratio <= SE3_K):
                    bad.append((kind, i, a, ratio, host, dev[i]))
                continue
            yard = max(np.abs(host.astype(np.float64) - ref).max(), float(pu.EPS32) * max(1.0, np.abs(ref).max()))
            ratio = np.abs(dev[i].astype(np.float64) - ref).max() / yard
            worst = max(worst, (ratio, i))
            if not ratio <= SE3_K:
                bad.append((kind, i, a, ratio))
        print(f"se3_{kind}: {len(inp)} samples, worst ratio {worst[0]:.3f} (sample {worst[1]}: {inp[worst[1]]}), "
              f"bit-equal to the host f32 build: {equal} of {len(inp)}, outside the domain: {outside}")
        assert outside <= 9  # (rotations by pi - 1e-6 only)
    assert not bad, bad[:5]


# ------------------------------------------------------------------------------------------------ layer 2: the launch forms
def _run(oracle, sc, form, psz, pts=None, lv_f=2, maxiter=5, ratio=0.0, donorm=0, with_oracle=False, robust=None):
    variant, team = FORMS[form]
    pts = sc["pts3d"] if pts is None else pts
    pr = Pair(oracle, dict(sc, pts3d=pts), lv_f, 0, psz, maxiter, ratio, donorm, 0, variant=variant)
    if team is not None:
        pr.odo.set_team(*team)
    if robust:
        pr.odo.set_robust(**robust)
    pr.odo.Set3Dpoints(np.ascontiguousarray(pts.copy()))
    pr.odo.SetPose(sc["p_a"], pr.gpa, pr.gpb)
    p_start = pr.pose.state()[0]
    if not donorm:
        assert same_bits(p_start, np.asarray(sc["p_a"], np.float32))  # host_setpose stores float32(p_in)
    pg = pr.odo.TrackPose()
    compose = None
    if robust and robust.get("compositional"):
        e, l = ic.util_SE3_coeff_to_group, ic.util_SE3_group_to_coeff
        compose = (SE3_K, e, l, e, l)
    tr = check_solver_turns(pr.odo, p_start, pr.op, p_final=pg, compose=compose)
    if with_oracle:
        pr.otr.set3dpoints(np.ascontiguousarray(pts.copy()))
        pr.otr.setpose(sc["p_a"], pr.opa, pr.opb)
        pr.otr.trackpose()
    return pr, tr, pg


@gpu
@pytest.mark.parametrize("psz", [8, 4, 5])
@pytest.mark.parametrize("form", list(FORMS))
def test_few_points_solve_their_own_system(oracle, form, psz):
    """1, 2 and 3 points: mathematical rank 2, 4, 6 -- the trailing pivots are rounding noise and the threshold decides.
    Whatever the device's sums are, its dp must be the serial solve of its own H and b."""
    sc = scene(256, 224, 12, seed=23 + psz, margin=40.0)
    for n in (1, 2, 3):
        pr, tr, pg = _run(oracle, sc, form, psz, pts=sc["pts3d"][:, :n].copy(), ratio=0.01 if n == 2 else 0.0)
        assert len(tr) >= 3 and tr[0]["H"].any()
        assert all(pu.lu6_np(r["H"])["rank"] <= 2 * n for r in tr)


@gpu
@pytest.mark.parametrize("horizontal", [False, True])
@pytest.mark.parametrize("form", list(FORMS))
def test_stripes_leave_one_parameter_exactly_alone(oracle, form, horizontal):
    """Vertical stripes: row and column 1 of H are exactly 0 in every launch form's summation order, the solver stops at
    five non-zero pivots and dp[1] is +0 in every record; horizontal stripes: parameter 0. The first dp agrees with the
    oracle's to the bar of test_gpu_parity.py's _check_trace."""
    pr, tr, pg = _run(oracle, _stripes(horizontal), form, 8, with_oracle=True)
    null = 0 if horizontal else 1
    assert len(tr) == 15
    _check_null_parameter(tr, null)
    assert all(pu.lu6_np(r["H"])["nonzero"] == 5 for r in tr)
    o = pr.otr.trace()[0]
    assert np.abs(o["dp"] - tr[0]["dp"]).max() <= 2e-3 * np.abs(o["dp"]).max(), "first dp"
    assert pg[null] == np.float32(pr.sc["p_a"][null])


@gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_constant_image_moves_nothing(oracle, form):
    """H == 0 through the gradients (not through visibility): dp == 0 in every record, the pose is float32(p_in)."""
    sc = scene(256, 224, 60, seed=5, margin=16.0)
    sc["img_a"] = np.full((224, 256), 97.0, np.float32)
    sc["img_b"] = np.full((224, 256), 97.0, np.float32)
    pr, tr, pg = _run(oracle, sc, form, 8, ratio=0.01)
    assert len(tr) == 3  # one iteration per level: normdp / normdp_init = 0 / 0 is not > ratio
    for r in tr:
        assert not r["H"].any() and np.array_equal(r["dp"].view(np.uint32), np.zeros(6, np.uint32))
    assert np.array_equal(pg, np.asarray(sc["p_a"], np.float32).astype(np.float64))


def _far_scene():
    from invcompcamtrack_amd import synth
    return synth.make_scene(256, 224, n_points=200, seed=77, margin=16.0, depth=1e4,
                            dp_gt=np.array([30.0, -20.0, 40.0, 0.004, -0.003, 0.005]))


@gpu
@pytest.mark.parametrize("donorm", [0, 1])
@pytest.mark.parametrize("form", list(FORMS))
def test_far_points_pivot_late_and_swap_columns(oracle, form, donorm):
    """Points 1e3 times farther than the scene's default: the translation and rotation blocks of H differ by orders of
    magnitude (late pivots, column swaps), with and without the cloud normalisation."""
    pr, tr, pg = _run(oracle, _far_scene(), form, 8, donorm=donorm, ratio=0.01, maxiter=6)
    f = pu.lu6_np(tr[0]["H"])
    assert any(f["colsw"][k] != k for k in range(6))
    if not donorm:
        d = np.abs(np.diag(tr[0]["H"]))
        assert d[3:].min() > 1e4 * d[:3].max()


@gpu
@pytest.mark.parametrize("form", ["one_workgroup", "graph"])
def test_compositional_update_is_the_composition_of_its_own_dp(oracle, form):
    """ICTR_ROBUST_COMPOSE: dp is still the serial solve of the traced H and b; p = log(exp(dp) G) to the f64 composition
    with the factor of the exp / log test."""
    sc = scene(256, 224, 150, seed=41, margin=16.0)
    _run(oracle, sc, form, 8, robust=dict(compositional=True))


@gpu
def test_resident_form_solves_its_own_system(oracle):
    """>= 8193 points: k_level_resident, whose solver workgroup factors H and iterates inside the level's launch."""
    sc = scene(256, 224, 8200, seed=12, margin=12.0)
    op = ic.optparam(2, 0, 8, 5, 0.01, 0, 0, 8200)
    cam = ic.CamClass(3, sc["fc"], sc["cc"], sc["wh"], 8)
    pose = ic.PoseClass(cam, op)
    odo = ic.OdometerClass(pose, op)
    odo.enable_trace()
    pa, pb = ic.Pyramid(sc["img_a"], 2, 8), ic.Pyramid(sc["img_b"], 2, 8)
    odo.Set3Dpoints(sc["pts3d"].copy())
    odo.SetPose(sc["p_a"], pa, pb)
    p_start = pose.state()[0]
    pg = odo.TrackPose()
    tr = check_solver_turns(odo, p_start, op, p_final=pg)
    assert len(tr) >= 3 and np.abs(pg - sc["p_b"]).max() < 5e-3
    # the same problem in a batch says which form ran
    b = ic.TrackBatch(cam, op, 1)
    b.Set3Dpoints(0, sc["pts3d"].copy())
    b.SetPose(0, sc["p_a"], pa, pb)
    b.track_async()
    assert np.array_equal(b.poses()[0], pg) and "k_level_resident" in b.path_name()
    assert int(b.iterations()[0]) == len(tr)


@gpu
def test_both_register_budgets_of_the_one_launch_tracker_solve_alike(oracle):
    """k_track1_p8's 128-register build (a batch with more problems than the chip has CUs) against its large build (the
    same problems alone, each trace-checked record by record): identical poses and iteration counts, so the small
    build's solver turn is the serial one too. Problems of 1, 2, 3 and 25..40 points."""
    sc = scene(320, 240, 40, seed=61)
    op = ic.optparam(3, 0, 8, 5, 0.01, 0, 0, 40)
    cam = ic.CamClass(4, sc["fc"], sc["cc"], sc["wh"], 8)
    pa, pb = ic.Pyramid(sc["img_a"], 3, 8), ic.Pyramid(sc["img_b"], 3, 8)
    B = 300
    poses = sc["p_a"][None, :] + np.random.default_rng(8).normal(0, 2e-3, (B, 6))
    npts = [(1, 2, 3)[i % 3] if i < 12 else 25 + i % 16 for i in range(B)]
    b = ic.TrackBatch(cam, op, B)
    for k in range(B):
        b.Set3Dpoints(k, np.ascontiguousarray(sc["pts3d"][:, :npts[k]].copy()))
    b.SetPoseAll(poses, pa, pb)
    b.track_async()
    got, iters = b.poses().copy(), b.iterations().copy()
    assert "k_track1" in b.path_name()
    for k in (0, 1, 2, 3, 4, 5, 12, 13, 100, 299):
        pose = ic.PoseClass(cam, op)
        odo = ic.OdometerClass(pose, op)
        odo.set_variant(ONE_LAUNCH | ic.VARIANT_NO_TEAMS)
        odo.enable_trace()
        odo.Set3Dpoints(np.ascontiguousarray(sc["pts3d"][:, :npts[k]].copy()))
        odo.SetPose(poses[k], pa, pb)
        p_start = pose.state()[0]
        pg = odo.TrackPose()
        check_solver_turns(odo, p_start, op, p_final=pg, iterations=iters[k])
        assert np.array_equal(pg, got[k]), k


def _corpus_pick(corpus, prefix, want=lambda f: True):
    for name, H, b in corpus:
        if name.startswith(prefix) and np.abs(ic.solve6(H, b)).max() < 50.0 and want(pu.lu6_np(H)):
            return name, H, b
    raise AssertionError(prefix)


@gpu
@pytest.mark.parametrize("psz,variant", [(8, 0), (8, ic.VARIANT_H_BY_SETUP), (4, 0), (5, 0)])
def test_sharded_finish_solves_what_the_caller_reduced(oracle, corpus, psz, variant):
    """The sharded phase API hands the caller's all-reduced 27 floats to k_level_finish / k_iter_finish (ws_factor on
    the adopted H -- with the first b where H is deferred --, ws_store_factor, ws_load_factor in the later iterations).
    Overwritten with corpus systems, p_in = 0 and no normalisation, the pose after k iterations is k additions of
    solve6(H, b) in f32."""
    import torch
    from invcompcamtrack_amd.dist import RED_STRIDE
    assert RED_STRIDE == 27
    sc = scene(256, 224, 60, seed=9, margin=float(max(12, psz + 9)))
    cam = ic.CamClass(1, sc["fc"], sc["cc"], sc["wh"], psz)
    pa, pb = ic.Pyramid(sc["img_a"], 0, psz), ic.Pyramid(sc["img_b"], 0, psz)
    iu = np.triu_indices(6)
    picks = [_corpus_pick(corpus, "rank3-zeroed"), _corpus_pick(corpus, "tie-integer-last"),
             _corpus_pick(corpus, "threshold-on-block"), _corpus_pick(corpus, "threshold-above-block"),
             _corpus_pick(corpus, "rank4-dup"),
             _corpus_pick(corpus, "jtj", lambda f: any(c != k for k, c in enumerate(f["colsw"]))),
             _corpus_pick(corpus, "indefinite")]
    seen_defer = set()
    for maxiter in (1, 2):
        op = ic.optparam(0, 0, psz, maxiter, 0.0, 0, 0, 60)
        for name, H, b in picks:
            e = ic.TrackBatch(cam, op, 1)
            e.set_variant(variant)
            e.enable_sharding(True)
            red = torch.zeros(RED_STRIDE, dtype=torch.float32, device="cuda")
            e.set_reduction_buffer(red.data_ptr())
            e.Set3Dpoints(0, sc["pts3d"].copy())
            e.SetPose(0, np.zeros(6), pa, pb)
            e.begin()
            e.level_accumulate(0)
            torch.cuda.synchronize()
            mine = np.zeros(RED_STRIDE, np.float32)
            mine[:21] = H[iu]
            defer = not e.needs_level_allreduce  # H rides with the first b
            seen_defer.add(defer)
            if not defer:
                red.copy_(torch.from_numpy(mine))
                torch.cuda.synchronize()
            e.level_finish(0)
            x = np.zeros(6, np.float32)
            for it in range(maxiter):
                e.iter_accumulate(0)
                torch.cuda.synchronize()
                mine[21:] = b
                if not (defer and it == 0):
                    mine[:21] = 0.0
                red.copy_(torch.from_numpy(mine))
                torch.cuda.synchronize()
                e.iter_finish(0)
                with np.errstate(all="ignore"):
                    x = (x + ic.solve6(H, b)).astype(np.float32)
            got = e.poses()[0]
            assert np.array_equal(got, x.astype(np.float64), equal_nan=True), (name, maxiter, got, x)
            assert int(e.iterations()[0]) == maxiter
    assert seen_defer == {psz != 5 and not variant}
