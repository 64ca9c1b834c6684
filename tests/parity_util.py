"""Shared helpers for the GPU parity tests: run the same tracking through the HIP path (via the C-ABI) and
through the CPU oracle on identical inputs."""
import numpy as np

import invcompcamtrack_amd as ic
from invcompcamtrack_amd import synth


# OR-ed into every Pair's kernel-selection bits (tests/test_gpu_parity.py runs its cases once with the automatic
# choice -- small problems take the one-launch tracker k_track1 -- and once with bit 13 = per-iteration launches)
FORCE_VARIANT = 0
# (target, min, max) points for the one-launch tracker's team form (ictr_batch_set_team), or None = library defaults
FORCE_TEAM = None


class Pair:
    """One scene, one parameter set, both implementations wired like run_io_reprojection_test.cpp:189-193."""

    def __init__(self, O, sc, lv_f, lv_l, psz, maxiter, ratio, donorm, dpn, maxpt=None, variant=0):
        n = sc["pts3d"].shape[1]
        maxpt = n if maxpt is None else maxpt
        self.O, self.sc = O, sc
        self.oop = O.make_op(lv_f, lv_l, psz, maxiter, ratio, donorm, dpn, maxpt)
        self.opa, self.opb = O.Pyramid(sc["img_a"], lv_f, psz), O.Pyramid(sc["img_b"], lv_f, psz)
        self.otr = O.Tracker(self.oop, sc["fc"], sc["cc"], sc["wh"])
        self.op = ic.optparam(lv_f, lv_l, psz, maxiter, ratio, donorm, dpn, maxpt)
        self.cam = ic.CamClass(lv_f + 1, sc["fc"], sc["cc"], sc["wh"], psz)
        self.pose = ic.PoseClass(self.cam, self.op)
        self.odo = ic.OdometerClass(self.pose, self.op)
        self.odo.set_variant(variant | FORCE_VARIANT)
        if FORCE_TEAM is not None:
            self.odo.set_team(*FORCE_TEAM)
        self.odo.enable_trace()
        self.gpa, self.gpb = ic.Pyramid(sc["img_a"], lv_f, psz), ic.Pyramid(sc["img_b"], lv_f, psz)
        self.M = self.op.maxpttrack
        self.n = min(n, self.M)

    def set_points(self, pts=None):
        pts = self.sc["pts3d"] if pts is None else pts
        a, b = np.ascontiguousarray(pts.copy()), np.ascontiguousarray(pts.copy())
        self.otr.set3dpoints(a)
        self.odo.Set3Dpoints(b)
        return a, b

    def set_pose(self, p=None, swap=False):
        p = self.sc["p_a"] if p is None else p
        if swap:
            self.otr.setpose(p, self.opb, self.opa)
            self.odo.SetPose(p, self.gpb, self.gpa)
        else:
            self.otr.setpose(p, self.opa, self.opb)
            self.odo.SetPose(p, self.gpa, self.gpb)

    def track(self):
        self.p_start = self.pose.state()[0]  # the f32 pose the device starts from (check_solver_turns)
        self.p_final = self.odo.TrackPose()
        return self.otr.trackpose(), self.p_final


def rel(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()
    s = max(np.abs(a).max(), np.abs(b).max(), 1e-30)
    return d / s


def scene(w, h, n, seed, **kw):
    return synth.make_scene(w, h, n_points=n, seed=seed, **kw)


# ---------------------------------------------------------------------------------------------------------------
# The solver turn (tests/test_gpu_solver.py, tests/test_abi_cpu.py): a corpus of crafted 6x6 systems, a NumPy f32
# restatement of lu_factor_ws<6> / lu_apply_ws<6> (se3_math.h) that also reports what ictr_solve6 does not return,
# and the per-record consistency check of a device trace.
EPS32 = np.float32(1.1920929e-07)


def bits(a):
    """Raw 32-bit patterns of an f32 array, every NaN mapped to one pattern (any NaN equals any NaN)."""
    a = np.ascontiguousarray(a, np.float32)
    u = a.view(np.uint32).copy()
    u[np.isnan(a)] = 0x7FC00000
    return u


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def lu6_np(H):
    """lu_factor_ws<6> in NumPy f32 scalars. Returns dict(lu, rowsw, colsw, rowmap, colmap, nonzero, rank): the factors,
    the transpositions per step, their compositions (c[i] = b[rowmap[i]], x[i] = c[colmap[i]]) and the two counts."""
    N = 6
    A = np.array(H, np.float32).reshape(N, N).copy()
    rowsw, colsw = list(range(N)), list(range(N))
    nonzero, maxpiv = N, np.float32(0.0)
    with np.errstate(all="ignore"):
        for k in range(N):
            br = bc = k
            best = np.abs(A[k, k])
            for cc in range(k, N):
                for r in range(k, N):
                    v = np.abs(A[r, cc])
                    if v > best:
                        best, br, bc = v, r, cc
            if best == 0.0:
                nonzero = k
                break
            if best > maxpiv:
                maxpiv = best
            rowsw[k], colsw[k] = br, bc
            if br != k:
                A[[k, br], :] = A[[br, k], :]
            if bc != k:
                A[:, [k, bc]] = A[:, [bc, k]]
            if k < N - 1:
                pv = A[k, k]
                for r in range(k + 1, N):
                    A[r, k] = A[r, k] / pv
                for cc in range(k + 1, N):
                    for r in range(k + 1, N):
                        A[r, cc] = A[r, cc] - A[r, k] * A[k, cc]
        rank = 0
        if nonzero > 0:
            thr = maxpiv * (EPS32 * np.float32(N))
            rank = sum(1 for i in range(nonzero) if np.abs(A[i, i]) > thr)
    rowmap, colmap = list(range(N)), list(range(N))
    for k in range(N):
        rowmap[k], rowmap[rowsw[k]] = rowmap[rowsw[k]], rowmap[k]
    for k in range(N - 1, -1, -1):
        colmap[k], colmap[colsw[k]] = colmap[colsw[k]], colmap[k]
    return dict(lu=A, rowsw=rowsw, colsw=colsw, rowmap=np.array(rowmap, np.int32), colmap=np.array(colmap, np.int32),
                nonzero=nonzero, rank=rank)


def lu6_apply_np(f, b):
    """lu_apply_ws<6> with the factors of lu6_np."""
    N = 6
    A, rank = f["lu"], f["rank"]
    if f["nonzero"] == 0:
        return np.zeros(N, np.float32)
    c = np.array(b, np.float32)[f["rowmap"]]
    with np.errstate(all="ignore"):
        for i in range(N):
            for r in range(i + 1, N):
                c[r] = c[r] - c[i] * A[r, i]
        for i in range(N - 1, -1, -1):
            if i < rank:
                c[i] = c[i] / A[i, i]
                for r in range(i):
                    c[r] = c[r] - c[i] * A[r, i]
    c[rank:] = 0.0
    return c[f["colmap"]]


def _sym32(H):
    """f32, bit-symmetric (the lower triangle is a copy of the upper one)."""
    with np.errstate(all="ignore"):
        H = np.asarray(H).astype(np.float32)
    return np.where(np.tri(6, k=-1, dtype=bool), np.triu(H, 1).T, H)


def solver_corpus(seed=20240607):
    """[(class name, H (6,6) f32 bit-symmetric, b (6,) f32)]: a few thousand systems, every class of the solver test.
    Classes whose name starts with 'nonfinite' hold NaN / Inf; every other one is finite."""
    import itertools
    rng = np.random.default_rng(seed)
    out = []

    def add(name, H, b=None):
        b = rng.normal(size=6) if b is None else b
        with np.errstate(all="ignore"):
            out.append((name, _sym32(H), np.asarray(b).astype(np.float32)))

    def jtj(rows=None, J=None):
        J = rng.normal(size=(int(rng.integers(3, 41)) if rows is None else rows, 6)) if J is None else J
        return J.T @ J

    # J^T J of 3..40 random rows (rank 3, 4, 5 for fewer than 6 rows)
    for rows in range(3, 41):
        for _ in range(8):
            add("jtj", jtj(rows))
    # ... times 10^k: entries, pivots and the threshold product pass through f32 denormals and near overflow
    for k in range(-44, 31):
        for i in range(8):
            H = jtj(int(rng.integers(6, 41))) * 10.0 ** k
            b = rng.normal(size=6) * (10.0 ** k if i % 2 == 0 else 1.0)
            add(f"jtj*1e{k:+03d}", H, b)
    # exact rank r: 6 - r columns of J zeroed, every choice of columns
    for r in range(0, 6):
        for keep in itertools.combinations(range(6), r):
            for _ in range(3 if 1 < r < 5 else 4):
                J = rng.normal(size=(int(rng.integers(8, 41)), 6))
                J[:, [c for c in range(6) if c not in keep]] = 0.0
                add(f"rank{r}-zeroed", jtj(J=J))
    # rank-deficient without a zero row: duplicated / negated columns (the trailing pivots are rounding noise)
    for ndup in (1, 2, 3):
        for _ in range(40):
            J = rng.normal(size=(int(rng.integers(8, 41)), 6))
            cols = rng.permutation(6)
            for d in range(ndup):
                J[:, cols[2 * d + 1]] = J[:, cols[2 * d]] * (1.0 if rng.random() < 0.5 else -1.0)
            add(f"rank{6 - ndup}-dup", jtj(J=J))
    # pivots sitting on the threshold maxpivot * 6 * eps32 (strict comparison): below, on, above
    c6 = EPS32 * np.float32(6)
    one, step = np.float32(1), np.float32(2.0 ** -20)

    def around(thr):
        return (("below", np.float32(thr * (one - step))), ("on", np.float32(thr)),
                ("above", np.float32(thr * (one + step))))

    for m in (1.0, 3.7, 1e10, 1e-10, 12345.678, 2.0 ** 20):
        m = np.float32(m)
        for name, t in around(np.float32(m * c6)):
            for k in range(1, 6):  # the k-th pivot and all later ones sit at t
                for sign in (1.0, -1.0):
                    d = np.concatenate([m * rng.uniform(0.01, 1.0, k), np.full(6 - k, t)]).astype(np.float32)
                    d[0] = m
                    d[k:] *= np.float32(sign)
                    add(f"threshold-{name}-diag", np.diag(d[rng.permutation(6)]))
        for _ in range(4):  # a dense SPD 3x3 block holds maxpivot (its largest entry); three pivots at t
            J = rng.normal(size=(12, 3))
            B = J.T @ J
            B = (B * (float(m) / np.abs(B).max())).astype(np.float32)
            B = np.triu(B) + np.triu(B, 1).T
            for name, t in around(np.float32(np.abs(B).max() * c6)):
                H = np.zeros((6, 6), np.float32)
                idx = rng.permutation(6)
                H[np.ix_(idx[:3], idx[:3])] = B
                H[idx[3:], idx[3:]] = t
                add(f"threshold-{name}-block", H)
    # ties: the column-major first maximum decides; every row / column swap pattern
    for c in (1.0, -1.0, 0.5, 3.0, 1e-30, 1e30, 7.0):
        add("tie-cI", np.eye(6) * c, np.arange(1, 7))
    for _ in range(150):
        S = rng.choice([-1.0, 1.0], size=(6, 6))
        add("tie-equal-magnitude", S * float(rng.choice([1.0, 0.75, 3.0, 1e-20, 1e20])), rng.integers(-4, 5, 6))
    for hi in (1, 2, 3, 9):
        for _ in range(100):
            add(f"tie-integer-{hi}", rng.integers(-hi, hi + 1, size=(6, 6)), rng.integers(-9, 10, 6))
    for _ in range(60):  # the repeated maximum in the last row / column, on and off the diagonal
        H = rng.integers(-2, 3, size=(6, 6)).astype(np.float64)
        H[rng.integers(0, 6), 5] = 3.0 * rng.choice([-1.0, 1.0])
        H[5, 5] = 3.0 * rng.choice([-1.0, 1.0, 0.0])
        i = int(rng.integers(0, 5))
        H[i, i] = 3.0 * rng.choice([-1.0, 1.0, 0.0])
        add("tie-integer-last", H, rng.integers(-9, 10, 6))
    # symmetric indefinite and negative definite
    for _ in range(120):
        A = rng.normal(size=(6, 6))
        add("indefinite", A + A.T)
    for _ in range(80):
        add("negative-definite", -jtj())
    # non-finite values (values, not addresses)
    for bad, nm in ((np.nan, "nan"), (np.inf, "+inf"), (-np.inf, "-inf")):
        for k in range(6):
            for _ in range(3):
                H = jtj()
                H[k, k] = bad
                add(f"nonfinite-diag-{nm}", H)
        for _ in range(6):
            H = jtj()
            i, j = sorted(rng.choice(6, 2, replace=False))
            H[i, j] = H[j, i] = bad
            add(f"nonfinite-offdiag-{nm}", H)
        for k in range(6):
            b = rng.normal(size=6)
            b[k] = bad
            add(f"nonfinite-b-{nm}", jtj(), b)
    add("nonfinite-all-nan", np.full((6, 6), np.nan))
    add("nonfinite-all-nan", np.full((6, 6), np.nan), np.full(6, np.nan))
    return out


def finite_corpus(seed=20240607):
    return [s for s in solver_corpus(seed) if not s[0].startswith("nonfinite")]


def expected_level_records(levels, maxiter, ratio, normdp_of):
    """The (level, iter) records the loop rule of odometer.cpp:341-346 allows, given normdp_of(level, iter) -> the f32
    |dp|_1 of an executed iteration (None: not in the trace): iteration k + 1 exists iff k + 1 < maxiter and
    normdp_k / normdp_0 > ratio."""
    out = []
    ratio = np.float32(ratio)
    for lv in levels:
        it, nd, nd0 = 0, np.float32(1e-10), np.float32(1e-10)
        with np.errstate(all="ignore"):
            while it < maxiter and np.float32(nd / nd0) > ratio:
                nd = normdp_of(lv, it)
                out.append((lv, it))
                if nd is None:  # the trace ends where the rule wants another record
                    return out
                if it == 0:
                    nd0 = nd
                it += 1
    return out


def normdp32(dp):
    """|dp|_1 in Eigen's redux order for 6 coefficients, f32."""
    d = np.abs(np.asarray(dp, np.float32))
    with np.errstate(all="ignore"):
        return np.float32(np.float32(d[0] + np.float32(d[1] + d[2])) + np.float32(d[3] + np.float32(d[4] + d[5])))


def check_solver_turns(odo, p_start, op, p_final=None, compose=None, iterations=None):
    """Every record of the device trace is the serial solver turn on the device's own H and b, bit for bit.
    p_start: the f32 pose SetPose produced (PoseClass.state()[0] before TrackPose). p_final: what TrackPose returned.
    compose: None for the additive update; else (K, exp_d, log_d, exp_f, log_f) for G <- exp(dp) G, p = log(G), checked
    against the f64 composition with the factor K of tests/test_gpu_solver.py. iterations: the engine's count."""
    tr = odo.trace()
    by = {(r["level"], r["iter"]): r for r in tr}
    assert len(by) == len(tr), "a (level, iteration) recorded twice"
    want = expected_level_records(range(op.lv_f, op.lv_l - 1, -1), op.maxiter, op.normdp_ratio,
                                  lambda lv, it: normdp32(by[(lv, it)]["dp"]) if (lv, it) in by else None)
    assert [(r["level"], r["iter"]) for r in tr] == want, "the records are not those the loop rule allows"
    if iterations is not None:
        assert int(iterations) == len(tr), "get_iterations against the trace"
    p_prev = np.asarray(p_start, np.float32).copy()
    H_level = {}
    for r in tr:
        at = (r["level"], r["iter"])
        H, b, dp, p = r["H"], r["b"], r["dp"], r["p"]
        assert same_bits(H, H.T), ("H not bit-symmetric", at)
        if r["level"] in H_level:
            assert same_bits(H, H_level[r["level"]]), ("H changed inside a level", at)
        H_level[r["level"]] = H
        x = ic.solve6(H, b)
        assert same_bits(dp, x), ("dp is not the serial solve of the traced H, b", at, dp, x)
        if compose is None:
            with np.errstate(all="ignore"):
                assert same_bits(p, (p_prev + dp).astype(np.float32)), ("p != f32(p_prev + dp)", at)
        else:
            K, exp_d, log_d, exp_f, log_f = compose

            def comp(e, l, dt):
                G, D = np.eye(4, dtype=dt), np.eye(4, dtype=dt)
                G[:3] = np.asarray(e(p_prev.astype(dt))).reshape(3, 4)
                D[:3] = np.asarray(e(dp.astype(dt))).reshape(3, 4)
                return np.asarray(l(np.ascontiguousarray((D @ G)[:3].reshape(12).astype(dt))), np.float64)
            ref, host = comp(exp_d, log_d, np.float64), comp(exp_f, log_f, np.float32)
            bar = K * max(np.abs(host - ref).max(), float(EPS32) * max(1.0, np.abs(ref).max()))
            assert np.abs(p.astype(np.float64) - ref).max() <= bar, ("composed pose", at)
        p_prev = p
    if p_final is not None and tr:
        sp = odo.pose.state()[0] if hasattr(odo, "pose") else None
        if sp is not None:
            assert same_bits(sp, tr[-1]["p"]), "the pose state after TrackPose is not the last record's p"
        if not op.donorm:
            assert np.array_equal(np.asarray(p_final), tr[-1]["p"].astype(np.float64), equal_nan=True), \
                "TrackPose() is not the getpose image of the last record's p"
        elif sp is not None:
            assert np.array_equal(np.asarray(p_final), odo.pose.getPose_se3(), equal_nan=True)
    return tr


def device_wave_solve(Hs, bs, through_state):
    """ictr_debug_wave_solve on n systems: dict(x [n,6], rank [n], nonzero [n], rowmap [n,6], colmap [n,6], lu [n,6,6])."""
    from invcompcamtrack_amd import _lib
    H = np.ascontiguousarray(Hs, np.float32).reshape(-1, 36)
    b = np.ascontiguousarray(bs, np.float32).reshape(-1, 6)
    n = H.shape[0]
    assert b.shape[0] == n
    x, lu = np.empty((n, 6), np.float32), np.empty((n, 6, 6), np.float32)
    rank, nonzero = np.empty(n, np.int32), np.empty(n, np.int32)
    rowmap, colmap = np.empty((n, 6), np.int32), np.empty((n, 6), np.int32)
    ip = lambda a: a.ctypes.data_as(_lib.IP)
    _lib.check(_lib.load().ictr_debug_wave_solve(_lib.fp(H), _lib.fp(b), n, int(through_state), _lib.fp(x), ip(rank),
                                                 ip(nonzero), ip(rowmap), ip(colmap), _lib.fp(lu)))
    return dict(x=x, rank=rank, nonzero=nonzero, rowmap=rowmap, colmap=colmap, lu=lu)


def device_se3(inp, log_not_exp):
    """ictr_debug_se3: the device builds of se3_exp<float> (p [n,6] -> G [n,12]) / se3_log<float> (G -> p)."""
    from invcompcamtrack_amd import _lib
    a = np.ascontiguousarray(inp, np.float32).reshape(-1, 12 if log_not_exp else 6)
    out = np.empty((a.shape[0], 6 if log_not_exp else 12), np.float32)
    _lib.check(_lib.load().ictr_debug_se3(_lib.fp(a), a.shape[0], int(bool(log_not_exp)), _lib.fp(out)))
    return out
