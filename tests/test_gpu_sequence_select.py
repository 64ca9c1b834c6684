"""The between-pairs selection of a sequence (k_seq_select_count / _scatter / _finish) across workgroup bounds, cap
limits and the cull's edges: every case of tests/seq_select_cases.py on two frames with maxiter = 0, read back with
SequenceTracker.last_selection and compared with select_points (integers) and with the f64 restatement of the finish
kernel's sums (bits); then one real tracking chain over a world of four workgroups against the host loop."""
import numpy as np
import pytest

import invcompcamtrack_amd as ic
from invcompcamtrack_amd import sequence as sq
import seq_select_cases as sc
from seq_scene import bound_margin, make_pan

pytestmark = pytest.mark.gpu

RUNS = [r + (donorm,) for r in sc.runs() for donorm in (0, 1)]
P_OTHER = np.array([0.3, -0.2, 0.1, 0.02, -0.03, 0.01])  # the run in between: another keep pattern in every buffer


@pytest.fixture(scope="module")
def frames():
    """Two frames of any texture: with maxiter = 0 their content does not reach the selection."""
    return np.random.default_rng(7).uniform(0, 255, (2, sc.H, sc.W)).astype(np.float32)


def _setup(form, cap, donorm, camd):
    op = ic.optparam(1, 0, sc.PSZ[form], 0, 0.01, donorm, 1, cap)
    assert op.maxpttrack == cap
    return op, ic.CamClass(2, camd["fc"], camd["cc"], camd["wh"], 8)


def _run(st, frames, p0):
    st.track_async(frames, p0)
    r = st.wait()
    r["hash"] = st.selection_hashes()
    last = st.last_selection()
    r["last_npts"] = last.pop("npts")
    r.update(last)
    return r


def _bytes(r):
    """Everything a run gives back (a NaN as the device wrote it: the same code gives the same NaN)."""
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in ("poses", "npts", "iters", "hash", "sel", "ms", "pt3d")) \
        + np.float64(r["varval"]).tobytes() + np.int64(r["last_npts"]).tobytes()


@pytest.mark.parametrize("case,stride,form,cap,donorm", RUNS,
                         ids=["%s-s%d-%s%d-n%d" % r for r in RUNS])
def test_selection_state(frames, case, stride, form, cap, donorm):
    wd = sc.world(sc.TABLE[case][0])
    X, p0 = wd["X"], wd["p0"]
    op, cam = _setup(form, cap, donorm, wd["cam"])
    want = sc.expected(case, stride, cap)
    n = want.size
    st = sq.SequenceTracker(cam, op, X, stride)
    r = _run(st, frames, p0)
    assert (st.last_team > 1) == (form == sc.TEAM)
    M = op.maxpttrack
    print("%s stride %d %s cap %d donorm %d: nblk %d survivors %d npts %d" % (
        case, stride, form, cap, donorm, sc.nblk(X.shape[1]), sc.survivors(case).size, r["npts"][0]))
    # the selection: integers
    assert r["npts"].tolist() == [n] and r["last_npts"] == n
    np.testing.assert_array_equal(r["sel"], want.astype(np.int32))
    assert int(r["hash"][0]) == sq.selection_hash(want)
    assert r["iters"].tolist() == [0]
    np.testing.assert_array_equal(r["poses"][0], p0)
    # the normalisation: the restated order, in the bits
    if donorm and n > 0:
        ms, varval = sc.finish_sums(X, want)
    else:
        ms, varval = np.zeros(3), 1.0
    assert r["ms"].tobytes() == np.asarray(ms, np.float64).tobytes(), (r["ms"], ms)
    assert np.float64(r["varval"]).tobytes() == np.float64(varval).tobytes(), (r["varval"], varval)
    # the f32 points from the device's own ms and varval: correctly rounded f64 operations and one cast
    # (one selected point under donorm: varval is exactly 0, as Set3Dpoints' is, and the point and the pose's
    # translation are 0 / 0 on the device as on the host; a NaN's sign and payload are not pinned)
    P = X[:, want]
    with np.errstate(invalid="ignore"):
        pts = ((P - r["ms"][:, None]) / r["varval"]).astype(np.float32) if donorm else P.astype(np.float32)
    assert r["pt3d"].shape == (3, M)
    assert np.isnan(pts).any() == bool(donorm and n == 1)
    got = r["pt3d"][:, :n]
    np.testing.assert_array_equal(np.isnan(got), np.isnan(pts))
    assert got[~np.isnan(pts)].tobytes() == pts[~np.isnan(pts)].tobytes()
    assert not r["pt3d"][:, n:].any() and not np.signbit(r["pt3d"][:, n:]).any()
    # the pose handed through the (untouched) tracking: the setpose / getpose round trip on the host
    if n == 0:
        assert r["poses"][1].tobytes() == np.asarray(p0, np.float64).tobytes()
    else:
        pose = ic.PoseClass(cam, op)
        pose.setpose_se3(p0, r["ms"], r["varval"])
        back = pose.getPose_se3()
        got = r["poses"][1]
        ok = ~np.isnan(back)
        assert ok.all() or (donorm and n == 1)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(back))
        assert np.all(np.abs(got - back)[ok] <= np.maximum(1e-6 * np.abs(back), 1e-9)[ok]), (got, back)
    # the same tracker again, behind a run that leaves another pose's masks, counts and indices in the buffers
    _run(st, frames, P_OTHER if not np.any(p0) else np.zeros(6))
    again = _run(st, frames, p0)
    assert _bytes(again) == _bytes(r)


CHAIN = {  # the option sets of test_gpu_sequence.py; strides that put fewer than the cap into every pair of this world
    "p8_single": ((4, 0, 8, 10, 0.01, 1, 1), 128, 40, "single"),
    "p8_team": ((4, 0, 8, 10, 0.01, 1, 1), 400, 13, "team"),
}
CHAIN_SEED = 5  # bound_margin > 1e-3 px at the six ground-truth poses (4.8e-3)


@pytest.fixture(scope="module")
def pan():
    return make_pan(640, 480, 6, 3 * sc.C + 37, step=-0.5, seed=CHAIN_SEED, tilt=0.5)


@pytest.mark.parametrize("name", list(CHAIN))
def test_chain_over_four_workgroups_equals_host_loop(pan, name):
    """Real tracking: each pair's selection is drawn from a world of four workgroups at the pose the pair before it
    found. (With the strides of test_gpu_sequence.py's sets the cap would bind inside workgroup 0 in every pair.)"""
    args, cap, stride, form = CHAIN[name]
    op = ic.optparam(*args, cap)
    cam = ic.CamClass(args[0] + 1, pan["cam"]["fc"], pan["cam"]["cc"], pan["cam"]["wh"], args[2])
    X, p0 = pan["pts3d"], pan["poses"][0]
    st = sq.SequenceTracker(cam, op, X, stride)
    dev = _run(st, pan["frames"], p0)
    assert (st.last_team > 1) == (form == "team")
    host = sq.track_sequence_host_loop(cam, op, X, pan["frames"], p0, stride, return_selection=True)
    margins = [bound_margin(X, p, pan["cam"]) for p in list(dev["poses"]) + list(host["poses"]) + list(pan["poses"])]
    print(name, "npts", host["npts"].tolist(), "iters", host["iters"].tolist(), "min margin %.3e" % min(margins))
    assert min(margins) > 1e-3
    assert any(len(set((s // sc.C).tolist())) >= 2 for s in host["selection"])
    assert all({0, 1, 2} <= set((s // sc.C).tolist()) for s in host["selection"])
    assert len(set(host["npts"].tolist())) > 1 and (host["npts"] < cap).all() and (host["npts"] > 0).all()
    np.testing.assert_array_equal(dev["npts"], host["npts"])
    want_hash = np.array([sq.selection_hash(s) for s in host["selection"]], np.uint64)
    np.testing.assert_array_equal(dev["hash"], want_hash)
    np.testing.assert_array_equal(dev["iters"], host["iters"])
    assert np.abs(dev["poses"] - host["poses"]).max() <= 1e-5
    np.testing.assert_array_equal(dev["poses"][0], host["poses"][0])
    # the last pair's selection state, read back behind four earlier pairs
    last = host["selection"][-1]
    np.testing.assert_array_equal(dev["sel"], last.astype(np.int32))
    ms, varval = sc.finish_sums(X, last)
    assert dev["ms"].tobytes() == ms.tobytes() and np.float64(dev["varval"]).tobytes() == np.float64(varval).tobytes()
