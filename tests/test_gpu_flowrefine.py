"""Variational refinement on the device (csrc/ictr_flowrefine.hip) against its definition patchflow.refine_flow_host.

The stage planes and the full runs are held to flowrefine_cases.MARGIN x the recorded differences of the f32 restatement
(flowrefine_cases.STAGE_DIFF / FULL_DIFF, measured by test_flowrefine_cpu.py), the warp to its derived bound; the exact
cases are demanded bit for bit. Every figure is printed before it is asserted.

Beyond the tolerances the device has the restatement's bits (flowrefine_f32.py): all twelve stage planes, one half-sweep
per colour and the full runs over the table and over flowrefine_cases.EDGE, the weights of flowrefine_cases.PARAMS, a
field far outside the frame, and a NaN in a field that lives in device memory."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import flowrefine_cases as FC
import flowrefine_f32 as R
import invcompcamtrack_amd as ic
from invcompcamtrack_amd import _lib
from invcompcamtrack_amd import patchflow as pf
from invcompcamtrack_amd import stereotrack as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PSZ = 8  # the pyramids' padding; the refinement reads level 0 only

_pyrs = {}


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):  # the "dense" inputs are tracked by the host oracle
    return oracle


def pyramids(frame, pad=PSZ):
    if (frame, pad) not in _pyrs:
        a, b = FC.pair(frame)
        _pyrs[frame, pad] = (ic.Pyramid(a, 0, pad, True), ic.Pyramid(b, 0, pad, False))
    return _pyrs[frame, pad]


def refiner(frame, **params):
    w, h = FC.frame_size(frame)
    return pf.FlowRefiner(w, h, **params)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(frame, kind, run, x_only=False, weights=None, src=None, **kw):
    """A refiner that has run (n_outer, n_sor, omega) = `run` on the entry's F0 (or on `src`); an EDGE frame's pyramids
    are padded by flowrefine_cases.pad_extra more than PSZ."""
    r = refiner(frame, n_outer=run[0], n_sor=run[1], omega=run[2], **FC.weight_args(weights))
    r.run(*pyramids(frame, PSZ + FC.pad_extra(frame)), FC.f0(frame, kind) if src is None else src, x_only=x_only, **kw)
    return r


ALL = FC.TABLE + FC.EDGE


def _assert_bits(got, want, what):
    """got has want's bits; otherwise the count and the first pixel that differs are printed."""
    bad = _bits(got) != _bits(want)
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        print(f"{what}: {int(bad.sum())} of {bad.size} differ, first at {at}: {got[at]!r} for {want[at]!r}")
    assert not bad.any(), what


def _assert_stage_bits(r, want, what):
    """All twelve stage planes of the refiner's last outer iteration have the bits of the restatement's trace entry."""
    for k in R.STAGES:
        _assert_bits(r.stage(k), want[k], f"{what} {k}")


# ---------------------------------------------------------------- stages
@pytest.mark.parametrize("frame,kind", FC.TABLE)
def test_warp_within_the_derived_bound(frame, kind):
    """|Bw - definition| <= 8 u max|B|, derived in flowrefine_cases.warp_error."""
    r = _run(frame, kind, FC.STAGE_RUN)
    err, bound = FC.warp_error(frame, kind, r.stage("bw"))
    print(f"warp {frame} {kind}: {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    f = FC.f0(frame, kind)
    assert np.array_equal(_bits(r.stage("u")), _bits(f[..., 0])) and np.array_equal(_bits(r.stage("v")), _bits(f[..., 1]))


@pytest.mark.parametrize("frame,kind", FC.TABLE)
@pytest.mark.parametrize("x_only", (False, True))
def test_coefficients_and_increment_after_one_outer_iteration(frame, kind, x_only):
    r = _run(frame, kind, FC.STAGE_RUN, x_only)
    planes = {k: r.stage(k) for k in FC.STAGE_DIFF if k != "sweep"}
    errs = FC.stage_errors(frame, kind, x_only, planes)
    print(frame, kind, x_only, {k: float(f"{v:.3g}") for k, v in errs.items()})
    for k, e in errs.items():
        assert e <= FC.MARGIN * FC.STAGE_DIFF[k], (k, e, FC.STAGE_DIFF[k])
    if x_only:
        assert not planes["dv"].any()


@pytest.mark.parametrize("frame,kind", ALL)
@pytest.mark.parametrize("x_only", (False, True))
def test_stage_planes_have_the_restatements_bits(frame, kind, x_only):
    """Bw, the five coefficients, both edge weights, du, dv, u and v after STAGE_RUN, and those of the last of three outer
    iterations (k_fr_warp's fold of the previous increment), bit for bit; and the refined field of both runs."""
    for run in (FC.STAGE_RUN, FC.RUNS[1]):
        r = _run(frame, kind, run, x_only)
        out, tr = FC.restated(frame, kind, *run, x_only)
        assert len(tr) == run[0]
        _assert_stage_bits(r, tr[-1], f"{frame} {kind} {run} x_only={x_only}")
        _assert_bits(r.dense(), out, f"{frame} {kind} {run} x_only={x_only} field")


@pytest.mark.parametrize("frame,kind", ALL)
def test_one_half_sweep_from_injected_coefficients(frame, kind):
    p = FC.sweep_inputs(frame, kind)
    h, w = p["u"].shape
    yy, xx = np.mgrid[0:h, 0:w]
    r = refiner(frame)
    rec = FC.MARGIN * FC.STAGE_DIFF["sweep"] if (frame, kind) in FC.TABLE else FC.EDGE_STAGE_DIFF["sweep"]
    for x_only in (False, True):
        for colour in (0, 1):
            for k, v in p.items():
                r._write_stage(k, v)
            r._half_sweep(colour, x_only)
            du, dv = r.stage("du"), r.stage("dv")
            e = FC.sweep_error(frame, kind, colour, x_only, du, dv)
            print(f"sweep {frame} {kind} colour {colour} x_only {x_only}: {e:.3e}")
            assert e <= rec
            q = {k: v.copy() for k, v in p.items()}
            R.half_sweep(colour, 1.6, x_only, q["u"], q["v"], q["du"], q["dv"], *[q[k] for k in FC.COEF_PLANES])
            _assert_bits(du, q["du"], f"sweep {frame} colour {colour} x_only={x_only} du")
            _assert_bits(dv, q["dv"], f"sweep {frame} colour {colour} x_only={x_only} dv")
            for k in FC.COEF_PLANES + ("u", "v"):  # read back through fr_ci: a half-sweep writes none of them
                _assert_bits(r.stage(k), p[k], f"sweep {frame} {k}")
            other = ((xx + yy) & 1) != colour
            assert np.array_equal(_bits(du)[other], _bits(p["du"])[other])  # the other colour is not written
            assert np.array_equal(_bits(dv)[other], _bits(p["dv"])[other])
            if x_only:
                assert np.array_equal(_bits(dv), _bits(p["dv"]))


# ---------------------------------------------------------------- full runs
@pytest.mark.parametrize("run", FC.RUNS)
@pytest.mark.parametrize("x_only", (False, True))
def test_full_runs(run, x_only):
    """The table at every run, EDGE at EDGE_RUNS: within the record of the definition (EDGE's carries no margin), and the
    restatement's bits."""
    for frame, kind in FC.TABLE + (FC.EDGE if run in FC.EDGE_RUNS else ()):
        edge = (frame, kind) in FC.EDGE
        rec = FC.EDGE_FULL_DIFF[run + (x_only,)] if edge else FC.FULL_DIFF[run + (x_only,)]
        got = _run(frame, kind, run, x_only).dense()
        e = FC.full_error(frame, kind, *run, x_only, got)
        same = np.array_equal(_bits(got), _bits(FC.restated(frame, kind, *run, x_only)[0]))
        print(f"full {run} x_only={x_only} {frame} {kind}: {e:.3e} (record {rec:.3e}); the restatement's bits: {same}")
        assert e <= (1.0 if edge else FC.MARGIN) * rec, (frame, kind)
        _assert_bits(got, FC.restated(frame, kind, *run, x_only)[0], f"full {run} x_only={x_only} {frame} {kind}")
        if x_only:
            assert np.array_equal(_bits(got[..., 1]), _bits(FC.f0(frame, kind)[..., 1]))


# ---------------------------------------------------------------- exact cases
@pytest.mark.parametrize("frame", FC.FRAMES + tuple(f for f, _ in FC.EDGE))
def test_identity_returns_zeros(frame):
    a, _ = FC.pair(frame)
    pa = ic.Pyramid(a, 0, PSZ, False)
    w, h = FC.frame_size(frame)
    for x_only in (False, True):
        out = refiner(frame).run(pa, pa, np.zeros((h, w, 2), np.float32), x_only=x_only).dense()
        assert not out.any()


def test_n_outer_0_and_x_only_keep_bits():
    frame, kind = "67x53", "smooth"
    f = FC.f0(frame, kind).copy()
    f[3, 4, 1], f[5, 6, 1], f[7, 8, 1] = -0.0, np.float32(1e-42), np.float32(-3.25)
    pa, pb = pyramids(frame)
    assert np.array_equal(_bits(refiner(frame, n_outer=0).run(pa, pb, f).dense()), _bits(f))
    out = refiner(frame).run(pa, pb, f, x_only=True).dense()
    assert np.array_equal(_bits(out[..., 1]), _bits(f[..., 1]))
    assert not np.array_equal(out[..., 0], f[..., 0])
    g = pf.FlowGrid(67, 53, 4)
    rng = np.random.default_rng(5)
    g.set_nodes(rng.normal(0, 1, (g.ny, g.nx, 2)).astype(np.float32), np.zeros((g.ny, g.nx), bool))
    assert np.array_equal(_bits(refiner(frame, n_outer=0).run(pa, pb, g).dense()), _bits(g.dense()))


@pytest.mark.parametrize("x_only", (False, True))
def test_a_timed_run_has_four_stage_times_and_the_untimed_runs_bits(x_only):
    """A refiner's own run with timing on, at 37 x 23 (odd width: the two colours' rows differ in length; 23 rows: the
    second row of tiles is partial) with one outer iteration of one sweep: every entry of kernel_ms (warp, coefficients,
    half-sweeps, init + final) is above 0, and the field has the bits of the untimed run and of the f32 restatement."""
    w, h, run = 37, 23, dict(n_outer=1, n_sor=1, omega=1.6)
    a = FC._noisy(FC.texture(w, h, 1237), 2237)
    b = FC._noisy(FC.texture(w, h, 1237, lambda X, Y: (X - 0.6, Y + 0.4)), 3237)
    f = FC.smooth_field(w, h, 5237, (0.6, -0.4), amp=0.3)
    pa, pb = ic.Pyramid(a, 0, PSZ, True), ic.Pyramid(b, 0, PSZ, False)
    r = pf.FlowRefiner(w, h, **run)
    plain = r.run(pa, pb, f, x_only=x_only).dense()
    assert not r.kernel_ms().any()
    r.set_timing(True)
    timed = r.run(pa, pb, f, x_only=x_only).dense()
    ms = r.kernel_ms()
    print(f"timed 37x23 x_only={x_only}: kernel_ms {ms.tolist()}")
    assert ms.shape == (4,) and (ms > 0).all()
    assert timed.tobytes() == plain.tobytes()
    _assert_bits(timed, R.refine(a, b, f, x_only=x_only, **run), f"timed 37x23 x_only={x_only}")
    r.set_timing(False)
    assert r.run(pa, pb, f, x_only=x_only).dense().tobytes() == plain.tobytes() and not r.kernel_ms().any()


def _hip_runtime():
    """The HIP runtime that libictr_hip.so runs on (already in the process), for a stream of the test's own."""
    import ctypes as C
    _lib.load()
    for name in (None, "libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            hip = C.CDLL(name)
            hip.hipStreamCreate, hip.hipStreamDestroy
            return hip
        except (OSError, AttributeError):
            continue
    raise RuntimeError("no HIP runtime to create a stream with")


class _DeviceField:
    """An (H, W, 2) float32 field in device memory, as FlowRefiner.run reads a tensor: the result buffer of a refiner
    that ran with n_outer = 0 holds its input's bits."""

    def __init__(self, frame, f):
        self._r = refiner(frame, n_outer=0).run(*pyramids(frame), f)
        self._r.dense()  # waited for
        self.shape, self.dtype = f.shape, "float32"

    def data_ptr(self):
        return self._r.device_ptr()

    def is_contiguous(self):
        return True


def test_same_bits_from_every_source_stream_and_padding():
    import ctypes as C
    frame, kind, run = "100x77", "dense", FC.RUNS[1]
    f = FC.f0(frame, kind)
    want = _run(frame, kind, run).dense()
    r = refiner(frame, n_outer=run[0], n_sor=run[1], omega=run[2])
    pa, pb = pyramids(frame)
    for _ in range(2):  # twice from the same object
        assert np.array_equal(_bits(r.run(pa, pb, f).dense()), _bits(want))
    hip, stream = _hip_runtime(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
    try:
        _same_sources(frame, r, f, want, stream.value)
    finally:
        assert hip.hipStreamDestroy(stream) == 0


def _same_sources(frame, r, f, want, stream):
    pa, pb = pyramids(frame)
    t = _DeviceField(frame, f)
    assert np.array_equal(_bits(r.run(pa, pb, t).dense()), _bits(want))
    assert np.array_equal(_bits(r.run(pa, pb, t, stream=stream).dense()), _bits(want))
    assert np.array_equal(_bits(r.run(pa, pb, f, stream=stream).dense()), _bits(want))
    other = _DeviceField(frame, np.zeros_like(f))  # its buffer receives the result on the device
    r.dense(out=other.data_ptr(), on_device=True)
    assert np.array_equal(_bits(other._r.dense()), _bits(want))
    for extra in (1, 5):
        qa, qb = pyramids(frame, PSZ + extra)
        assert np.array_equal(_bits(r.run(qa, qb, f).dense()), _bits(want)), extra
        assert np.array_equal(_bits(r.run(qa, pb, f).dense()), _bits(want)), extra  # two paddings in one run
    # a FlowGrid source is its dense field
    g = pf.FlowGrid(100, 77, 4)
    rng = np.random.default_rng(6)
    g.set_nodes((rng.normal(0, 0.4, (g.ny, g.nx, 2)) + (-0.4, -2.4)).astype(np.float32), np.zeros((g.ny, g.nx), bool))
    from_grid = r.run(pa, pb, g).dense()
    assert np.array_equal(_bits(from_grid), _bits(r.run(pa, pb, g.dense()).dense()))
    assert np.array_equal(_bits(from_grid), _bits(r.run(pa, pb, g, stream=stream).dense()))
    # refine_flow: host arrays in and out
    assert np.array_equal(_bits(pf.refine_flow(pa, pb, f, **r.params)), _bits(want))


@pytest.mark.parametrize("w,h,step", ((4, 4, 1), (65, 5, 3), (67, 53, 4)))
def test_one_dense_from_grid_launch_for_the_grid_and_the_refiner(w, h, step):
    """The dense field of a grid is one kernel with one launcher behind FlowGrid.dense (to host, into device memory) and
    behind a grid source of FlowRefiner.run (null stream, a stream of the test's own): the bits of the NumPy restatement
    from all four. One partial wave; a wave and a lane; a partial last row group; 4 x 4 is the refiner's smallest."""
    import ctypes as C

    import frontend_np as FN
    d, lost = FN.grid_nodes(w, h, step, 0.3, 11)
    assert lost.any() and not lost.all()
    g = pf.FlowGrid(w, h, step).set_nodes(d, lost)
    ys, xs = np.mgrid[0:h, 0:w]
    want = _bits(FN.field_at(FN.fill(d, lost), step, w, h, xs.ravel(), ys.ravel()).reshape(h, w, 2))
    img = np.zeros((h, w), np.float32)
    pa, pb = ic.Pyramid(img, 0, PSZ, False), ic.Pyramid(img, 0, PSZ, False)
    assert np.array_equal(_bits(g.dense()), want)
    sink = pf.FlowRefiner(w, h, n_outer=0).run(pa, pb, np.zeros((h, w, 2), np.float32))
    sink.dense()  # waited for; its result buffer is device memory of the field's size
    g.dense(out=sink.device_ptr(), on_device=True)
    assert np.array_equal(_bits(sink.dense()), want)
    r = pf.FlowRefiner(w, h, n_outer=0)
    assert np.array_equal(_bits(r.run(pa, pb, g).dense()), want)
    hip, stream = _hip_runtime(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
    try:
        r.run(pa, pb, np.zeros((h, w, 2), np.float32))  # the result buffer no longer holds the field
        assert np.array_equal(_bits(r.run(pa, pb, g, stream=stream.value).dense()), want)
    finally:
        assert hip.hipStreamDestroy(stream) == 0


# ---------------------------------------------------------------- other weights, fields that leave the frame
@pytest.mark.parametrize("params", FC.PARAMS)
@pytest.mark.parametrize("x_only", (False, True))
def test_other_weights_have_the_restatements_bits(params, x_only):
    """gamma = 0 (wg = 0), delta = 0 (w0 = 0), both (every coefficient 0), and all far from the defaults: the refined
    field and the last outer iteration's planes after (3, 5, omega). The restatement's distance to the definition at
    these weights is flowrefine_cases.PARAM_DIFF, measured on the CPU."""
    run = (3, 5, params[3])
    for frame, kind in FC.PARAM_CASES:
        r = _run(frame, kind, run, x_only, params[:3])
        out, tr = FC.restated(frame, kind, *run, x_only, params[:3])
        what = f"weights {params} x_only={x_only} {frame}"
        _assert_stage_bits(r, tr[-1], what)
        _assert_bits(r.dense(), out, what + " field")
        e = FC.full_error(frame, kind, *run, x_only, r.dense(), params[:3])
        print(f"{what}: {e:.3e} (record {FC.PARAM_DIFF[params]:.3e})")
        assert e <= FC.PARAM_DIFF[params]
        if params[1] == 0 and params[2] == 0:
            assert not any(r.stage(k).any() for k in ("a11", "a12", "a22", "b1", "b2"))


FAR_CASES = (("67x53", "smooth"), ("edge-18x33", "edge"))


@pytest.mark.parametrize("frame,kind", FAR_CASES)
@pytest.mark.parametrize("x_only", (False, True))
def test_a_field_far_outside_the_frame(frame, kind, x_only):
    """Six rows 400 px and six rows 1e6 px out of the frame, from host memory: finite, and the restatement's bits (the
    position is clamped before an index is formed; the rows are outside, so their data weights are 0)."""
    f = FC.far_field(frame, kind)
    a, b = FC.pair(frame)
    run = FC.RUNS[1]
    r = _run(frame, kind, run, x_only, src=f)
    got = r.dense()
    assert np.isfinite(got).all()
    tr = []
    want = R.refine(a, b, f, n_outer=run[0], n_sor=run[1], omega=run[2], x_only=x_only, trace=tr)
    _assert_stage_bits(r, tr[-1], f"far {frame} x_only={x_only}")
    _assert_bits(got, want, f"far {frame} x_only={x_only} field")


def _poke(hip, ptr, value):
    """One float32 into device memory at ptr."""
    import ctypes as C
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    v = C.c_float(value)
    assert hip.hipMemcpy(C.c_void_p(ptr), C.byref(v), 4, 1) == 0  # hipMemcpyHostToDevice


@pytest.mark.parametrize("frame,kind", FAR_CASES)
@pytest.mark.parametrize("x_only", (False, True))
def test_a_nan_in_a_device_field_stays_where_the_rule_carries_it(frame, kind, x_only):
    """The host path refuses a NaN; a field in device memory is not checked. One NaN in u of the far field, (1, 5, 1.6):
    NaN exactly where the restatement has NaN (payloads are not compared), its bits everywhere else. No index depends on
    the value: k_fr_warp clamps the position with fmaxf / fminf first, every other index is formed from the pixel's
    coordinates."""
    f = FC.far_field(frame, kind)
    w, h = FC.frame_size(frame)
    x, y = FC.NAN_AT
    assert 6 <= y < h - 6 and 0 < x < w - 1
    t = _DeviceField(frame, f)
    _poke(_hip_runtime(), t.data_ptr() + 4 * (2 * (y * w + x)), float("nan"))
    got = _run(frame, kind, FC.STAGE_RUN, x_only, src=t).dense()
    f[y, x, 0] = np.nan
    a, b = FC.pair(frame)
    want = R.refine(a, b, f, n_outer=1, n_sor=5, omega=1.6, x_only=x_only)
    nan = np.isnan(want)
    print(f"nan {frame} x_only={x_only}: {int(nan.sum())} of {nan.size} floats are NaN")
    assert nan[y, x, 0] and not nan.all()
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


# ---------------------------------------------------------------- dependence cone
@pytest.mark.parametrize("frame,at", (("farxy-320x64", (160, 32)), ("farxy-64x320", (32, 160))))
@pytest.mark.parametrize("run", FC.RUNS[:2])
def test_dependence_cone(frame, at, run):
    """3 px added to one pixel of F0, on a tile corner: an outer iteration carries it 2 px through the coefficients and 1 px
    per half-sweep, so nothing farther than n_outer (2 n_sor + 2) in Chebyshev distance may change a bit."""
    f = FC.f0(frame, "smooth")
    g = f.copy()
    g[at[1], at[0], 0] += 3.0
    pa, pb = pyramids(frame)
    r = refiner(frame, n_outer=run[0], n_sor=run[1], omega=run[2])
    base = r.run(pa, pb, f).dense().copy()
    moved = r.run(pa, pb, g).dense()
    h, w = f.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    dist = np.maximum(np.abs(xx - at[0]), np.abs(yy - at[1]))
    radius = run[0] * (2 * run[1] + 2)
    changed = (_bits(base) != _bits(moved)).any(-1)
    print(f"cone {frame} {run}: radius {radius}, farthest changed pixel {dist[changed].max()}, {changed.sum()} changed")
    assert (dist > radius).any()
    assert not changed[dist > radius].any()
    assert changed[dist <= 1].all() and changed.sum() > 9


# ---------------------------------------------------------------- refusals
def test_refusals():
    with pytest.raises(_lib.IctrError):
        pf.FlowRefiner(3, 3)
    with pytest.raises(_lib.IctrError):
        pf.FlowRefiner(3, 40)
    for bad in (dict(omega=2.0), dict(omega=0.0), dict(alpha=-1.0), dict(n_sor=-1), dict(n_outer=-2),
                dict(gamma=float("nan")), dict(delta=float("inf")), dict(alpha=0.0), dict(alpha=-0.0)):
        with pytest.raises(_lib.IctrError):
            pf.FlowRefiner(67, 53, **bad)
    with pytest.raises(_lib.IctrError, match="alpha > 0"):
        pf.FlowRefiner(67, 53, alpha=0.0)
    with pytest.raises(_lib.IctrError, match="alpha > 0"):  # the coarse-to-fine flow's refiners take the same check
        pf.CoarseToFineFlow(67, 53, 1, refine=dict(alpha=0.0))
    pf.FlowRefiner(67, 53, gamma=0.0, delta=0.0)  # these stay legal
    with pytest.raises(TypeError):
        pf.FlowRefiner(67, 53, beta=1.0)
    r = refiner("67x53")
    pa, pb = pyramids("67x53")
    qa, _ = pyramids("100x77")
    f = FC.f0("67x53", "smooth")
    with pytest.raises(_lib.IctrError):
        r.dense()  # no run yet
    with pytest.raises(_lib.IctrError):
        r.run(qa, pb, f)
    with pytest.raises(_lib.IctrError):
        r.run(pa, qa, f)
    with pytest.raises(ValueError):
        r.run(pa, pb, FC.f0("100x77", "smooth"))
    big = pf.FlowGrid(100, 77, 4)
    big.set_nodes(np.zeros((big.ny, big.nx, 2), np.float32), np.zeros((big.ny, big.nx), bool))
    with pytest.raises(_lib.IctrError):
        r.run(pa, pb, big)
    with pytest.raises(_lib.IctrError):
        r.run(pa, pb, pf.FlowGrid(67, 53, 4))  # a grid without a field
    for v in (np.nan, np.inf, -np.inf):
        g = f.copy()
        g[11, 13, 1] = v
        with pytest.raises(_lib.IctrError):
            r.run(pa, pb, g)
    assert np.isfinite(r.run(pa, pb, f).dense()).all()  # and the object still runs


# ---------------------------------------------------------------- usefulness on the device
@pytest.mark.parametrize("kind", sorted(FC.USEFUL))
@pytest.mark.parametrize("seed", FC.SEEDS)
def test_device_usefulness(kind, seed):
    n_outer, _ = FC.USEFUL[kind]
    a, b, f, truth, mask = FC.scene(kind, seed)
    pa, pb = ic.Pyramid(a, 0, PSZ, False), ic.Pyramid(b, 0, PSZ, False)
    out = pf.FlowRefiner(FC.SCENE_W, FC.SCENE_H, n_outer=n_outer).run(pa, pb, f).dense()
    before, after = FC.epe(f, truth, mask), FC.epe(out, truth, mask)
    print(f"{kind} seed {seed}: {before:.4f} -> {after:.4f} px ({after / before:.3f}), bar {FC.useful_bar(kind):.3f}")
    assert after <= FC.useful_bar(kind) * before


# ---------------------------------------------------------------- the stereo track window
def _same(got, want):
    assert got[1].tobytes() == want[1].tobytes()
    assert got[0].tobytes() == want[0].tobytes()


def test_window_with_refinement(tmp_path, capsys):
    from invcompcamtrack_amd import run_stereo_track as RS
    from test_gpu_stereotrack import _stereo_frames
    left, right = _stereo_frames()
    kw = dict(step=4, psz=8, lv_f=2)
    params = dict(n_outer=3, n_sor=5)

    def window(**extra):
        t = S.StereoPointTracker(96, 64, 4, **kw, **extra)
        for a, b in zip(left, right):
            t.push_frames(a, b)
        return t, t.window()

    t, got = window(keep_grids=True, refine=params)
    assert len(t.refiners) == 4 and sorted(t.refiners[1]) == ["l_bwd", "l_fwd", "lr", "r_bwd", "r_fwd", "rl"]
    want = S.stereo_track_window_host(*RS.dense_fields_of(t))
    _same(got, want)
    # a refiner's field is the refinement of its grid's dense field, the stereo ones along x only
    pl, pr = ic.Pyramid(left[1], 2, 8, True), ic.Pyramid(right[1], 2, 8, True)
    ql = ic.Pyramid(left[0], 2, 8, True)
    lr = pf.FlowRefiner(96, 64, **params).run(pl, pr, t.grids[1]["lr"].dense(), x_only=True).dense()
    assert np.array_equal(_bits(lr), _bits(t.refiners[1]["lr"].dense()))
    assert np.array_equal(_bits(lr[..., 1]), _bits(t.grids[1]["lr"].dense()[..., 1]))
    fw = pf.FlowRefiner(96, 64, **params).run(ql, pl, t.grids[1]["l_fwd"].dense()).dense()
    assert np.array_equal(_bits(fw), _bits(t.refiners[1]["l_fwd"].dense()))
    _same(window(refine=params)[1], want)  # two refiner sets reused in turn
    plain_t, plain = window(keep_grids=True)
    none_t, none = window(keep_grids=True, refine=None)
    _same(none, plain)
    _same(plain, S.stereo_track_window_host(*RS.dense_fields_of(plain_t)))
    assert none_t.refiners == [] and none_t._rsets == [None, None]
    # the CLI, on the device and with --host
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        for k, (a, b) in enumerate(zip(left, right)):
            np.save(str(tmp_path / f"l{k}.npy"), a)
            np.save(str(tmp_path / f"r{k}.npy"), b)
            f.write(f"{tmp_path / f'l{k}.npy'} {tmp_path / f'r{k}.npy'}\n")
    for extra in ([], ["--host"]):
        out = str(tmp_path / "o.npz")
        assert RS.main([lst, out, "--bsize", "4", "--psz", "8", "--lv_f", "2", "--refine", "16,13,4.5,3,5,1.6"] + extra) == 0
        with np.load(out) as z:
            _same((z["xy_t"], z["rows"]), want)
    out = str(tmp_path / "d.npz")
    assert RS.main([lst, out, "--bsize", "4", "--psz", "8", "--lv_f", "2", "--refine"]) == 0  # the defaults
    with np.load(out) as z:
        assert len(z["rows"]) > 0 and z["xy_t"].shape[1:] == (4, 4)
    assert "kept" in capsys.readouterr().out
    with capsys.disabled():  # recorded, no bar
        print("survivors of", 96 * 64, "start points: without refinement", len(plain[1]), "with", len(got[1]))


def test_cxx_driver(tmp_path):
    """tests/cxx/flowrefine_driver.cpp (CTR::FlowRefineClass of include/ctr_shim.hpp) prints the Python call's bits."""
    exe = str(tmp_path / "flowrefine_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "flowrefine_driver.cpp"),
                           "-L" + os.path.join(ROOT, "invcompcamtrack_amd"), "-l:libictr_hip.so",
                           "-Wl,-rpath," + os.path.join(ROOT, "invcompcamtrack_amd")], timeout=300)
    frame, kind = "67x53", "smooth"
    a, b = FC.pair(frame)
    f = FC.f0(frame, kind)
    raw, ffile = str(tmp_path / "frames.f32"), str(tmp_path / "flow.f32")
    np.stack([a, b]).astype(np.float32).tofile(raw)
    f.tofile(ffile)
    for x_only in (0, 1):
        r = subprocess.run([exe, raw, ffile, "67", "53", str(PSZ), "16", "13", "4.5", "3", "5", "1.6", str(x_only)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.array([[float.fromhex(t) for t in ln.split()] for ln in r.stdout.splitlines()], np.float32)
        want = _run(frame, kind, FC.RUNS[1], bool(x_only)).dense()
        assert np.array_equal(_bits(got.reshape(53, 67, 2)), _bits(want))
    r = subprocess.run([exe, raw, ffile, "67", "53", str(PSZ), "16", "13", "4.5", "3", "5", "2.0", "0"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1 and "omega" in r.stderr
    r = subprocess.run([exe, raw, ffile, "67", "53", str(PSZ), "0", "13", "4.5", "3", "5", "1.6", "0"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "alpha > 0" in r.stderr and not r.stdout
