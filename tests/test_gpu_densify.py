"""Densification of a flow grid on the device (csrc/ictr_densify.hip) against its f32 restatement (densify_f32.py), bit for
bit: the field and both stage planes of every table entry, so that every figure densify_cases.py records for the
restatement against the definition (patchflow.densify_flow_host) is the device's too. Then the exact properties of the
rule, the hand-over to the refinement and to the stereo track window, the C++ facade, the CLI, the refusals and the
usefulness bars."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import densify_cases as DC
import densify_f32 as R
import flowrefine_cases as FC
import invcompcamtrack_amd as ic
from invcompcamtrack_amd import _lib
from invcompcamtrack_amd import patchflow as pf
from invcompcamtrack_amd import stereotrack as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_pyrs = {}


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):  # the "tracked" tables and the usefulness scenes are tracked by the host oracle
    return oracle


def pyramids(frame, pad, lv_f=0):
    """Level 0 is all the densifier reads; lv_f > 0 and gradients are for FlowGrid.compute."""
    if (frame, pad, lv_f) not in _pyrs:
        a, b = FC.pair(frame)
        _pyrs[frame, pad, lv_f] = (ic.Pyramid(a, lv_f, pad, lv_f > 0), ic.Pyramid(b, lv_f, pad, lv_f > 0))
    return _pyrs[frame, pad, lv_f]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _grid(frame, step, d, lost):
    w, h = FC.frame_size(frame)
    return pf.FlowGrid(w, h, step).set_nodes(d, lost)


def _same_as_restatement(z, a, b, grid, psz, power, what):
    """The device's field and stage planes against the restatement on the grid's own nodes."""
    d, lost = grid.nodes()
    st = {}
    want = R.densify(a, b, d, lost, grid.step, psz, DC.MINERR, power, stages=st)
    assert np.array_equal(_bits(z.dense()), _bits(want)), what
    assert np.array_equal(z.stage("count"), st["count"]), what
    assert np.array_equal(_bits(z.stage("wsum")), _bits(st["wsum"])), what


# ---------------------------------------------------------------- the table, bit for bit
@pytest.mark.parametrize("frame", DC.FRAMES)
def test_table_has_the_restatements_bits(frame):
    w, h = FC.frame_size(frame)
    zs = {p: pf.FlowDensifier(w, h, power=p) for p in DC.POWERS}
    n = 0
    for k, case in enumerate(c for c in DC.GPU_TABLE if c[0] == frame):
        _, step, psz, kind, power = case
        d, lost = DC.nodes(frame, step, kind, psz)
        g = _grid(frame, step, d, lost)
        assert np.array_equal(_bits(g.nodes()[0]), _bits(DC.filled(d, lost, w, h, step))), (case, "the fill")
        z = zs[power].run(g, *pyramids(frame, psz + DC.PAD_EXTRA[k % 3]), psz)
        want, st = DC.restated(*case)  # on the host's fill, which is the device's
        assert np.array_equal(_bits(z.dense()), _bits(want)), case
        assert np.array_equal(z.stage("count"), st["count"]), case
        assert np.array_equal(_bits(z.stage("wsum")), _bits(st["wsum"])), case
        n += 1
    assert n >= 2 * len(DC.GEOMS)


@pytest.mark.parametrize("step,psz", DC.GEOMS)
def test_same_bits_twice_on_a_stream_and_with_any_padding(step, psz):
    from test_gpu_flowrefine import _hip_runtime
    frame = "67x53"
    a, b = FC.pair(frame)
    d, lost = DC.nodes(frame, step, "outside")
    g = _grid(frame, step, d, lost)
    z = pf.FlowDensifier(67, 53, power=2)
    want = z.run(g, *pyramids(frame, psz), psz).dense().copy()
    _same_as_restatement(z, a, b, g, psz, 2, (step, psz))
    assert np.array_equal(_bits(z.run(g, *pyramids(frame, psz), psz).dense()), _bits(want))  # twice from one object
    for extra in DC.PAD_EXTRA[1:]:
        qa, qb = pyramids(frame, psz + extra)
        assert np.array_equal(_bits(z.run(g, qa, qb, psz).dense()), _bits(want)), extra
        assert np.array_equal(_bits(z.run(g, qa, pyramids(frame, psz)[1], psz).dense()), _bits(want)), extra
    hip, stream = _hip_runtime(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
    try:
        assert np.array_equal(_bits(z.run(g, *pyramids(frame, psz), psz, stream=stream.value).dense()), _bits(want))
        z.set_timing(True)
        z.run(g, *pyramids(frame, psz), psz, stream=stream.value)
        assert z.kernel_ms() > 0 and np.array_equal(_bits(z.dense()), _bits(want))
        z.set_timing(False)
        assert z.run(g, *pyramids(frame, psz), psz).kernel_ms() == 0
    finally:
        assert hip.hipStreamDestroy(stream) == 0
    assert np.array_equal(_bits(pf.densify_flow(*pyramids(frame, psz), g, psz, power=2)), _bits(want))
    other = pf.FlowDensifier(67, 53)  # its buffer receives the result on the device
    other.run(g, *pyramids(frame, psz), psz).dense()
    z.dense(out=other.device_ptr(), on_device=True)
    assert np.array_equal(_bits(other.dense()), _bits(want))


# ---------------------------------------------------------------- grids that the tracker filled
@pytest.mark.parametrize("psz", (15, 8))
def test_a_computed_grid_and_its_reinjected_nodes(psz):
    frame, step = "100x77", 4
    a, b = FC.pair(frame)
    pa, pb = pyramids(frame, psz, 2)
    g = pf.FlowGrid(100, 77, step).compute(pa, pb, psz=psz)
    z = pf.FlowDensifier(100, 77)
    got = z.run(g, pa, pb, psz).dense().copy()
    _same_as_restatement(z, a, b, g, psz, 1, "computed")
    d, lost = g.nodes()
    assert 0 < lost.sum() < lost.size
    again = z.run(_grid(frame, step, d, lost), pa, pb, psz).dense()
    assert np.array_equal(_bits(again), _bits(got))
    # a compute_x grid: +0.0 in v, in the votes and in the fallback
    gx = pf.FlowGrid(100, 77, step).compute_x(pa, pb, psz=psz)
    assert not _bits(gx.nodes()[0][..., 1]).any()
    out = z.run(gx, pa, pb, psz).dense()
    _same_as_restatement(z, a, b, gx, psz, 1, "compute_x")
    assert not _bits(out[..., 1]).any() and out[..., 0].any()


# ---------------------------------------------------------------- the exact properties of the rule, on the device
FRAME = "67x53"


def _device(d, lost, step, psz, **params):
    z = pf.FlowDensifier(67, 53, **params)
    g = _grid(FRAME, step, d, lost)
    return z.run(g, *pyramids(FRAME, psz), psz), g


@pytest.mark.parametrize("step,psz", DC.GEOMS)
def test_every_node_lost_gives_the_grids_dense_field(step, psz):
    d, _ = DC.nodes(FRAME, step, "lost0")
    z, g = _device(d, np.ones(d.shape[:2], bool), step, psz)
    assert np.array_equal(_bits(z.dense()), _bits(g.dense()))
    assert not z.stage("count").any() and not z.stage("wsum").any()


@pytest.mark.parametrize("step", (8, 4, 2))
@pytest.mark.parametrize("kind", ("lost0", "smooth", "outside"))
def test_a_tiling_gives_each_pixel_its_nodes_bits(step, kind):
    d, lost = DC.nodes(FRAME, step, kind)
    z, g = _device(d, lost, step, step)
    got, cnt = z.dense(), z.stage("count")
    h, w = 53, 67
    ny, nx = lost.shape
    yy, xx = np.mgrid[0:h, 0:w]
    dn = d[np.minimum(yy // step, ny - 1), np.minimum(xx // step, nx - 1)]
    takes = cnt == 1
    assert takes.any() and (cnt <= 1).all() and (kind == "lost0" or (~takes).any())
    assert np.array_equal(_bits(got)[takes], _bits(dn)[takes])
    assert np.array_equal(_bits(got)[~takes], _bits(g.dense())[~takes])
    st = {}
    pf.densify_flow_host(*FC.pair(FRAME), d, lost, step, step, _stages=st)
    assert np.array_equal(cnt, st["count"])  # the definition's votes: no seeded vote is near the inside boundary


def test_stripes_take_the_fallback():
    step, psz = 5, 4
    d, lost = DC.nodes(FRAME, step, "lost0")
    z, g = _device(d, lost, step, psz)
    yy, xx = np.mgrid[0:53, 0:67]
    stripe = (xx % step == step - 1) | (yy % step == step - 1)
    got, up, cnt = z.dense(), g.dense(), z.stage("count")
    assert not cnt[stripe].any() and (cnt[~stripe] == 1).any()
    assert np.array_equal(_bits(got)[stripe], _bits(up)[stripe])
    assert not np.array_equal(_bits(got)[~stripe], _bits(up)[~stripe])


def test_a_constant_table_comes_back():
    """Within 2 ulp of the constant wherever a vote exists, as the rule states it for the f32 form; the mean about the
    first vote returns the constant's bits (test_densify_cpu.test_a_constant_table_comes_back)."""
    a, b = FC.pair(FRAME)
    worst = 0
    for step, psz in DC.CONST_GEOMS:
        _, lost = DC.nodes(FRAME, step, "smooth")
        for c in DC.CONSTANTS:
            dc = np.empty(lost.shape + (2,), np.float32)
            dc[...] = np.float32(c)
            for power in DC.POWERS:
                z, g = _device(dc, lost, step, psz, power=power)
                _same_as_restatement(z, a, b, g, psz, power, (step, psz, c, power))
                voted = z.stage("count") > 0
                assert voted.any()
                ulps = np.abs(_bits(z.dense()).astype(np.int64) - _bits(dc[0, 0]).astype(np.int64))[voted]
                worst = max(worst, int(ulps.max()))
        print(f"constant table, step {step} psz {psz}: worst distance in ulps so far {worst}")
    assert worst == DC.CONST_ULP["restatement"]
    assert worst <= 2


# ---------------------------------------------------------------- the refinement reads a densifier
def test_the_refiner_reads_a_densifier():
    frame, step, psz = "100x77", 4, 15
    d, lost = DC.nodes(frame, step, "tracked", psz)
    pa, pb = pyramids(frame, psz)
    z = pf.FlowDensifier(100, 77).run(_grid(frame, step, d, lost), pa, pb, psz)
    params = dict(n_outer=3, n_sor=5)
    for x_only in (False, True):
        got = pf.FlowRefiner(100, 77, **params).run(pa, pb, z, x_only=x_only).dense()
        assert np.array_equal(_bits(got), _bits(pf.refine_flow(pa, pb, z.dense(), x_only=x_only, **params)))
    with pytest.raises(ValueError):
        pf.FlowRefiner(67, 53).run(*pyramids("67x53", psz), z)


# ---------------------------------------------------------------- the stereo track window
def _same(got, want):
    assert got[1].tobytes() == want[1].tobytes()
    assert got[0].tobytes() == want[0].tobytes()


def test_window_with_densification(tmp_path, capsys):
    from invcompcamtrack_amd import run_stereo_track as RS
    from test_gpu_stereotrack import _stereo_frames
    left, right = _stereo_frames()
    kw = dict(step=4, psz=8, lv_f=2)

    def window(**extra):
        t = S.StereoPointTracker(96, 64, 4, **kw, **extra)
        for a, b in zip(left, right):
            t.push_frames(a, b)
        return t, t.window()

    t, got = window(keep_grids=True, densify={})
    assert len(t.densifiers) == 4 and sorted(t.densifiers[1]) == ["l_bwd", "l_fwd", "lr", "r_bwd", "r_fwd", "rl"]
    assert t.refiners == []
    fields = RS.dense_fields_of(t)
    want = S.stereo_track_window_host(*fields)
    _same(got, want)
    # a densifier's field is the densification of its grid
    pl, pr, ql = ic.Pyramid(left[1], 2, 8, True), ic.Pyramid(right[1], 2, 8, True), ic.Pyramid(left[0], 2, 8, True)
    assert np.array_equal(_bits(pf.densify_flow(pl, pr, t.grids[1]["lr"], 8)), _bits(t.densifiers[1]["lr"].dense()))
    assert np.array_equal(_bits(pf.densify_flow(ql, pl, t.grids[1]["l_fwd"], 8)), _bits(t.densifiers[1]["l_fwd"].dense()))
    assert not np.array_equal(t.densifiers[1]["l_fwd"].dense(), t.grids[1]["l_fwd"].dense())
    _same(window(densify={})[1], want)  # two densifier sets reused in turn
    # densify -> refine: the refiners read the densifiers, the window reads the refiners
    params = dict(n_outer=3)
    tr, both = window(keep_grids=True, densify={}, refine=params)
    _same(both, S.stereo_track_window_host(*RS.dense_fields_of(tr)))
    lr = pf.FlowRefiner(96, 64, **params).run(pl, pr, tr.densifiers[1]["lr"].dense(), x_only=True).dense()
    assert np.array_equal(_bits(lr), _bits(tr.refiners[1]["lr"].dense()))
    assert np.array_equal(_bits(tr.densifiers[1]["lr"].dense()), _bits(t.densifiers[1]["lr"].dense()))
    _same(window(densify={}, refine=params)[1], both)
    # densify=None is today's path: no object, the grids' window
    plain_t, plain = window(keep_grids=True)
    none_t, none = window(keep_grids=True, densify=None)
    _same(none, plain)
    _same(plain, S.stereo_track_window_host(*RS.dense_fields_of(plain_t)))
    assert none_t.densifiers == [] and none_t._dsets == [None, None] and none_t.refiners == []
    # the 1-D stereo grids densify like the others
    t1, got1 = window(keep_grids=True, densify=dict(power=2), disparity="1d")
    _same(got1, S.stereo_track_window_host(*RS.dense_fields_of(t1)))
    assert not _bits(t1.densifiers[2]["lr"].dense()[..., 1]).any()
    # the CLI, on the device and with --host
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        for k, (a, b) in enumerate(zip(left, right)):
            np.save(str(tmp_path / f"l{k}.npy"), a)
            np.save(str(tmp_path / f"r{k}.npy"), b)
            f.write(f"{tmp_path / f'l{k}.npy'} {tmp_path / f'r{k}.npy'}\n")
    base = [lst, str(tmp_path / "o.npz"), "--bsize", "4", "--psz", "8", "--lv_f", "2"]
    for extra in ([], ["--host"]):
        assert RS.main(base + ["--densify"] + extra) == 0  # the defaults
        with np.load(base[1]) as zf:
            _same((zf["xy_t"], zf["rows"]), want)
        assert RS.main(base + ["--densify", "2,1", "--refine", "16,13,4.5,3"] + extra) == 0
        with np.load(base[1]) as zf:
            _same((zf["xy_t"], zf["rows"]), both)
    assert "kept" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        RS.main(base + ["--densify", "2,1,3"])
    with capsys.disabled():  # recorded, no bar
        print("survivors of", 96 * 64, "start points: grids", len(plain[1]), "densified", len(got[1]),
              "densified + refined", len(both[1]))


# ---------------------------------------------------------------- the C++ facade
def test_cxx_driver(tmp_path):
    """tests/cxx/densify_driver.cpp (CTR::FlowDensifyClass of include/ctr_shim.hpp) prints the Python call's bits."""
    exe = str(tmp_path / "densify_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "densify_driver.cpp"),
                           "-L" + os.path.join(ROOT, "invcompcamtrack_amd"), "-l:libictr_hip.so",
                           "-Wl,-rpath," + os.path.join(ROOT, "invcompcamtrack_amd")], timeout=300)
    frame, step, psz = "67x53", 4, 15
    a, b = FC.pair(frame)
    d, lost = DC.nodes(frame, step, "outside")
    files = [str(tmp_path / n) for n in ("frames.f32", "nodes.f32", "lost.u8")]
    np.stack([a, b]).astype(np.float32).tofile(files[0])
    d.tofile(files[1])
    lost.astype(np.uint8).tofile(files[2])
    for power in (1, 4):
        r = subprocess.run([exe] + files + ["67", "53", str(psz + 1), str(step), str(psz), "2.0", str(power)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.array([[float.fromhex(t) for t in ln.split()] for ln in r.stdout.splitlines()], np.float32)
        want = _device(d, lost, step, psz, power=power)[0].dense()
        assert np.array_equal(_bits(got.reshape(53, 67, 2)), _bits(want))
    r = subprocess.run([exe] + files + ["67", "53", str(psz), str(step), str(psz), "2.0", "5"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 1 and "power" in r.stderr


# ---------------------------------------------------------------- refusals
def test_refusals():
    for bad in (dict(power=0), dict(power=5), dict(minerr=0.0), dict(minerr=-1.0), dict(minerr=float("nan")),
                dict(minerr=float("inf"))):
        with pytest.raises(_lib.IctrError):
            pf.FlowDensifier(67, 53, **bad)
    with pytest.raises(ValueError):
        pf.FlowDensifier(67, 53, power=1.5)
    with pytest.raises(TypeError):
        pf.FlowDensifier(67, 53, beta=1.0)
    with pytest.raises(_lib.IctrError):
        pf.FlowDensifier(1, 53)
    z = pf.FlowDensifier(67, 53)
    pa, pb = pyramids("67x53", 15)
    qa, _ = pyramids("100x77", 15)
    d, lost = DC.nodes("67x53", 4, "smooth")
    g = _grid("67x53", 4, d, lost)
    with pytest.raises(_lib.IctrError):
        z.dense()  # no run yet
    with pytest.raises(_lib.IctrError):
        z.stage("count")
    with pytest.raises(_lib.IctrError):
        z.run(pf.FlowGrid(67, 53, 4), pa, pb, 15)  # a grid without a field
    big = pf.FlowGrid(100, 77, 4)
    big.set_nodes(np.zeros((big.ny, big.nx, 2), np.float32), np.zeros((big.ny, big.nx), bool))
    with pytest.raises(_lib.IctrError):
        z.run(big, pa, pb, 15)
    with pytest.raises(_lib.IctrError):
        z.run(g, qa, pb, 15)
    with pytest.raises(_lib.IctrError):
        z.run(g, pa, qa, 15)
    for psz in (0, 33, -1):
        with pytest.raises(_lib.IctrError):
            z.run(g, pa, pb, psz)
    with pytest.raises(TypeError):
        z.run(d, pa, pb, 15)
    with pytest.raises(ValueError):
        S._descriptor(z, False, 100, 77)
    assert np.isfinite(z.run(g, pa, pb, 15).dense()).all()  # and the object still runs


# ---------------------------------------------------------------- usefulness on the device
@pytest.mark.parametrize("kind,power", sorted(DC.USEFUL))
@pytest.mark.parametrize("seed", FC.SEEDS)
def test_device_usefulness(kind, power, seed):
    a, b, d, lost, f, truth, mask = DC.useful_inputs(kind, seed)
    pad = DC.USEFUL_PSZ
    pa, pb = ic.Pyramid(a, 0, pad, False), ic.Pyramid(b, 0, pad, False)
    g = pf.FlowGrid(FC.SCENE_W, FC.SCENE_H, DC.USEFUL_STEP).set_nodes(d, lost)
    assert np.array_equal(_bits(g.dense()), _bits(f))
    out = pf.densify_flow(pa, pb, g, DC.USEFUL_PSZ, power=power)
    before, after = FC.epe(f, truth, mask), FC.epe(out, truth, mask)
    print(f"{kind} power {power} seed {seed}: {before:.4f} -> {after:.4f} px ({after / before:.3f}), "
          f"bar {DC.useful_bar(kind, power):.3f}")
    assert after <= DC.useful_bar(kind, power) * before
