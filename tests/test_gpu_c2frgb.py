"""The coarse-to-fine dense flow on colour frames on the device (the NCH = 3 forms of k_c2f_level, k_densify and k_fr_warp, and
k_fr_coef_rgb) against its f32 restatement (c2frgb_f32.py), bit for bit and with nothing left out: per table entry and
per level the node displacements, the status bytes, the node bias and the level's field, and the final field, so that every
figure c2frgb_cases.py records for the restatement against the definition (patchflow.c2f_flow_host on triples) is the
device's too. Then the exact properties of the rule on the device and the refusals.

The device pyramids are built from the host pyramids' planes, so that both sides read the same bits."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import c2frgb_cases as RC
import c2frgb_f32 as R
import c2fflow_f32 as C2
import invcompcamtrack_amd as ic
from invcompcamtrack_amd import _lib
from invcompcamtrack_amd import patchflow as pf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_pyrs = {}


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):  # the host pyramids are the oracle's
    return oracle


def pyramids(case, patnorm, equal=False):
    """Device pyramids holding the planes of c2frgb_cases.host_pyramids: ([A_c], [B_c])."""
    key = (case[0], RC.pad_of(case), case[2], patnorm, equal)
    if key not in _pyrs:
        w, h = RC.frame_size(case[0])
        host = RC.host_pyramids(case[0], RC.pad_of(case), case[2], offsets=patnorm, equal=equal)
        _pyrs[key] = tuple([ic.Pyramid(lv_f=case[2], imgpadding=RC.pad_of(case), wh=(w, h),
                                       host_planes=(o.img, o.dx, o.dy)) for o in side] for side in host)
    return _pyrs[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _flow(case, patnorm, **over):
    frame, psz, lv_f, maxiter, eps, step, x_only, _ = case
    w, h = RC.frame_size(frame)
    kw = dict(maxiter=maxiter, eps=eps, patnorm=patnorm, x_only=x_only, lv_l=RC.lv_l_of(case), refine=RC.refine_of(case),
              channels=3)
    kw.update(over)
    return pf.CoarseToFineFlow(w, h, lv_f, step, psz, **kw)


def _same_as_restatement(c, case, patnorm, want=None):
    field, stages = want or RC.restated(case, patnorm)
    for level, f, d, status, bias in stages:
        gf, gd, gs = c.level(level)
        assert np.array_equal(gs, status), (case, patnorm, level, "status")
        assert np.array_equal(_bits(gd), _bits(d)), (case, patnorm, level, "d")
        if patnorm:
            gb = c.level_bias(level)
            assert gb.shape == bias.shape and np.array_equal(_bits(gb), _bits(bias)), (case, patnorm, level, "bias")
        assert np.array_equal(_bits(gf), _bits(f)), (case, patnorm, level, "field")
    assert np.array_equal(_bits(c.dense()), _bits(field)), (case, patnorm, "final field")


# ---------------------------------------------------------------- the table, bit for bit
@pytest.mark.parametrize("case,patnorm", RC.RUNS, ids=lambda v: RC.case_id(v) if isinstance(v, tuple) else f"patnorm{int(v)}")
def test_table_has_the_restatements_bits(case, patnorm):
    c = _flow(case, patnorm).run(*pyramids(case, patnorm))
    _same_as_restatement(c, case, patnorm)


@pytest.mark.parametrize("case", RC.STATUS_FORMS, ids=lambda c: f"psz{c[1]}")
def test_the_status_pair_has_the_restatements_bits_in_the_other_forms(case):
    c = _flow(case, False).run(*pyramids(case, False))
    _same_as_restatement(c, case, False)


def test_same_bits_twice_and_on_a_stream():
    from test_gpu_flowrefine import _hip_runtime
    case, patnorm = RC.TABLE[0], True
    pa, pb = pyramids(case, patnorm)
    c = _flow(case, patnorm).run(pa, pb)
    _same_as_restatement(c, case, patnorm)
    _same_as_restatement(c.run(pa, pb), case, patnorm)  # twice from one object
    hip, stream = _hip_runtime(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
    try:
        _same_as_restatement(c.run(pa, pb, stream=stream.value), case, patnorm)
    finally:
        assert hip.hipStreamDestroy(stream) == 0
    frame, psz, lv_f, maxiter, eps, step, _, _ = case
    got = pf.c2f_flow(pa, pb, step, psz, lv_f, maxiter=maxiter, eps=eps, patnorm=True)  # channels follows from the triples
    assert np.array_equal(_bits(got), _bits(RC.restated(case, patnorm)[0]))


def test_one_channel_of_the_same_frames_has_the_grey_restatements_bits():
    import patnorm_f32 as PN
    case = RC.TABLE[0]
    frame, psz, lv_f, maxiter, eps, step, _, _ = case
    w, h = RC.frame_size(frame)
    for patnorm, mod in ((False, C2), (True, PN)):
        pa, pb = pyramids(case, patnorm)
        ha, hb = RC.pyramids_of(case, patnorm)
        for ch in (0, 2):
            want = mod.run(ha[ch], hb[ch], step, psz, lv_f, maxiter, eps)
            c = pf.CoarseToFineFlow(w, h, lv_f, step, psz, maxiter=maxiter, eps=eps, patnorm=patnorm, channels=1)
            assert np.array_equal(_bits(c.run(pa[ch], pb[ch]).dense()), _bits(want)), (patnorm, ch)
            if patnorm:
                assert c.level_bias(0).ndim == 2


def test_grey_and_colour_objects_in_turn_keep_their_bits():
    """Both channel counts through the shared paths in one process: the densifier's and the refiner's one run function
    take the channel count, the densifier's LDS byte count follows the record's size, and the colour refinement's two more
    Bw planes are the object's. 33 x 17 frames (level 1 is 16 x 8: the refiner's 4 x 4 holds, two workgroup columns'
    worth of tiles, odd sizes), lv_f 1, step 4, psz 8, patnorm on, refinement (1, 5, 1.6). Colour, grey, colour, grey:
    every run has the bits of c2frgb_f32.run and patnorm_f32.run respectively, and each second run those of the first."""
    import patnorm_f32 as PN
    from invcompcamtrack_amd import synth
    from oracle import oracle as O
    w, h, lv_f, step, psz, pad = 33, 17, 1, 4, 8, 9
    refine = dict(n_outer=1, n_sor=5, omega=1.6)
    sc = [synth.make_scene(w, h, n_points=4, seed=9, tex_seed=1234 + k, margin=4.0,
                           dp_gt=np.array([0.1, -0.06, 0.05, 0.02, -0.015, 0.01])) for k in range(3)]
    a = [np.ascontiguousarray(s["img_a"], np.float32) for s in sc]
    b = [np.ascontiguousarray(s["img_b"].astype(np.float64) + off, np.float32) for s, off in zip(sc, RC.OFFSETS)]
    ha, hb = [O.Pyramid(x, lv_f, pad) for x in a], [O.Pyramid(x, lv_f, pad) for x in b]
    pa, pb = ([ic.Pyramid(lv_f=lv_f, imgpadding=pad, wh=(w, h), host_planes=(o.img, o.dx, o.dy)) for o in side]
              for side in (ha, hb))
    want = {}
    for nch in (3, 1):
        st = []
        if nch == 3:
            out = R.run(ha, hb, step, psz, lv_f, 0, patnorm=True, stages=st, refine_params=refine)
        else:
            out = PN.run(ha[0], hb[0], step, psz, lv_f, refine=refine, stages=st)
        want[nch] = (out, st)
    flow = {nch: pf.CoarseToFineFlow(w, h, lv_f, step, psz, patnorm=True, refine=refine, channels=nch) for nch in (3, 1)}
    first = {}
    for nch in (3, 1, 3, 1):
        c = flow[nch].run(pa, pb) if nch == 3 else flow[nch].run(pa[0], pb[0])
        _same_as_restatement(c, ("33x17", nch), True, want[nch])
        got = [c.dense()] + [x for level in range(lv_f, -1, -1) for x in list(c.level(level)) + [c.level_bias(level)]]
        assert got[-1].shape[2:] == ((3,) if nch == 3 else ())
        again = first.setdefault(nch, got)
        assert len(got) == 9 and all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), nch


# ---------------------------------------------------------------- exact and near-exact properties, on the device
def test_three_equal_channels_have_the_grey_statuses_and_a_close_field():
    """Channel 0 three times against the grey run on channel 0, the entry with the refinement among them (k_fr_coef_rgb's
    joint weights and channel means against k_fr_coef): H, b and the coefficients are summed three times, so the bits
    differ; the statuses are equal and the field is within c2frgb_cases.EQUAL_F32, the restatement's own gap."""
    assert any(RC.refine_of(c) for c in RC.EQUAL_CASES)
    for k, case in enumerate(RC.EQUAL_CASES):
        frame, psz, lv_f, maxiter, eps, step, _, _ = case
        w, h = RC.frame_size(frame)
        for patnorm in (False, True):
            pa, pb = pyramids(case, patnorm, equal=True)
            col = _flow(case, patnorm).run(pa, pb)
            grey = pf.CoarseToFineFlow(w, h, lv_f, step, psz, maxiter=maxiter, eps=eps, patnorm=patnorm,
                                       refine=RC.refine_of(case)).run(pa[0], pb[0])
            for level in range(lv_f, -1, -1):
                assert np.array_equal(col.level(level)[2], grey.level(level)[2]), (case, patnorm, level)
            gap = float(np.abs(col.dense().astype(np.float64) - grey.dense()).max())
            print(f"equal channels {RC.case_id(case)} patnorm {patnorm}: max |colour - grey| = {gap:.3e} px")
            assert 0 < gap <= RC.EQUAL_F32[k, patnorm], (case, patnorm, gap)


def test_maxiter_0_gives_zeros_at_every_level():
    for case in (RC.TABLE[0], RC.TABLE[7]):
        c = _flow(case, False, maxiter=0).run(*pyramids(case, False))
        for level in range(case[2], -1, -1):
            field, d, status = c.level(level)
            assert not _bits(field).any() and not _bits(d).any(), (case, level)
            assert np.isin(status, (pf.C2F_TRACKED, pf.C2F_HELD_COND)).all()


def test_held_nodes_keep_their_starts_bits_and_silent_nodes_have_zero_bias():
    case = RC.TABLE[7]  # the status pair
    step, lv_f = case[5], case[2]
    c = _flow(case, True).run(*pyramids(case, True))
    coarse, held_seen, silent_seen = None, 0, 0
    for level in range(lv_f, -1, -1):
        field, d, status = c.level(level)
        bias = c.level_bias(level)
        h, w = field.shape[:2]
        init = C2.init_of(coarse, w, h, step)
        held = status >= pf.C2F_HELD_COND
        assert np.array_equal(_bits(d[held]), _bits(init[held])), level
        xs, ys = np.meshgrid(np.arange(step // 2, w, step), np.arange(step // 2, h, step))
        fx, fy = xs.astype(np.float32) + d[..., 0], ys.astype(np.float32) + d[..., 1]
        lost = status == pf.C2F_LOST
        out = ~((fx >= 0) & (fx <= w) & (fy >= 0) & (fy <= h))  # (a lost node's d is the fill's: its own is not read)
        silent = lost | (out & ~lost)
        assert bias.shape == status.shape + (3,) and not _bits(bias[silent]).any(), level
        held_seen += int(held.sum())
        silent_seen += int(silent.sum())
        coarse = field
    assert held_seen > 0 and silent_seen > 0


def test_x_only_leaves_v_at_plus_zero_at_every_level():
    for case in (c for c in RC.TABLE if c[6]):
        for patnorm in (False, True):
            c = _flow(case, patnorm).run(*pyramids(case, patnorm))
            for level in range(case[2], -1, -1):
                field, d, _ = c.level(level)
                assert not _bits(field[..., 1]).any() and not _bits(d[..., 1]).any(), (case, patnorm, level)
            assert not _bits(c.dense()[..., 1]).any()


# ---------------------------------------------------------------- the C++ facade
def test_cxx_driver(tmp_path):
    """tests/cxx/c2frgb_driver.cpp (CTR::CoarseFlowClass::SetChannels / RunRGB / ReadLevelBiasRGB of include/ctr_shim.hpp)
    prints the Python call's bits."""
    exe = str(tmp_path / "c2frgb_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "c2frgb_driver.cpp"),
                           "-L" + os.path.join(ROOT, "invcompcamtrack_amd"), "-l:libictr_hip.so",
                           "-Wl,-rpath," + os.path.join(ROOT, "invcompcamtrack_amd")], timeout=300)
    frame, lv_f, step = "67x53", 2, 4
    a, b = RC.colour_pair(frame, offsets=True)
    frames = str(tmp_path / "frames.f32")
    np.stack([a, b]).astype(np.float32).tofile(frames)
    for psz, maxiter, eps, patnorm, refine in ((8, 10, 0.01, 1, 0), (17, 3, 0.0, 0, 1)):
        pad = psz + 1
        r = subprocess.run([exe, frames, "67", "53", str(pad), str(lv_f), str(step), str(psz), str(maxiter), repr(eps),
                            str(patnorm), str(refine)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.splitlines()
        got = np.array([[float.fromhex(t) for t in ln.split()] for ln in lines[:67 * 53]], np.float32)
        pa = [ic.Pyramid(np.ascontiguousarray(a[c]), lv_f, pad, True) for c in range(3)]
        pb = [ic.Pyramid(np.ascontiguousarray(b[c]), lv_f, pad, True) for c in range(3)]
        c = pf.CoarseToFineFlow(67, 53, lv_f, step, psz, maxiter=maxiter, eps=eps, patnorm=bool(patnorm), channels=3,
                                refine=dict(n_outer=refine, n_sor=2) if refine else None).run(pa, pb)
        assert np.array_equal(_bits(got.reshape(53, 67, 2)), _bits(c.dense())), (psz, refine)
        rest = lines[67 * 53:]
        for ln, level in zip(rest, range(lv_f, -1, -1)):
            assert [int(t) for t in ln.split()[1:]] == [level] + np.bincount(c.level(level)[2].ravel(), minlength=5).tolist()
        if patnorm:
            beta = np.array([[float.fromhex(t) for t in ln.split()] for ln in rest[lv_f + 1:]], np.float32)
            assert np.array_equal(_bits(beta.reshape(c.level_bias(0).shape)), _bits(c.level_bias(0)))
    r = subprocess.run([exe, frames, "67", "53", "8", "2", "4", "9", "10", "0.01", "0", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1 and "padding" in r.stderr


# ---------------------------------------------------------------- the stereo pipeline and the CLI
def _colour_stereo_frames(w=96, h=64, n=4):
    """test_gpu_stereotrack's rendered stereo sequence, once per channel with a texture of its own: (h, w, 3) frames."""
    from invcompcamtrack_amd import synth
    step = np.array([0.15, -0.06, 0.0, 0.0, 0.0, 0.004])
    base = np.array([0.3, -0.2, 0.5, 0.02, -0.03, 0.01])
    right = np.array([-0.55, 0.0, 0.0, 0.0, 0.0, 0.0])
    poses = [base + k * step for k in range(n)] + [base + k * step + right for k in range(n)]
    ch = [synth.make_sequence(w, h, poses, 0, 10, seed=4, tex_seed=1234 + c)["frames"] for c in range(3)]
    fr = [np.ascontiguousarray(np.stack([ch[c][k] for c in range(3)], -1), np.float32) for k in range(2 * n)]
    return fr[:n], fr[n:]


def _same(got, want):
    assert got[1].tobytes() == want[1].tobytes()
    assert got[0].tobytes() == want[0].tobytes()


def test_window_with_colour_frames(tmp_path, capsys):
    from invcompcamtrack_amd import run_stereo_track as RS
    from invcompcamtrack_amd import stereotrack as S
    left, right = _colour_stereo_frames()
    kw = dict(step=4, psz=8, lv_f=2)

    def window(frames=(left, right), **extra):
        t = S.StereoPointTracker(96, 64, 4, **kw, **extra)
        for a, b in zip(*frames):
            t.push_frames(a, b)
        return t, t.window()

    t, got = window(keep_grids=True, flow="c2f", colour=True)
    assert len(t.flows) == 4 and all(c.channels == 3 for f in t.flows for c in f.values())
    want = S.stereo_track_window_host(*RS.dense_fields_of(t))
    _same(got, want)
    assert len(want[1]) > 100
    # an object's field is the stage's on that pair's three pyramids
    tri = lambda im: [ic.Pyramid(np.ascontiguousarray(im[..., c]), 2, 8, True) for c in range(3)]
    assert np.array_equal(_bits(pf.c2f_flow(tri(left[1]), tri(right[1]), 4, 8, 2)), _bits(t.flows[1]["lr"].dense()))
    assert np.array_equal(_bits(pf.c2f_flow(tri(left[0]), tri(left[1]), 4, 8, 2)), _bits(t.flows[1]["l_fwd"].dense()))
    _same(window(flow="c2f", colour=True)[1], want)  # two sets of pyramids and objects reused in turn
    t1, got1 = window(keep_grids=True, flow="c2f-1d", colour=True, patnorm=True, refine=dict(n_outer=1, n_sor=2))
    _same(got1, S.stereo_track_window_host(*RS.dense_fields_of(t1)))
    assert not _bits(t1.flows[1]["lr"].dense()[..., 1]).any()
    # the refiner takes a colour object as a field source exactly as a grey one
    pl, pr = ic.Pyramid(np.ascontiguousarray(left[1][..., 0]), 2, 8, True), ic.Pyramid(
        np.ascontiguousarray(right[1][..., 0]), 2, 8, True)
    c = t.flows[1]["lr"]
    r = pf.FlowRefiner(96, 64, n_outer=1, n_sor=2)
    assert np.array_equal(_bits(r.run(pl, pr, c).dense()), _bits(r.run(pl, pr, c.dense()).dense().copy()))
    with pytest.raises(ValueError, match="colour=True needs flow='c2f'"):
        S.StereoPointTracker(96, 64, 4, flow="grid", colour=True)
    with pytest.raises(ValueError, match="colour frames"):
        S.StereoPointTracker(96, 64, 4, flow="c2f", colour=True, **kw).push_frames(left[0][..., 0], right[0][..., 0])
    # grey against colour on this sequence, recorded without a bar
    grey = [[np.ascontiguousarray(f.mean(-1), np.float32) for f in side] for side in (left, right)]
    _, gw = window(frames=grey, flow="c2f")
    with capsys.disabled():
        print("survivors of", 96 * 64, "start points: grey (channel mean)", len(gw[1]), "colour", len(got[1]))
    # the CLI reads binary .ppm as it reads .npy: the same 8-bit frames in both containers give the same window
    windows = []
    for ext in ("npy", "ppm"):
        qlst = str(tmp_path / f"list_{ext}.txt")
        with open(qlst, "w") as f:
            for k, pair in enumerate(zip(left, right)):
                names = []
                for side, im in zip("lr", pair):
                    q = np.clip(np.rint(im), 0, 255).astype(np.uint8)
                    names.append(str(tmp_path / f"q{side}{k}.{ext}"))
                    if ext == "npy":
                        np.save(names[-1], q.astype(np.float32))
                    else:
                        with open(names[-1], "wb") as g:
                            g.write(b"P6\n96 64\n255\n" + q.tobytes())
                f.write(" ".join(names) + "\n")
        out = str(tmp_path / f"q_{ext}.npz")
        assert RS.main([qlst, out, "--bsize", "4", "--psz", "8", "--lv_f", "2", "--flow", "c2f", "--colour"]) == 0
        with np.load(out) as zf:
            windows.append((zf["xy_t"], zf["rows"]))
    _same(windows[1], windows[0])
    assert len(windows[0][1]) > 100
    # the CLI on the float frames (.npy), on the device and with --host
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        for k, (a, b) in enumerate(zip(left, right)):
            np.save(str(tmp_path / f"l{k}.npy"), a)
            np.save(str(tmp_path / f"r{k}.npy"), b)
            f.write(f"{tmp_path / f'l{k}.npy'} {tmp_path / f'r{k}.npy'}\n")
    base = [lst, str(tmp_path / "o.npz"), "--bsize", "4", "--psz", "8", "--lv_f", "2"]
    for extra in ([], ["--host"]):
        assert RS.main(base + ["--flow", "c2f", "--colour"] + extra) == 0
        with np.load(base[1]) as zf:
            _same((zf["xy_t"], zf["rows"]), want)
        assert RS.main(base + ["--flow", "c2f-1d", "--colour", "--patnorm", "--refine", "16,13,4.5,1,2"] + extra) == 0
        with np.load(base[1]) as zf:
            _same((zf["xy_t"], zf["rows"]), got1)
    with pytest.raises(SystemExit):
        RS.main(base + ["--colour"])


def test_refusals_say_why():
    case = RC.TABLE[2]
    frame, psz, lv_f, _, _, step, _, _ = case
    w, h = RC.frame_size(frame)
    pa, pb = pyramids(case, False)
    col, grey = pf.CoarseToFineFlow(w, h, lv_f, step, psz, channels=3), pf.CoarseToFineFlow(w, h, lv_f, step, psz)
    L = _lib.load()
    trip = lambda ps: (C.c_void_p * 3)(*[p._h.value for p in ps])
    assert L.ictr_c2fflow_run(col._h, pa[0]._h, pb[0]._h, None) != 0 and b"3 channels" in L.ictr_last_error()
    assert L.ictr_c2fflow_run_rgb(grey._h, trip(pa), trip(pb), None) != 0 and b"1 channel" in L.ictr_last_error()
    with pytest.raises(ValueError, match="three pyramids"):
        col.run(pa[0], pb[0])
    with pytest.raises(ValueError, match="one pyramid"):
        grey.run(pa, pb)
    # a channel of another size, and one of the same size with another padding (in both frames: each pair is sound)
    for other in (RC.TABLE[0], RC.TABLE[4]):
        assert RC.pad_of(other) != RC.pad_of(case) and other[2] == lv_f
        qa, qb = pyramids(other, False)
        with pytest.raises(ic.IctrError, match="differ in geometry"):
            col.run([pa[0], qa[1], pa[2]], [pb[0], qb[1], pb[2]])
    n = C.c_int()
    assert L.ictr_c2fflow_get_channels(col._h, C.byref(n)) == 0 and n.value == 3
    assert L.ictr_c2fflow_set_channels(grey._h, 2) != 0 and b"1: grey, or 3: colour" in L.ictr_last_error()
    with pytest.raises(ValueError, match="channels is 2"):
        pf.CoarseToFineFlow(w, h, lv_f, step, psz, channels=2)
    col.run(pa, pb)
    assert L.ictr_c2fflow_set_channels(col._h, 1) != 0 and b"before the first run" in L.ictr_last_error()
    with pytest.raises(ic.IctrError, match="patnorm off"):
        col.level_bias(0)
    pn = pf.CoarseToFineFlow(w, h, lv_f, step, psz, channels=3, patnorm=True).run(pa, pb)
    bias = np.empty(pn.level_dims(0)[2] * pn.level_dims(0)[3] * 3, np.float32)
    assert L.ictr_c2fflow_read_level_bias(pn._h, 0, bias.ctypes.data_as(_lib.FP)) != 0
    assert b"read_level_bias_rgb" in L.ictr_last_error()
    # the stages that stay grey refuse a colour frame and say so
    g = pf.FlowGrid(w, h, step)
    for call in (lambda: g.compute(pa, pb, psz), lambda: g.compute_x(pa, pb, psz),
                 lambda: pf.track_points(pa, pb, np.zeros((1, 2), np.float32), psz),
                 lambda: pf.track_disparity(pa, pb, np.zeros((1, 2), np.float32), psz),
                 lambda: pf.FlowDensifier(w, h).run(g, pa, pb, psz),
                 lambda: pf.FlowRefiner(w, h).run(pa, pb, np.zeros((h, w, 2), np.float32))):
        with pytest.raises(ValueError, match="grey"):
            call()
    tracker = pf.PointTracker(w, h, bsize=2, lv_f=lv_f, psz=psz)
    with pytest.raises(ValueError, match="grey"):
        tracker.push_frame(np.zeros((h, w, 3), np.float32))
    assert tracker.frcounter == 0  # nothing was pushed
