"""k_patchdisp, the 1-D (x only) patch search for a rectified stereo pair, in its three launch forms against the f64
oracle (patchdisp_np.py) over the job table of patchdisp_cases.py, and every layer above it: FlowGrid.compute_x against
dense_disparity, StereoPointTracker(disparity="1d"), the native caller and the CLI. Every job runs once per session; run
with -s to see the worst ratios and the survivor counts (DESIGN.md records them)."""
import os
import subprocess

import numpy as np
import pytest

import patchdisp_cases as DC
import patchdisp_np as DN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_results = {}


@pytest.fixture(scope="module")
def O(oracle):
    return oracle


@pytest.fixture(scope="module")
def res():
    """{job key: (new, status, iters, form)} of every job of the table, and of the far jobs, on the device."""
    if not _results:
        import invcompcamtrack_amd as ic
        from invcompcamtrack_amd import patchflow as pf
        pyr = {}
        for job in list(DC.jobs().values()) + list(DC.far_jobs().values()):
            if (job.frame, job.pad) not in pyr:
                a, b = DC.pair(job.frame)
                pyr[job.frame, job.pad] = (ic.Pyramid(a, DC.LV, job.pad), ic.Pyramid(b, DC.LV, job.pad))
            pa, pb = pyr[job.frame, job.pad]
            new, ok, it = pf.track_disparity(pa, pb, job.pts, psz=job.psz, lv_f=job.lv_f, lv_l=job.lv_l,
                                             maxiter=job.maxiter, eps=DC.EPS)
            _results[job.key] = (new, ok, it, pf.disparity_last_form())
    return _results


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _collect(jobs, fn):
    """Run fn(job) over the jobs, report every failure, return the worst ratio per form."""
    worst, failed = {}, []
    for job in jobs:
        try:
            r = fn(job)
        except AssertionError as e:
            failed.append(str(e)[:600])
            continue
        worst[DC.form(job)] = max(worst.get(DC.form(job), 0.0), r)
    assert not failed, "\n".join(failed)
    return worst


# ---------------------------------------------------------------- refusals
def test_refusals_and_the_empty_launch():
    import invcompcamtrack_amd as ic
    from invcompcamtrack_amd import patchflow as pf
    from invcompcamtrack_amd._lib import IctrError
    a, b = DC.pair("100x77")
    small, _ = DC.pair("67x53")
    pa, pb = ic.Pyramid(a, DC.LV, 15), ic.Pyramid(b, DC.LV, 15)
    pts = DC.interior("100x77")
    bad = {
        "psz 0": lambda: pf.track_disparity(pa, pb, pts, psz=0, lv_f=2),
        "psz 33": lambda: pf.track_disparity(ic.Pyramid(a, DC.LV, 33), ic.Pyramid(b, DC.LV, 33), pts, psz=33, lv_f=2),
        "lv_l > lv_f": lambda: pf.track_disparity(pa, pb, pts, psz=15, lv_f=1, lv_l=2),
        "lv_f beyond the pyramid": lambda: pf.track_disparity(pa, pb, pts, psz=15, lv_f=3),
        "first pyramid without gradients": lambda: pf.track_disparity(ic.Pyramid(a, DC.LV, 15, False), pb, pts, psz=15,
                                                                      lv_f=2),
        "pad < psz": lambda: pf.track_disparity(pa, pb, pts, psz=16, lv_f=2),
        "pyramids of different size": lambda: pf.track_disparity(pa, ic.Pyramid(small, DC.LV, 15), pts, psz=15, lv_f=2),
        "maxiter < 0": lambda: pf.track_disparity(pa, pb, pts, psz=15, lv_f=2, maxiter=-1),
    }
    for name, call in bad.items():
        with pytest.raises(IctrError):
            call()
            pytest.fail(f"{name} was accepted")
    new, ok, it = pf.track_disparity(pa, pb, np.zeros((0, 2), np.float32), psz=15, lv_f=2)
    assert new.shape == (0, 2) and ok.shape == (0,) and it.shape == (0,)
    assert new.dtype == np.float32 and ok.dtype == bool and it.dtype == np.int32
    from invcompcamtrack_amd import stereotrack as S
    with pytest.raises(ValueError):
        S.StereoPointTracker(96, 64, 4, disparity="3d")


# ---------------------------------------------------------------- the job table
def test_every_launch_took_its_form_and_all_three_ran(res):
    for key, job in DC.jobs().items():
        assert res[key][3] == DC.form(job), (key, res[key][3], DC.form(job))
    assert {r[3] for r in res.values()} == {11, 41, 82}
    assert {j.psz for j in DC.jobs().values()} == {1, 8, 9, 15, 16, 17, 31, 32}


def test_one_step_within_the_derived_bound(O, res):
    """lv_f = lv_l = l, maxiter = 1: (new_x - x) / 2^l against bx / hxx in f64, per point, within one_step's bound for
    the form's lane load (plus the half ulp of the f32 position that comes back)."""
    worst = _collect([j for j in DC.jobs().values() if j.kind == "step"], lambda j: DC.compare_step(j, *res[j.key][:3], O))
    print(f"\ndevice one-step error / bound, worst per form: {worst}")
    assert len(worst) == 3


def test_full_runs_equal_decisions_and_close_positions(O, res):
    """maxiter = 8, eps = 0.005, every level range, K = 1..9, the leaving points, NaN and out-of-view points: status and
    iters equal the oracle's, x within patchdisp_cases.full_tolerance, y with the input's bits, lost points NaN."""
    jobs = [j for j in DC.jobs().values() if j.kind in ("full", "pad")]
    assert {len(j.pts) for j in jobs} >= set(DC.KS) and {(j.lv_f, j.lv_l) for j in jobs} == set(DC.RANGES)
    worst = _collect(jobs, lambda j: DC.compare_full(j, *res[j.key][:3], O))
    print(f"\ndevice full-run error / (bound sum + u |new_x|), worst per form: {worst} "
          f"(tolerance at {DC.FULL_MARGIN * DC.FULL_FACTOR})")
    assert len(worst) == 3


def test_exact_cases(O, res):
    """rows frame: pts' bits with iters = levels where the 2-D call loses points; columns and textureless frames: lost
    with 0 iterations; maxiter 0 returns its input."""
    import invcompcamtrack_amd as ic
    from invcompcamtrack_amd import patchflow as pf
    seen = {"rows": 0, "lost": 0, "maxiter0": 0}
    for key, job in DC.jobs().items():
        new, ok, it, _ = res[key]
        if job.kind == "rows":
            assert ok.all() and np.array_equal(_bits(new), _bits(job.pts)), key
            assert np.all(it == job.lv_f - job.lv_l + 1), (key, it)
        elif job.kind == "lost":
            assert not ok.any() and np.all(it == 0) and np.isnan(new).all(), key
        elif job.kind == "maxiter0":
            _, ok_o, _, _ = DC.oracle_full(O, job)
            assert np.array_equal(ok, ok_o) and np.all(it == 0), key
            assert np.array_equal(_bits(new[ok]), _bits(job.pts[ok])) and np.isnan(new[~ok]).all(), key
        else:
            continue
        seen[job.kind] += 1
    assert seen["rows"] == 24 and seen["lost"] >= 16 and seen["maxiter0"] == 8
    a, b = DC.pair("rows-100x77")
    for psz in (8, 15):
        _, ok2, _ = pf.track_points(ic.Pyramid(a, DC.LV, psz), ic.Pyramid(b, DC.LV, psz), DC.interior("100x77"), psz=psz,
                                    lv_f=2, maxiter=DC.MAXITER, eps=DC.EPS)
        assert not ok2.all(), psz


def test_padding_beyond_psz_gives_the_same_bits(res):
    for psz in DC.FORM_PSZ:
        ref = res[f"pad0-p{psz}"]
        assert ref[1].all()
        for extra in DC.PAD_EXTRA[1:]:
            got = res[f"pad{extra}-p{psz}"]
            assert got[3] == ref[3] == DC.FORM[psz]
            assert np.array_equal(_bits(got[0]), _bits(ref[0])), (psz, extra, np.abs(got[0] - ref[0]).max())
            assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]), (psz, extra)


def test_a_patch_does_not_depend_on_its_launch(res):
    """The full set, a permutation, every point alone and the set interleaved with lost points (in the two-wave form
    every live patch then shares its workgroup's barriers with a lost one): the same bits per point."""
    for psz in DC.FORM_PSZ:
        new, ok, it, form = res[f"pad0-p{psz}"]
        assert form == DC.FORM[psz] and ok.all()
        perm = DC.perm_of(psz)
        pn, pk, pi, pf_ = res[f"indep-perm-p{psz}"]
        assert pf_ == form and np.array_equal(_bits(pn), _bits(new[perm])) and np.array_equal(pi, it[perm]) and pk.all()
        nn, nk, ni, nf = res[f"indep-nan-p{psz}"]
        assert nf == form and np.array_equal(_bits(nn[0::2]), _bits(new)) and np.array_equal(ni[0::2], it), psz
        assert nk[0::2].all() and not nk[1::2].any() and np.isnan(nn[1::2]).all() and np.all(ni[1::2] == 0), psz
        for k in range(DC.N_INTERIOR):
            on, ok1, oi, of = res[f"indep-one{k}-p{psz}"]
            assert of == form and ok1.all()
            assert np.array_equal(_bits(on[0]), _bits(new[k])) and oi[0] == it[k], (psz, k, on[0], new[k])


# ---------------------------------------------------------------- the far jobs: x of 256 and more
def test_far_one_step_within_the_derived_bound(O, res):
    """The far frame's 'step' jobs in the three forms: integer x of 40, 255, 256, 300, the values one ulp to either
    side, half-pixel and two-decimal points, each level."""
    def one(job):
        new, ok, it, form = res[job.key]
        assert form == DC.form(job) and ok.all(), job.key
        return DC.compare_step(job, new, ok, it, O)

    worst = _collect([j for j in DC.far_jobs().values() if j.kind == "step"], one)
    print(f"\nfar frame: device one-step error / bound, worst per form: {worst}")
    assert len(worst) == 3


def test_far_full_runs_truth_and_continuity(O, res):
    """The far frame's full runs: status and iters equal the oracle's, x within compare_full's tolerance (one spacing of
    f32 at x taken off first), y with the input's bits; every point kept and within TRUTH_BAR of the 1.7 px the frame was
    made with; inside a triple of x one ulp apart the displacements agree to 4 x the tolerance, with equal iters."""
    truth, cont = {}, [0.0]

    def one(job):
        new, ok, it, form = res[job.key]
        assert form == DC.form(job), job.key
        r = DC.compare_full(job, new, ok, it, O)
        truth[job.psz] = max(truth.get(job.psz, 0.0), DC.check_truth(job, new, ok))
        cont[0] = max(cont[0], DC.check_continuity(job, new, ok, it, O))
        return r

    worst = _collect([j for j in DC.far_jobs().values() if j.kind == "full"], one)
    print(f"\nfar frame: device full-run error beyond one spacing / (bound sum + u |new_x|), worst per form: {worst}; "
          f"worst truth error per psz {truth} (bars {DC.TRUTH_BAR}); largest difference inside a triple {cont[0]:.2e} px")
    assert len(worst) == 3


def test_flow_grid_compute_x_on_the_far_pair():
    """FlowGrid.compute_x on the far pair, its dense field read at the node pixels (so after the fill): patchflow_cases.
    check_grid with the 1-D bar."""
    import invcompcamtrack_amd as ic
    from invcompcamtrack_amd import patchflow as pf
    PC = DC.PC
    a, b = DC.pair(DC.FAR_FRAME)
    w, h = PC.frame_size(DC.FAR_FRAME)
    pa, pb = ic.Pyramid(a, PC.GRID_LV, PC.GRID_PSZ), ic.Pyramid(b, PC.GRID_LV, PC.GRID_PSZ)
    g = pf.FlowGrid(w, h, PC.GRID_STEP).compute_x(pa, pb, psz=PC.GRID_PSZ, lv_f=PC.GRID_LV)
    assert pf.disparity_last_form() == 41
    field = g.dense()
    assert not field[..., 1].any()
    got = PC.check_grid(DC.FAR_FRAME, field, g.nodes()[1], DC.TRUTH_BAR[PC.GRID_PSZ])
    print(f"\ndevice grid (x only), largest interior error {got[0]:.4f} px, median below 256 {got[1]:.4f}, from 256 on "
          f"{got[2]:.4f}")


# ---------------------------------------------------------------- usefulness
@pytest.mark.parametrize("tilt", DC.SCENE_TILTS)
def test_usefulness_on_the_device(tilt):
    """The CPU module's scene and bars: the 1-D launch keeps every node with a median |x error| <= 0.05 px where the 2-D
    launch's median is >= 0.3 px."""
    import invcompcamtrack_amd as ic
    from invcompcamtrack_amd import patchflow as pf
    a, b = DC.scene(tilt, 1)
    pa, pb = ic.Pyramid(a, DC.SCENE_LV, DC.SCENE_PSZ), ic.Pyramid(b, DC.SCENE_LV, DC.SCENE_PSZ)
    nodes = DC.scene_nodes()
    new1, ok1, _ = pf.track_disparity(pa, pb, nodes, psz=DC.SCENE_PSZ, lv_f=DC.SCENE_LV)
    new2, ok2, _ = pf.track_points(pa, pb, nodes, psz=DC.SCENE_PSZ, lv_f=DC.SCENE_LV)
    k1, med1, max1 = DC.scene_errors(new1, ok1)
    k2, med2, _ = DC.scene_errors(new2, ok2)
    print(f"\ntilt {tilt}: 1-D kept {k1}, median {med1:.4f} max {max1:.4f} px; 2-D kept {k2}, median {med2:.4f} px")
    assert k1 == 98 and med1 <= DC.BAR_1D
    assert med2 >= DC.BAR_2D
    assert np.array_equal(_bits(new1[:, 1]), _bits(nodes[:, 1]))


# ---------------------------------------------------------------- grid
@pytest.mark.parametrize("frame, psz, lv_f", [("100x77", 15, 2), ("67x53", 8, 2), ("cols-100x77", 15, 0)])
def test_flow_grid_compute_x_equals_dense_disparity(frame, psz, lv_f):
    import invcompcamtrack_amd as ic
    from invcompcamtrack_amd import patchflow as pf
    a, b = DC.pair(frame)
    w, h = DC.PC.frame_size(frame)
    pa, pb = ic.Pyramid(a, DC.LV, psz), ic.Pyramid(b, DC.LV, psz)
    g = pf.FlowGrid(w, h, 4).compute_x(pa, pb, psz=psz, lv_f=lv_f)
    assert pf.disparity_last_form() == DC.FORM[psz]
    want = pf.dense_disparity(pa, pb, step=4, psz=psz, lv_f=lv_f)
    field = g.dense()
    assert np.array_equal(field, want)
    d, lost = g.nodes()
    assert np.array_equal(d, want[2::4, 2::4])                              # the nodes are the field at the node pixels
    assert np.array_equal(_bits(d[..., 1]), np.zeros(d.shape[:2], np.uint32))   # +0.0, sign bit included
    assert np.array_equal(_bits(field[..., 1]), np.zeros((h, w), np.uint32))
    if frame.startswith("cols"):
        # nodes x = 26 .. 70: patch and gradient support inside the equal columns, no x gradient; the fill took over
        assert lost[:, 6:18].all() and 0 < lost.sum() < lost.size
    else:
        assert np.abs(d[..., 0]).max() > 0.5
    # moving points by the field: y + 0.0 has y's bits, so a caller that takes x only gets the same pair
    rng = np.random.default_rng(3)
    xy = np.stack([rng.uniform(0, w - 1.01, 200), rng.uniform(0, h - 1.01, 200)], 1)
    out = g.gather(xy)
    assert np.array_equal(out[:, 1].view(np.uint64), xy[:, 1].view(np.uint64))
    g2 = pf.FlowGrid(w, h, 4).set_nodes(np.stack([d[..., 0], np.full_like(d[..., 0], 0.75)], -1), np.zeros_like(lost))
    out2 = g2.gather(xy)
    assert np.array_equal(out2[:, 0], out[:, 0]) and not np.array_equal(out2[:, 1], out[:, 1])


# ---------------------------------------------------------------- window
def test_stereo_point_tracker_with_the_1d_search():
    """The rendered 64x96 stereo sequence of test_gpu_stereotrack.py: the "1d" object's window equals the host function
    fed its grids' dense fields, its stereo grids are compute_x's; the default object is the 2-D one, unchanged."""
    from invcompcamtrack_amd import patchflow as pf
    from invcompcamtrack_amd import run_stereo_track as R
    from invcompcamtrack_amd import stereotrack as S
    from invcompcamtrack_amd.tracker import Pyramid
    from test_gpu_stereotrack import _same, _stereo_frames
    left, right = _stereo_frames()
    kw = dict(step=4, psz=8, lv_f=2)
    trk = {}
    for mode in ("1d", "2d", None):
        t = trk[mode] = S.StereoPointTracker(96, 64, 4, keep_grids=True, **kw, **({"disparity": mode} if mode else {}))
        for a, b in zip(left, right):
            t.push_frames(a, b)
        got = t.window()
        want = S.stereo_track_window_host(*R.dense_fields_of(t))
        _same(got, want)
        print(f"\nStereoPointTracker(disparity={mode!r}) keeps {len(want[1])} of {96 * 64}")
        t.result = got
    _same(trk[None].result, trk["2d"].result)
    pl, pr = Pyramid(left[0], 2, 8, True), Pyramid(right[0], 2, 8, True)
    for mode, fn in (("1d", "compute_x"), (None, "compute")):
        for name, (p, q) in (("lr", (pl, pr)), ("rl", (pr, pl))):
            d, lost = trk[mode].grids[0][name].nodes()
            d2, lost2 = getattr(pf.FlowGrid(96, 64, 4), fn)(p, q, psz=8, lv_f=2).nodes()
            assert np.array_equal(_bits(d), _bits(d2)) and np.array_equal(lost, lost2), (mode, name)
            assert (not d[..., 1].any()) == (mode == "1d")
    for name in ("l_fwd", "l_bwd", "r_fwd", "r_bwd"):   # the temporal grids stay 2-D
        assert np.array_equal(trk["1d"].grids[1][name].nodes()[0], trk[None].grids[1][name].nodes()[0])


# ---------------------------------------------------------------- native caller and CLI
def test_cxx_driver_and_cli(tmp_path):
    import invcompcamtrack_amd as ic
    from invcompcamtrack_amd import patchflow as pf
    from invcompcamtrack_amd import run_stereo_track as R
    from test_gpu_stereotrack import _stereo_frames
    exe = str(tmp_path / "patchdisp_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "patchdisp_driver.cpp"),
                           "-L" + os.path.join(ROOT, "invcompcamtrack_amd"), "-l:libictr_hip.so",
                           "-Wl,-rpath," + os.path.join(ROOT, "invcompcamtrack_amd")], timeout=300)
    a, b = DC.pair("100x77")
    pts = np.concatenate([DC.interior("100x77"), DC.special("100x77")])
    raw, pfile = str(tmp_path / "frames.f32"), str(tmp_path / "pts.f32")
    np.stack([a, b]).astype(np.float32).tofile(raw)
    pts.tofile(pfile)
    for psz, form in ((8, 11), (15, 41), (31, 82)):
        r = subprocess.run([exe, raw, pfile, "100", "77", str(len(pts)), str(psz), "2", "0", "8", "0.005"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        new, ok, it = pf.track_disparity(ic.Pyramid(a, 2, psz), ic.Pyramid(b, 2, psz, False), pts, psz=psz, lv_f=2,
                                         maxiter=8, eps=0.005)
        lines = r.stdout.splitlines()
        assert lines[-1].split() == ["form", str(form)] and len(lines) == len(pts) + 1
        assert ok.sum() >= DC.N_INTERIOR and not ok.all()
        for k, ln in enumerate(lines[:-1]):
            x, y, s, n = ln.split()
            want = ["nan", "nan"] if not ok[k] else [float(new[k, 0]).hex(), float(new[k, 1]).hex()]
            got = [x, y] if x == "nan" else [float.fromhex(x).hex(), float.fromhex(y).hex()]
            assert got == want and int(s) == int(ok[k]) and int(n) == it[k], (psz, k, ln)
    # the CLI with --disparity 1d, device and --host
    left, right = _stereo_frames()
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        for k, (l, r) in enumerate(zip(left, right)):
            np.save(str(tmp_path / f"l{k}.npy"), l)
            np.save(str(tmp_path / f"r{k}.npy"), r)
            f.write(f"{tmp_path / f'l{k}.npy'} {tmp_path / f'r{k}.npy'}\n")
    outs = {}
    for name, extra in (("1d", ["--disparity", "1d"]), ("1d-host", ["--disparity", "1d", "--host"]), ("2d", [])):
        out = str(tmp_path / f"{name}.npz")
        assert R.main([lst, out, "--bsize", "4", "--psz", "8", "--lv_f", "2"] + extra) == 0
        with np.load(out) as z:
            outs[name] = (z["xy_t"].copy(), z["rows"].copy())
    assert np.array_equal(outs["1d"][0], outs["1d-host"][0], equal_nan=True) and np.array_equal(outs["1d"][1], outs["1d-host"][1])
    assert len(outs["1d"][1]) > 100
    assert not (outs["1d"][0].shape == outs["2d"][0].shape and np.array_equal(outs["1d"][0], outs["2d"][0]))
    with pytest.raises(SystemExit):
        R.main([lst, str(tmp_path / "x.npz"), "--disparity", "3d"])
