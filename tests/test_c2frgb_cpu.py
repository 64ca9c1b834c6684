"""The coarse-to-fine dense flow on colour frames, on the CPU: the f32 restatement of the kernels (c2frgb_f32.py) against the
definition (patchflow.c2f_flow_host on triples of pyramids, f64) over c2frgb_cases.RUNS, with the worst differences measured
against their records; the injected defects; the exact and near-exact properties of the rule on both; the usefulness of
colour on an isoluminant scene, on the definition alone; and the C interface's text. test_gpu_c2frgb.py demands the
restatement's bits of the device, so that every figure here is the device's too."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import c2fflow_cases as CC
import c2frgb_cases as RC
import c2frgb_f32 as R
import flowrefine_cases as FC
from invcompcamtrack_amd import _lib
from invcompcamtrack_amd import patchflow as pf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):  # the host pyramids are the oracle's
    return oracle


def _within_record(measured, record, what):
    """The project's rule for a recorded difference: above the record or below half of it fails."""
    print(f"{what}: measured {measured:.3e}, record {record:.3e}")
    assert measured <= record, (what, measured, record)
    assert measured >= 0.5 * record, (what, measured, record, "the record is stale: more than twice what is measured")


# ---------------------------------------------------------------- restatement against definition
def test_restatement_against_definition_level_by_level():
    """From the definition's own starts, on the nodes whose decisions all keep c2fflow_cases.MARGIN_*: every status is
    equal; the worst |d| and |beta| differences are measured against their records; the nodes left out are counted on the
    definition alone and stay within the cap."""
    worst_d, worst_b, worst_out = {}, 0.0, (0.0, None)
    for case, patnorm in RC.RUNS:
        for level, nodes, out, same, diff, bdiff in RC.level_differences(case, patnorm):
            assert same, (case, patnorm, level, "a status differs on a compared node")
            worst_d[level] = max(worst_d.get(level, 0.0), diff)
            worst_b = max(worst_b, bdiff)
            if nodes >= CC.LEFT_OUT_MIN_NODES:
                assert out <= CC.LEFT_OUT_CAP * nodes, (case, patnorm, level, out, nodes)
                if out / nodes > worst_out[0]:
                    worst_out = (out / nodes, (case, patnorm, level))
    for level, record in RC.D_DIFF.items():
        _within_record(worst_d[level], record, f"|d - definition| at level {level}")
    _within_record(worst_b, RC.BETA_DIFF, "|beta - definition|")
    print("left out at most", worst_out)
    assert abs(worst_out[0] - RC.LEFT_OUT[0]) < 1e-3 and worst_out[1] == RC.LEFT_OUT[1]


def test_final_fields_against_definition_at_eps_0():
    worst = 0.0
    for case, patnorm in RC.RUNS:
        if case[4] == 0.0:
            diff = float(np.abs(RC.restated(case, patnorm)[0].astype(np.float64) - RC.host_run(case, patnorm)[0]).max())
            print(RC.case_id(case), patnorm, f"{diff:.3e}")
            worst = max(worst, diff)
    _within_record(worst, RC.FIELD_DIFF, "|final field - definition|")
    case = RC.TABLE[-1]
    assert RC.refine_of(case)
    worst = max(float(np.abs(RC.restated(case, pn)[0].astype(np.float64) - RC.host_run(case, pn)[0]).max())
                for pn in (False, True))
    _within_record(worst, RC.REFINE_FIELD_DIFF, "|final field - definition| with the refinement")


def test_every_status_occurs_on_the_coloured_status_pair():
    """Counted on the definition and on the restatement, which agree: every status 0..4 occurs in all three forms (counts
    of 0..4 at psz 8 / 15 / 17: 40, 380, 54, 6, 24; 26, 420, 35, 17, 6; 22, 427, 35, 19, 1)."""
    for case, need in ((RC.TABLE[7], 5), (RC.STATUS_FORMS[0], 5), (RC.STATUS_FORMS[1], 5)):
        seen_def, seen_f32 = np.zeros(5, int), np.zeros(5, int)
        for s in RC.host_run(case, False)[1]:
            seen_def += np.bincount(s["status"].ravel(), minlength=5)
        for s in RC.restated(case, False)[1]:
            seen_f32 += np.bincount(s[3].ravel(), minlength=5)
        print(RC.case_id(case), seen_def, seen_f32)
        assert len(RC.host_run(case, False)[1]) == 3 and (seen_def[:need] > 0).all() and (seen_f32[:need] > 0).all()


# ---------------------------------------------------------------- injected defects
@pytest.mark.parametrize("defect", R.DEFECTS)
def test_defect_is_seen_by_bits_and_by_the_definition(defect):
    case, patnorm = RC.DEFECT_CASE, True
    want, got = RC.restated(case, patnorm), RC.restated(case, patnorm, defect)
    assert not np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), "the bits of a run do not see it"
    ref = RC.host_run(case, patnorm)[0]
    clean = float(np.abs(want[0].astype(np.float64) - ref).max())
    bad = float(np.abs(got[0].astype(np.float64) - ref).max())
    print(f"{defect}: |field - definition| {bad:.3e}, clean {clean:.3e}")
    assert bad > 100 * clean
    if defect in R.DEFECTS[:3]:  # the search's: the level comparison sees them too, in d or beta or a status
        clean_l, bad_l = RC.level_differences(case, patnorm), RC.level_differences(case, patnorm, defect)
        assert any(not b[3] or b[4] > 100 * max(c[4], 1e-6) or b[5] > 100 * max(c[5], 1e-5) for c, b in zip(clean_l, bad_l))


# ---------------------------------------------------------------- exact and near-exact properties
def test_three_equal_channels_give_the_grey_rule():
    """Channel 0 three times. The definition: the grey definition's statuses and its field to within f64 rounding
    (measured: exactly equal, 0.0 px). The f32 restatement: equal statuses, and a field that is close but not equal in
    bits, because H and b are summed three times; the gap is measured against c2frgb_cases.EQUAL_F32."""
    import c2fflow_f32 as C2
    import patnorm_f32 as PN
    assert any(RC.refine_of(c) for c in RC.EQUAL_CASES)  # the refinement's rule is among them
    for k, case in enumerate(RC.EQUAL_CASES):
        frame, psz, lv_f, maxiter, eps, step, _, _ = case
        refine = RC.refine_of(case)
        for patnorm in (False, True):
            pa, pb = RC.host_pyramids(frame, RC.pad_of(case), lv_f, offsets=patnorm, equal=True)
            sc, sg = [], []
            col = pf.c2f_flow_host(pa, pb, step, psz, lv_f, maxiter, eps, patnorm=patnorm, _stages=sc, refine=refine)
            grey = pf.c2f_flow_host(pa[0], pb[0], step, psz, lv_f, maxiter, eps, patnorm=patnorm, _stages=sg, refine=refine)
            assert all(np.array_equal(a["status"], b["status"]) for a, b in zip(sc, sg))
            host_gap = float(np.abs(col.astype(np.float64) - grey).max())
            assert host_gap <= RC.EQUAL_HOST, (case, patnorm, host_gap)
            if patnorm:
                for a, b in zip(sc, sg):
                    assert np.abs(a["bias"] - b["bias"][..., None]).max() <= 1e-9
            fc, fg = [], []
            f32_col = R.run(pa, pb, step, psz, lv_f, 0, maxiter, eps, patnorm=patnorm, stages=fc, refine_params=refine)
            f32_grey = (PN if patnorm else C2).run(pa[0], pb[0], step, psz, lv_f, maxiter, eps, refine=refine, stages=fg)
            assert all(np.array_equal(a[3], b[3]) for a, b in zip(fc, fg))
            gap = float(np.abs(f32_col.astype(np.float64) - f32_grey).max())
            assert gap > 0
            _within_record(gap, RC.EQUAL_F32[k, patnorm], f"equal channels {RC.case_id(case)} patnorm {patnorm}: host gap "
                           f"{host_gap:.3e}, |colour - grey| of the f32 restatement")


def test_the_refinement_on_three_equal_planes_is_the_grey_refinement():
    """refine_flow_host alone, three outer iterations at full strength on a field that is not converged: the joint weights
    and the channel means of _fr_coef_rgb on three equal planes against _fr_coef (definition, to within f64 rounding), and
    the same on the f32 restatement of k_fr_coef_rgb (close: every channel sum and its quotient by 3 round)."""
    import flowrefine_f32 as FR
    a, b = RC.colour_pair("67x53")
    f0 = FC.smooth_field(67, 53, 5, mean=(1.0, -0.5))
    params = dict(n_outer=3, n_sor=5)
    a3, b3 = np.stack([a[0]] * 3), np.stack([b[0]] * 3)
    for x_only in (False, True):
        grey = pf.refine_flow_host(a[0], b[0], f0, x_only=x_only, **params)
        col = pf.refine_flow_host(a3, b3, f0, x_only=x_only, **params)
        assert float(np.abs(col.astype(np.float64) - grey).max()) <= RC.EQUAL_HOST
        assert float(np.abs(grey - f0).max()) > 0.01  # the refinement moved the field
        g32, c32 = FR.refine(a[0], b[0], f0, x_only=x_only, **params), R.refine(a3, b3, f0, x_only=x_only, **params)
        gap = float(np.abs(c32.astype(np.float64) - g32).max())
        _within_record(gap, RC.EQUAL_REFINE_F32[x_only], f"the refinement alone, x_only {x_only}: f32 |colour - grey|")
    other = pf.refine_flow_host(a, b, f0, **params)  # the three different channels do not give channel 0's result
    assert float(np.abs(other - pf.refine_flow_host(a[0], b[0], f0, **params)).max()) > 1e-3


def test_maxiter_0_held_nodes_silent_nodes_and_x_only_on_the_definition():
    case = RC.TABLE[7]  # the status pair
    frame, psz, lv_f, maxiter, eps, step, _, _ = case
    pa, pb = RC.pyramids_of(case, True)
    st = []
    pf.c2f_flow_host(pa, pb, step, psz, lv_f, 0, eps, _stages=st)
    assert all(not s["field"].any() and not s["d"].any() for s in st)
    silent_seen = 0
    for s in RC.host_run(case, True)[1]:
        held = s["status"] >= pf.C2F_HELD_COND
        assert held.any() and np.array_equal(s["d"][held].view(np.uint32), s["init"][held].view(np.uint32))
        h, w = s["field"].shape[:2]
        xs, ys = np.meshgrid(np.arange(step // 2, w, step), np.arange(step // 2, h, step))
        fx, fy = xs + s["d"][..., 0].astype(np.float64), ys + s["d"][..., 1].astype(np.float64)
        silent = (s["status"] == pf.C2F_LOST) | ~((fx >= 0) & (fx <= w) & (fy >= 0) & (fy <= h))
        assert s["bias"].shape == s["status"].shape + (3,)
        assert not s["bias"][silent].any() and not np.signbit(s["bias"][silent]).any()
        silent_seen += int(silent.sum())
    assert silent_seen > 0
    for case in (c for c in RC.TABLE if c[6]):
        for patnorm in (False, True):
            out, stages = RC.host_run(case, patnorm)
            assert not out[..., 1].view(np.uint32).any()
            assert all(not s["field"][..., 1].view(np.uint32).any() and not s["d"][..., 1].view(np.uint32).any()
                       for s in stages)


def test_host_refusals_say_why():
    case = RC.TABLE[2]
    pa, pb = RC.pyramids_of(case, False)
    with pytest.raises(ValueError, match="three pyramids"):
        pf.c2f_flow_host(pa[:2], pb[:2], 4, 8, 2)
    with pytest.raises(ValueError, match="one frame is grey"):
        pf.c2f_flow_host(pa, pb[0], 4, 8, 2)
    other = RC.pyramids_of(RC.TABLE[0], False)
    with pytest.raises(ValueError, match="differ in geometry"):
        pf.c2f_flow_host([pa[0], other[0][1], pa[2]], pb, 4, 8, 2)
    a, b = RC.colour_pair("67x53")
    d, lost = np.zeros((13, 17, 2), np.float32), np.zeros((13, 17), bool)
    with pytest.raises(ValueError, match=r"bias \(13, 17, 3\)"):
        pf.densify_flow_host(a, b, d, lost, 4, 8, bias=np.zeros((13, 17)))
    with pytest.raises(ValueError, match="three"):
        pf.densify_flow_host(a[:2], b[:2], d, lost, 4, 8)
    with pytest.raises(ValueError, match="three"):
        pf.refine_flow_host(a[:2], b[:2], np.zeros((53, 67, 2), np.float32))
    for call in (lambda: pf.track_points(pa, pb, np.zeros((1, 2), np.float32)),
                 lambda: pf.track_disparity(pa, pb, np.zeros((1, 2), np.float32))):
        with pytest.raises(ValueError, match="grey"):
            call()


# ---------------------------------------------------------------- usefulness, on the host definition
def test_colour_sees_isoluminant_structure():
    """flowrefine_cases' two layers, placed isoluminantly (channels 128 + a, 128 - a, 128): the grey flow on the channel
    mean has no gradient, every node is held and its error is the motion itself; the colour flow tracks. The bar is the
    project's: the worst seed's colour / grey ratio plus a quarter of its gain. Recorded without a bar: the grey flow on
    the luminance twin (the plane 128 + a), and a mixed scene (isoluminant foreground over a luminance background)."""
    worst = 0.0
    for seed in FC.SEEDS:
        grey, col, twin = RC.useful_errors(seed)
        print(f"isoluminant seed {seed}: grey on the channel mean {grey:.3f} px, colour {col:.3f} px, "
              f"grey on the luminance twin {twin:.3f} px")
        assert grey > 1.0  # about the motion itself
        worst = max(worst, col / grey)
        assert col / grey <= RC.useful_bar(), (seed, col / grey)
    _within_record(worst, RC.USEFUL_ISO, "the worst colour / grey ratio")
    for seed in FC.SEEDS:
        grey, col, _ = RC.useful_errors(seed, "mixed")
        print(f"mixed seed {seed} (no bar): grey on the channel mean {grey:.3f} px, colour {col:.3f} px")


# ---------------------------------------------------------------- reading colour frames
def test_read_image_rgb_reads_npy_and_ppm(tmp_path):
    from invcompcamtrack_amd import io_formats as iof
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (5, 7, 3)).astype(np.uint8)
    np.save(str(tmp_path / "c.npy"), img.astype(np.float32) + 0.25)
    got = iof.read_image_rgb(str(tmp_path / "c.npy"))
    assert got.dtype == np.float32 and np.array_equal(got, img.astype(np.float32) + 0.25)
    with open(str(tmp_path / "c.ppm"), "wb") as f:
        f.write(b"P6\n# a comment\n7 5\n255\n" + img.tobytes())
    got = iof.read_image_rgb(str(tmp_path / "c.ppm"))
    assert got.dtype == np.float32 and got.shape == (5, 7, 3) and np.array_equal(got, img.astype(np.float32))
    np.save(str(tmp_path / "g.npy"), img[..., 0])
    with pytest.raises(ValueError, match=r"\(h, w, 3\)"):
        iof.read_image_rgb(str(tmp_path / "g.npy"))
    with open(str(tmp_path / "g.ppm"), "wb") as f:
        f.write(b"P5\n7 5\n255\n" + img[..., 0].tobytes())
    with pytest.raises(ValueError, match="P6"):
        iof.read_image_rgb(str(tmp_path / "g.ppm"))
    # one space behind maxval, and a raster that begins with bytes that read as whitespace and digits: none is the header's
    raster = b"\n12 " + img.tobytes()[4:]
    with open(str(tmp_path / "s.ppm"), "wb") as f:
        f.write(b"P6 7 5 255 " + raster)
    got = iof.read_image_rgb(str(tmp_path / "s.ppm"))
    assert np.array_equal(got, np.frombuffer(raster, np.uint8).reshape(5, 7, 3).astype(np.float32))
    big = rng.integers(0, 65536, (5, 7, 3)).astype(">u2")  # maxval above 255: two bytes per sample, high byte first
    with open(str(tmp_path / "w.ppm"), "wb") as f:
        f.write(b"P6\n7 5\n65535\n" + big.tobytes())
    assert np.array_equal(iof.read_image_rgb(str(tmp_path / "w.ppm")), big.astype(np.float32))
    for name, data, why in (("t.ppm", b"P6\n7 5\n255\n" + img.tobytes()[:-1], "truncated PPM raster"),
                            ("h.ppm", b"P6\n7 5\n", "truncated PPM header"),
                            ("n.ppm", b"P6\n7 x 255\n", "decimal"), ("e.ppm", b"P6\n7 5\n255", "one whitespace byte")):
        with open(str(tmp_path / name), "wb") as f:
            f.write(data)
        with pytest.raises(ValueError, match=why):
            iof.read_image_rgb(str(tmp_path / name))


def test_tracker_and_cli_refuse_colour_with_the_flow_grids():
    from invcompcamtrack_amd import run_stereo_track as RS
    from invcompcamtrack_amd import stereotrack as S
    with pytest.raises(ValueError, match="colour=True needs flow='c2f'"):
        S.StereoPointTracker(96, 64, 4, flow="grid", colour=True)
    with pytest.raises(SystemExit):
        RS.main(["list.txt", "o.npz", "--colour"])


# ---------------------------------------------------------------- the C interface's text
def test_header_declares_what_the_ctypes_table_holds():
    want = ["ictr_c2fflow_get_channels", "ictr_c2fflow_read_level_bias_rgb", "ictr_c2fflow_run_rgb",
            "ictr_c2fflow_set_channels"]
    i, vp = C.c_int, C.c_void_p
    sigs = {"ictr_c2fflow_set_channels": (i, [vp, i]),
            "ictr_c2fflow_get_channels": (i, [vp, C.POINTER(i)]),
            "ictr_c2fflow_run_rgb": (i, [vp, C.POINTER(vp), C.POINTER(vp), vp]),
            "ictr_c2fflow_read_level_bias_rgb": (i, [vp, i, C.POINTER(C.c_float)])}
    assert sorted(sigs) == want
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ictr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ictr_[a-z0-9_]+)\s*\(", txt))
    assert all(n in declared for n in want)
    assert {n: _lib.SIGNATURES[n] for n in want} == sigs
    import __graft_entry__ as G
    assert any(os.path.normpath(h).endswith(os.path.join("include", "ictr.h")) for h in G.HEADERS)
    G.build()
    raw = C.CDLL(_lib.LIB_PATH)
    assert all(hasattr(raw, n) for n in want)
