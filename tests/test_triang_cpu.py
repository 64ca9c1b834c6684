"""Triangulation without a GPU: the NumPy restatement (tests/triang_np.py) against the reference binary's recorded
outputs (tests/golden/triang_golden.npz) bit for bit, the C-ABI's argument checks, the helpers and the text format."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

import triang_np as TN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "triang_golden.npz"))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from invcompcamtrack_amd import _lib
    return _lib.load()


def _assert_bits(got, want, what):
    ok = TN.same_bits(got, want)
    assert ok.all(), f"{what}: {int((~ok).sum())} of {ok.size} words differ, first at {np.argwhere(~ok)[0]}"


@pytest.mark.parametrize("mode", TN.MODES)
def test_np_equals_the_reference_binary_main_group(golden, mode):
    g = golden
    no, mr, di, fct, md = g["options"]
    want_p, want_c, want_i = g[mode + "_pts"], g[mode + "_cov"], g[mode + "_iters"]
    assert len(want_p) == 512
    # no excluded case: the binary returned finite words for every point of the main group
    assert np.isfinite(want_p).all() and np.isfinite(want_c).all()
    r = TN.triangulate(g["P"], g["offsets"], g["view"], g["x"], g["y"], mode, int(no), mr, di, fct, md,
                       init=g["dlt_pts"], campos=g["campos"], ptdir=g["ptdir"])
    _assert_bits(r["pts"], want_p, "points")
    _assert_bits(r["cov"], want_c, "covariances")
    assert np.array_equal(r["iters"], want_i)
    assert not (r["status"] & 1).any()


@pytest.mark.parametrize("mode", TN.MODES)
def test_np_equals_the_reference_binary_degenerate_group(golden, mode):
    g = golden
    off, opts = g["deg_offsets"], g["deg_options"]
    n = len(off) - 1
    assert 8 <= n <= 16
    if mode != "dlt":  # the group does pin non-finite words and early exits
        assert (~np.isfinite(g[f"deg_{mode}_pts"])).any()
        assert len(set(g[f"deg_{mode}_iters"].tolist())) >= 3 and 0 in g[f"deg_{mode}_iters"]
    for i in range(n):
        s = slice(off[i], off[i + 1])
        o = opts[i]
        r = TN.triangulate(g["P"], [0, off[i + 1] - off[i]], g["deg_view"][s], g["deg_x"][s], g["deg_y"][s], mode,
                           int(o[0]), o[1], o[2], o[3], o[4], init=g["deg_init"][i:i + 1],
                           campos=g["deg_campos"][i:i + 1], ptdir=g["deg_ptdir"][i:i + 1])
        _assert_bits(r["pts"], g[f"deg_{mode}_pts"][i:i + 1], f"track {i} point")
        _assert_bits(r["cov"], g[f"deg_{mode}_cov"][i:i + 1], f"track {i} covariance")
        assert r["iters"][0] == g[f"deg_{mode}_iters"][i], i
        nonfinite = not (np.isfinite(r["pts"]).all() and np.isfinite(r["cov"]).all())
        assert bool(r["status"][0] & 1) == nonfinite


def test_reference_named_entry_points_are_declared_and_exported(lib):
    from invcompcamtrack_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ictr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ictr_[A-Za-z0-9_]+)\s*\(", txt))
    names = sorted(_lib.SIGNATURES_REFERENCE_NAMES)
    assert names == ["ictr_triangulate_DLT", "ictr_triangulate_full3D", "ictr_triangulate_full3D_LM"]
    raw = C.CDLL(_lib.LIB_PATH)
    for n in names + ["ictr_triangulate_depthonly"]:
        assert n in declared and hasattr(raw, n), n
    # both tables together are the header's list
    assert declared == set(_lib.SIGNATURES) | set(names)
    for n in ("ictr_triang_create", "ictr_triang_destroy", "ictr_triang_set_cameras", "ictr_triang_set_tracks",
              "ictr_triang_run", "ictr_triang_wait"):
        assert n in _lib.SIGNATURES
    assert C.sizeof(_lib.TriangParams) == 20
    defs = dict(re.findall(r"#define\s+ICTR_TRIANG_([A-Z]+)\s+(\d+)", txt))
    from invcompcamtrack_amd import triang
    assert {k.lower(): int(v) for k, v in defs.items() if k.lower() in triang.MODES} == triang.MODES
    assert (int(defs["NONFINITE"]), int(defs["BEHIND"])) == (triang.STATUS_NONFINITE, triang.STATUS_BEHIND)


def test_argument_validation_and_no_device(lib):
    import invcompcamtrack_amd as ic
    from invcompcamtrack_amd import triang
    from invcompcamtrack_amd._lib import IctrError
    h = C.c_void_p()
    for args in ((0, 10, 4), (1 << 25, 1 << 26, 4), (10, 19, 4), (10, (1 << 28) + 1, 4), (10, 20, 0), (10, 20, (1 << 20) + 1)):
        assert lib.ictr_triang_create(C.byref(h), *args) == 1, args  # ICTR_ERR_INVALID, with or without a device
    assert lib.ictr_triang_create(None, 10, 20, 4) == 1
    z3, z9 = np.zeros(3, np.float32), np.zeros(9, np.float32)
    a = lambda v: v.ctypes.data_as(FP)  # noqa: E731
    one = np.zeros(12, np.float32)
    assert lib.ictr_triangulate_DLT(a(z3), a(z9), a(one), a(one), 1) == 1  # fewer than 2 views
    assert lib.ictr_triangulate_DLT(None, a(z9), a(one), a(one), 2) == 1
    assert lib.ictr_triangulate_full3D(a(z3), a(z9), a(one), a(one), 0, 10, 1e-5) == 1
    assert lib.ictr_triangulate_full3D_LM(a(z3), a(z9), a(one), a(one), 1, 10, 2.0, 10.0, 1e-5, 1e10) == 1
    assert lib.ictr_triangulate_depthonly(a(z3), a(z9), None, a(z3), a(one), a(one), 2, 10, 1e-5) == 1
    assert lib.ictr_triang_wait(None, None, None, None, None) == 1
    with pytest.raises(ValueError):
        triang.triangulate_tracks(np.zeros((2, 12)), [0, 2], [0, 1], np.zeros((2, 2)), mode="nope")
    with pytest.raises(ValueError):
        triang.func_pt_triangulate_from_P_linear_sq([1, 1], [0, 0], [np.eye(3)] * 2, [np.zeros(3)] * 2,
                                                    [np.zeros(2)] * 2, use_c_interf=False)
    P2 = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1], np.float32), (2, 1))
    if ic.device_count() == 0:
        with pytest.raises(IctrError, match="no usable HIP device"):
            triang.Triangulator(10, 20, 4)
        with pytest.raises(IctrError, match="no usable HIP device"):
            triang.triangulate_tracks(P2, [0, 2], [0, 1], np.zeros((2, 2)))
        with pytest.raises(IctrError, match="no usable HIP device"):
            triang.func_pt_triangulate_from_P_linear_sq([1, 1], [0, 0], [np.eye(3)] * 2,
                                                        [np.zeros(3), np.ones(3)], [np.zeros(2)] * 2)
        pl = np.ascontiguousarray(P2.T)
        assert lib.ictr_triangulate_DLT(a(z3), a(z9), a(np.zeros(4, np.float32)), a(pl), 2) == 2  # ICTR_ERR_NO_DEVICE
    else:
        t = triang.Triangulator(10, 20, 4)
        with pytest.raises(IctrError):  # tracks before cameras
            t.set_tracks([0, 2], [0, 1], np.zeros((2, 2)))


def test_cameras_from_poses_is_k_times_exp(lib, oracle):
    from invcompcamtrack_amd import triang
    rng = np.random.default_rng(3)
    cam = dict(fc=np.array([1000.0, 1200.0]), cc=np.array([660.0, 390.0]))
    poses = rng.normal(0, 1, (40, 6)) * np.array([2, 2, 2, 0.3, 0.3, 0.3])
    P = triang.cameras_from_poses(cam, poses)
    assert P.dtype == np.float32 and P.shape == (40, 12)
    K = np.array([[1000.0, 0, 660.0], [0, 1200.0, 390.0], [0, 0, 1.0]])
    for i, p in enumerate(poses):
        want = K @ np.asarray(oracle.se3_exp(p), np.float64).reshape(3, 4)
        # the same sums with K's zeros skipped: equal in f64 up to the last bit, so the f32 words differ by 1 ulp at most
        assert np.all(np.abs(P[i].astype(np.float64) - want.reshape(-1))
                      <= np.spacing(np.abs(want.reshape(-1)).astype(np.float32)).astype(np.float64)), i
    # the reference's matrix of a camera (R, position tw) is the same projection with the other sign
    G = np.asarray(oracle.se3_exp(poses[0]), np.float64).reshape(3, 4)
    R, tw = G[:, :3], -G[:, :3].T @ G[:, 3]
    Pr = triang.func_get_P_from_KRt(cam["fc"], cam["cc"], R, tw)
    assert Pr.shape == (3, 4) and np.allclose(-Pr, K @ G, rtol=1e-12, atol=1e-9)
    # rays: centre and direction of the first view reproduce a noise-free point
    X = np.array([0.5, -0.2, 9.0])
    h = (K @ G) @ np.append(X, 1.0)
    campos, ptdir = triang.rays_from_first_view(cam, poses[:1], [0, 2], [0, 0], np.tile(h[:2] / h[2], (2, 1)))
    assert campos.dtype == np.float32 and np.allclose(campos[0], tw, atol=1e-5)
    d = (X - tw) / np.linalg.norm(X - tw)
    assert np.allclose(ptdir[0], d, atol=1e-5) and abs(np.linalg.norm(ptdir[0].astype(np.float64)) - 1) < 1e-6


def test_reference_named_helpers_form_the_goldens_inputs(golden):
    """func_get_P_from_KRt and the first-view ray, formed in f64 and narrowed, are the words the golden file's binary was
    given (the matrix with the reference's other sign, which changes no result word)."""
    from invcompcamtrack_amd import triang
    g = golden
    for k in range(len(g["P"])):
        Pk = triang.func_get_P_from_KRt(g["fc"], g["cc"], g["cam_R"][k], g["cam_c"][k]).astype(np.float32)
        assert np.array_equal((-Pk).reshape(-1).view(np.uint32), g["P"][k].view(np.uint32)), k
    off, view = g["offsets"], g["view"]
    for i in range(64):
        o = off[i]
        d = triang._ray(g["fc"], g["cc"], g["cam_R"][view[o]], (g["x"][o], g["y"][o])).astype(np.float32)
        assert np.array_equal(d.view(np.uint32), g["ptdir"][i].view(np.uint32)), i
        assert np.array_equal(g["cam_c"][view[o]].astype(np.float32), g["campos"][i])


def test_tracks_from_oftrack_on_the_committed_tracks():
    from invcompcamtrack_amd import triang
    g = np.load(os.path.join(ROOT, "tests", "golden", "classoftrack_golden.npz"))
    blocks = [None if bool(g[f"tracks_none_{i}"]) else g[f"tracks_{i}"] for i in range(int(g["ntracks"]))]
    obj = types.SimpleNamespace(tracks=blocks)
    off, view, xy, origin = triang.tracks_from_oftrack(obj, first_frame=100)
    n = len(off) - 1
    assert n > 20 and off[0] == 0 and off[-1] == len(view) == len(xy) and xy.dtype == np.float32
    want = 0
    for b, blk in enumerate(blocks):
        if blk is None:
            continue
        for k in range(blk.shape[0]):
            L = 0
            while L < blk.shape[2] and np.isfinite(blk[k, :, L]).all():
                L += 1
            want += L >= 2
    assert n == want
    for i in range(n):
        b, k = origin[i]
        L = off[i + 1] - off[i]
        assert L >= 2
        assert np.array_equal(view[off[i]:off[i + 1]], 100 + b + np.arange(L))
        assert np.array_equal(xy[off[i]:off[i + 1]], blocks[b][k, :, :L].T.astype(np.float32))
        assert L == blocks[b].shape[2] or not np.isfinite(blocks[b][k, :, L]).all()
    off3 = triang.tracks_from_oftrack(obj, min_views=3)[0]
    assert len(off3) <= len(off) and np.all(np.diff(off3) >= 3)


def test_text_format_round_trip(tmp_path, golden):
    from invcompcamtrack_amd import run_triangulate as RT
    g = golden
    k = 40
    m = int(g["offsets"][k])
    xy = np.stack([g["x"][:m], g["y"][:m]], 1)
    f = str(tmp_path / "in.txt")
    RT.write_triang_input(f, g["P"], g["offsets"][:k + 1], g["view"][:m], xy, 7, 1e-5, 2.0, 10.0, 1e10,
                          init=g["dlt_pts"][:k], campos=g["campos"][:k], ptdir=g["ptdir"][:k])
    r = RT.read_triang_input(f)
    assert np.array_equal(r["P"].view(np.uint32), g["P"].view(np.uint32))
    assert np.array_equal(r["offsets"], g["offsets"][:k + 1]) and np.array_equal(r["view"], g["view"][:m])
    assert np.array_equal(r["xy"].view(np.uint32), xy.view(np.uint32))
    for key, want in (("init", g["dlt_pts"][:k]), ("campos", g["campos"][:k]), ("ptdir", g["ptdir"][:k])):
        assert np.array_equal(r[key].view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), key
    assert r["noiter"] == 7 and np.float32(r["minres"]) == np.float32(1e-5) and np.float32(r["maxdamp"]) == np.float32(1e10)
    f2 = str(tmp_path / "in2.txt")
    RT.write_triang_input(f2, r["P"], r["offsets"], r["view"], r["xy"], r["noiter"], r["minres"], r["damp_init"],
                          r["damp_fct"], r["maxdamp"], r["init"], r["campos"], r["ptdir"])
    assert open(f2).read() == open(f).read()
    f3 = str(tmp_path / "noopt.txt")
    RT.write_triang_input(f3, g["P"], g["offsets"][:k + 1], g["view"][:m], xy)
    r3 = RT.read_triang_input(f3)
    assert r3["init"] is None and r3["campos"] is None and r3["noiter"] == 10
    out = str(tmp_path / "out.txt")
    res = dict(pts=np.array([[1.5, np.nan, -np.inf]], np.float32), cov=np.arange(9, dtype=np.float32).reshape(1, 3, 3),
               iters=np.array([3]), status=np.array([1]))
    RT.write_triang_result(out, res)
    assert open(out).read() == "1.5 nan -inf 0 1 2 3 4 5 6 7 8 3 1\n"


def test_cxx_driver_compiles(tmp_path, lib):
    exe = str(tmp_path / "triang_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "triang_driver.cpp"),
                           "-L" + os.path.join(ROOT, "invcompcamtrack_amd"), "-l:libictr_hip.so",
                           "-Wl,-rpath," + os.path.join(ROOT, "invcompcamtrack_amd")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
