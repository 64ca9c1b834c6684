"""The staged form of the 8x8 setup kernel's static groups (k_ref8 with a per-wave LDS tile: each 16-patch group's
bounding box of the reference image is copied into LDS line by line, the taps are LDS reads) against the oracle and
against the direct-tap form it replaces where it is faster.

Frames 168 x 104 with two more levels (84 x 52, 42 x 26; padded rows of 184 / 100 / 58 floats, none a multiple of the
32 floats of a cache line: box rows start and end off line boundaries, and at the coarse levels most windows touch the
border rules). Builder-made pyramids, once image-only (getgrad = 2); per-iteration launches (variant bit 13); the chunk
size forced to 16 / 32 / 64 with ICTR_CPW in a fresh child process (tests/ref8_staged_child.py).

Point sets -- a, b, c as the three ragged problems of one batch, `one` alone:
  a    the dense 8-px grid with +-0.35 px jitter, 21 x 13 = 273 points: groups of 16 wrap grid rows, the last chunk is
       partial;
  b    70 uniformly scattered points: every group's box overflows the tile -> the direct taps inside the staged kernel;
  c    17 points: three that leave the reference view (stale patch, stale coefficient line), one on the last valid
       row (y = 104, the inclusive bound, up to the f32 projection's rounding), 13 scattered;
  one  a single point.
Stale entries: a level's size, focal length and principal point are the finest level's times an exact power of two, so
a point is in or out of the reference view at ALL levels of a tracking alike; what keeps a stale patch is a second
SetPose on the same batch without new points (run_track_nposes.cpp:232-258, as
test_points_out_of_view_and_stale_state_across_frames does). Every problem is therefore tracked twice: from p_a, where
all its points are in view, then from p_a moved by 0.34 along the camera's x axis, which shifts every projection ~4.5 px
to the right: the three points of c and the grid's last column (13 points of a, inside dense groups) fall out of view
and keep the first tracking's level-0 patches and coefficient lines. Everything below is checked after the second one.

For every last level lv_l = 2, 1, 0 (the buffers then hold what that level's setup left, stale entries included):
  * T, Gx, Gy: bit-equal to the oracle's buffers -- staged, direct, and staged on the image-only pyramid;
  * coefficient lines: the oracle keeps none, so, as tests/test_gpu_pyramid_patch.py does, bit-equal to the form that
    reads the gradient planes (bit 27) -- which tests/test_gpu_parity.py holds to the oracle's trajectory;
  * H after the level's tail: against the oracle with float64 sums, relative to its largest entry <= 1e-6 -- the
    expression and the bound of test_updates_match_the_summation_order_free_cpu_path (tests/test_gpu_parity.py);
  * staged against direct (bit 29): H and the final poses bit for bit (H is the tail's fixed-order sum of the setup
    launch's per-workgroup partials, so equal H is equal partials up to that sum).
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
W, H, LV_F, PSZ, MAXITER, DEPTH = 168, 104, 2, 8, 3, 10.0
SETS = ("a", "b", "c", "one")


def _lift(sc, px):
    """Pixels of frame A -> world points on the scene's plane (as synth.make_scene lifts its own)."""
    from invcompcamtrack_amd import synth
    fc, cc = sc["fc"].astype(np.float64), sc["cc"].astype(np.float64)
    Ga = synth.se3_exp(sc["p_a"])
    XA = np.stack([(px[:, 0] - cc[0]) / fc[0] * DEPTH, (px[:, 1] - cc[1]) / fc[1] * DEPTH, np.full(len(px), DEPTH)], 0)
    return np.ascontiguousarray(Ga[:, :3].T @ (XA - Ga[:, 3][:, None]))


def _oracle_pt2d(O, sc, pts, pose):
    """The oracle's f32 projections at level 0 and which of them are in the reference view."""
    op = O.make_op(LV_F, 0, PSZ, MAXITER, 0.0, 0, 0, pts.shape[1])
    tr = O.Tracker(op, sc["fc"], sc["cc"], sc["wh"])
    tr.set3dpoints(pts.copy())
    tr.setpose(pose, O.Pyramid(sc["img_a"], LV_F, PSZ), O.Pyramid(sc["img_b"], LV_F, PSZ))
    n, M = pts.shape[1], op.maxpttrack
    x, y = tr.pt2d(0)[:n], tr.pt2d(0)[M:M + n]
    return x, y, (x >= 0) & (y >= 0) & (x <= np.float32(W)) & (y <= np.float32(H))


@functools.lru_cache(maxsize=None)
def _inputs():
    """The scene, the four point sets and the oracle's answers, once for all chunk sizes."""
    from invcompcamtrack_amd import synth
    from oracle import oracle as O
    O.build()
    sc = synth.make_scene(W, H, grid_step=8, margin=4.0, jitter=0.35, seed=31)
    rng = np.random.default_rng(32)
    sets = {"a": sc["pts3d"]}
    assert sets["a"].shape[1] == 21 * 13
    sets["b"] = _lift(sc, np.stack([rng.uniform(4, W - 4, 70), rng.uniform(4, H - 4, 70)], 1))
    p2 = sc["p_a"].copy()
    p2[0] += 0.34
    # c: three points near the right border, which the second pose pushes out; candidates for the last valid row,
    # classified by the oracle's own f32 projections from the second pose
    leave = _lift(sc, np.stack([rng.uniform(165.0, 167.5, 3), rng.uniform(10, H - 10, 3)], 1))
    cand = _lift(sc, np.stack([rng.uniform(20, 140, 4000), H + rng.uniform(-0.05, 0.05, 4000)], 1))
    _, y2, in2 = _oracle_pt2d(O, sc, cand, p2)
    _, _, in1 = _oracle_pt2d(O, sc, cand, sc["p_a"])
    edge = np.flatnonzero(in1 & in2)
    assert len(edge) > 0
    edge = edge[np.argmax(y2[edge])]
    assert y2[edge] > H - 1e-3   # tap row floor(y) = the last one or the one before
    rest = _lift(sc, np.stack([rng.uniform(4, 150, 13), rng.uniform(4, H - 4, 13)], 1))
    sets["c"] = np.ascontiguousarray(np.concatenate([rest[:, :5], leave, rest[:, 5:], cand[:, [edge]]], 1))
    assert sets["c"].shape[1] == 17
    assert np.all(_oracle_pt2d(O, sc, sets["c"], sc["p_a"])[2])
    assert np.flatnonzero(~_oracle_pt2d(O, sc, sets["c"], p2)[2]).tolist() == [5, 6, 7]
    sets["one"] = np.ascontiguousarray(sets["a"][:, 100:101])
    # the oracle, with float64 sums for H (patches and coefficients do not depend on the sum mode)
    opa, opb = O.Pyramid(sc["img_a"], LV_F, PSZ), O.Pyramid(sc["img_b"], LV_F, PSZ)
    want = {}
    O.lib().orc_set_sum_mode(1)
    try:
        for nm, pts in sets.items():
            n = pts.shape[1]
            for lv_l in (2, 1, 0):
                tr = O.Tracker(O.make_op(LV_F, lv_l, PSZ, MAXITER, 0.0, 0, 0, n), sc["fc"], sc["cc"], sc["wh"])
                tr.set3dpoints(pts.copy())
                tr.setpose(sc["p_a"], opa, opb)
                tr.trackpose()
                tr.setpose(p2, opa, opb)
                tr.trackpose()
                rec = [r for r in tr.trace() if r["level"] == lv_l and r["iter"] == 0]
                want[nm, lv_l] = dict(T=tr.buffer(0, 64 * n), Gx=tr.buffer(1, 64 * n), Gy=tr.buffer(2, 64 * n),
                                      H=rec[-1]["H"].copy(), vis=tr.ind(0)[:n].copy())
                tr.close()
    finally:
        O.lib().orc_set_sum_mode(0)
    # the stale entries are really there
    for lv_l in (2, 1, 0):
        assert int((want["c", lv_l]["vis"] == 0).sum()) == 3 and int((want["a", lv_l]["vis"] == 0).sum()) == 13
        assert int((want["one", lv_l]["vis"] == 0).sum()) == 0
    return sc, sets, want, p2


@pytest.mark.parametrize("cpw", [16, 32, 64])
def test_staged_reference_windows_give_the_oracles_patches_and_the_direct_forms_sums(cpw, tmp_path):
    sc, sets, want, p2 = _inputs()
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, img_a=sc["img_a"], img_b=sc["img_b"], fc=sc["fc"], cc=sc["cc"], wh=sc["wh"], p_a=sc["p_a"], p_2=p2,
             **{"pts_" + nm: p for nm, p in sets.items()})
    env = dict(os.environ, ICTR_CPW=str(cpw))
    r = subprocess.run([sys.executable, os.path.join(HERE, "ref8_staged_child.py"), str(cpw), src, dst], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.load(dst)
    relinf = lambda a, b: float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max())
    for nm in SETS:
        for lv_l in (2, 1, 0):
            o = want[nm, lv_l]
            g = lambda form, q: got[f"{form}/{lv_l}/{nm}/{q}"]
            for form in ("staged", "direct", "image"):
                for q in ("T", "Gx", "Gy"):
                    assert np.array_equal(g(form, q), o[q]), (form, nm, lv_l, q, np.abs(g(form, q) - o[q]).max())
                assert np.array_equal(g(form, "coef"), g("planes", "coef")), (form, nm, lv_l, "coefficient lines")
                e = relinf(g(form, "H").reshape(6, 6), o["H"])
                print(f"cpw {cpw} set {nm} lv_l {lv_l} {form}: H vs the float64-sum oracle {e:.3e}")
                assert e <= 1e-6, (form, nm, lv_l, e)
            for form in ("direct", "image"):
                assert np.array_equal(g("staged", "H"), g(form, "H")), (form, nm, lv_l, "H bits")
                assert np.array_equal(g("staged", "pose"), g(form, "pose")), (form, nm, lv_l, "pose bits")
            assert np.all(np.isfinite(g("staged", "pose")))
    assert np.abs(got["staged/0/a/Gx"]).max() > 0.1
