"""Destroying an object gives back the device memory it took. Per case: one warm-up cycle (the runtime's own lazy
allocations -- code objects, scratch, the team events -- land there), then CYCLES cycles of create -> use once -> drop;
the device's free memory may have dropped by at most F, a LOWER bound on one cycle's footprint computed from the case's
sizes as the sum of the large buffers named in the object's struct. A leak of any of them shows as about CYCLES x F.

The reading is device-wide, so the cases are sized by footprint (F >= 16 MiB each, to stand out from other tenants'
traffic), not by arithmetic difficulty: the work per cycle stays tiny."""
import gc

import numpy as np
import pytest

import invcompcamtrack_amd as ic
from invcompcamtrack_amd import icgn, patchflow as pf, ransac, sequence as sq, synth

pytestmark = pytest.mark.gpu
MIB = 1 << 20
CYCLES = 10
W = H = 1024


def _free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _check_returns_memory(cycle, F, cycles=CYCLES):
    assert F >= 16 * MIB, f"the case's footprint bound is only {F / MIB:.1f} MiB"
    cycle()  # warm-up
    gc.collect()
    before = _free_bytes()
    for _ in range(cycles):
        cycle()
        gc.collect()
    drop = before - _free_bytes()
    print(f"free memory dropped by {drop / MIB:.2f} MiB over {cycles} cycles; one cycle holds >= {F / MIB:.2f} MiB")
    assert drop <= F, f"{drop / MIB:.2f} MiB not returned after {cycles} cycles (one cycle holds >= {F / MIB:.2f} MiB)"


def _plane7(w, h, pad):
    """Level 0 of a gradient pyramid: img, dx, dy and the packed texels, 7 padded f32 planes."""
    return 7 * 4 * (w + 2 * pad) * (h + 2 * pad)


@pytest.fixture(scope="module")
def frames():
    """Three 1024 x 1024 frames: blocky integer noise (corners everywhere), moved by two pixels per frame."""
    rng = np.random.default_rng(3)
    base = np.kron(rng.integers(0, 256, (H // 8 + 1, W // 8 + 1)), np.ones((8, 8))).astype(np.float32)
    return np.stack([np.ascontiguousarray(base[2 * k:2 * k + H, 2 * k:2 * k + W]) for k in range(3)])


@pytest.fixture(scope="module")
def dense600():
    """600 points in a 640 x 384 frame pair, as test_gpu_errors.py's team case; its pyramids outlive the cycles."""
    sc = synth.make_scene(640, 384, n_points=600, seed=3)
    cam = ic.CamClass(3, sc["fc"], sc["cc"], sc["wh"], 8)
    return sc, cam, ic.Pyramid(sc["img_a"], 2, 8), ic.Pyramid(sc["img_b"], 2, 8)


def test_pyramid(frames):
    lv_f, pad = 2, 8

    def cycle():
        p = ic.Pyramid(frames[0], lv_f, pad, True)
        p.rebuild(frames[1])  # from the host: brings the stage buffer to life
        assert np.isfinite(p.download(lv_f)).all()
        del p

    _check_returns_memory(cycle, _plane7(W, H, pad) + 4 * W * H)


@pytest.mark.parametrize("form", ["team", "timing", "default", "graph"])
def test_track_batch(dense600, form):
    sc, cam, pa, pb = dense600
    B, M = 2, 12000  # T, Gx, Gy: 3 x B x M x 64 floats
    op = ic.optparam(2, 0, 8, 4, 0.0, 0, 0, M)
    P = np.tile(sc["p_a"], (B, 1))

    def cycle():
        e = ic.TrackBatch(cam, op, B)
        for k in range(B):
            e.Set3Dpoints(k, sc["pts3d"].copy())
        if form == "team":
            e.set_team(64)  # the team mailbox and the pinned error flag
        elif form == "timing":
            e.set_timing(True)  # the event vectors
        elif form == "graph":
            e.set_variant(ic.VARIANT_NO_TEAMS)
        e.SetPoseAll(P, pa, pb)
        e.track_async()
        assert np.isfinite(e.poses()).all()
        if form == "team":
            assert e.last_team() > 1
        elif form == "timing":
            assert e.level_times()[1].sum() > 0
        elif form == "graph":
            assert "hipGraph" in e.path_name()
        del e

    _check_returns_memory(cycle, 3 * B * M * 64 * 4)


def _flat_world(cam_fc, cam_cc, n, seed=5):
    """n world points on the plane Z = 10 that the identity pose projects well inside the frame."""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(100, W - 100, n), rng.uniform(100, H - 100, n)
    return np.ascontiguousarray(np.stack([(u - cam_cc[0]) / cam_fc[0] * 10.0, (v - cam_cc[1]) / cam_fc[1] * 10.0,
                                          np.full(n, 10.0)]))


def test_sequence(frames):
    lv_f, psz, cap = 2, 8, 128
    fc, cc = np.array([900.0, 900.0], np.float32), np.array([W / 2, H / 2], np.float32)
    cam = ic.CamClass(lv_f + 1, fc, cc, np.array([W, H], np.int32), psz)
    op = ic.optparam(lv_f, 0, psz, 3, 0.0, 0, 0, cap)
    X = _flat_world(fc, cc, 1000)

    def cycle():
        s = sq.SequenceTracker(cam, op, X, 10)
        s.track_async(frames, np.zeros(6))  # host frames: the owning copy, the result buffers
        out = s.wait()
        assert out["npts"].min() > 0 and out["poses"].shape == (3, 6)
        del s

    # the two ring pyramids' level 0 and the owning copy of the frames
    _check_returns_memory(cycle, 2 * _plane7(W, H, psz) + 3 * 4 * W * H)


def test_sequence_refused_create():
    """psz 16 and a cap above 2048 points: refused after the inner batch exists."""
    lv_f, psz, cap = 1, 16, 6000
    cam = ic.CamClass(lv_f + 1, np.array([100.0, 100.0], np.float32), np.array([80.0, 60.0], np.float32),
                      np.array([160, 120], np.int32), psz)
    op = ic.optparam(lv_f, 0, psz, 3, 0.0, 0, 0, cap)
    X = np.ones((3, 16))

    def cycle():
        with pytest.raises(ic.IctrError, match="has no one-launch form"):
            sq.SequenceTracker(cam, op, X, 1)

    _check_returns_memory(cycle, 3 * cap * 256 * 4, cycles=20)  # the batch's T, Gx, Gy alone


def test_ransac():
    n, smax = 4096, 40000  # the result block holds smax inlier masks of n bits, on the device and pinned
    rng = np.random.default_rng(9)
    fc, cc = np.array([500.0, 500.0]), np.array([320.0, 240.0])
    P3 = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 8, n)])
    xy = np.stack([fc[0] * P3[0] / P3[2] + cc[0], fc[1] * P3[1] / P3[2] + cc[1]])

    def cycle():
        r = ransac.RansacSampler(n, smax)
        r.set_points(xy, P3)
        r.run_async(fc, cc, 4, 256, 1.0, seed=1)
        assert r.wait()["accepted"] == 4  # exact matches: the first trials give the four samples
        del r

    _check_returns_memory(cycle, 8 * smax * (n // 64))


def test_triangulator():
    N, n = 150000, 1000  # sized for N tracks of two views; n are set and run
    rng = np.random.default_rng(4)
    X = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(4, 6, n)], 1)
    P = np.zeros((2, 3, 4), np.float32)
    P[:, :, :3] = np.diag([500.0, 500.0, 1.0])
    P[1, 0, 3] = -250.0  # the second camera half a unit to the right
    xh = np.einsum("fij,nj->fni", P.astype(np.float64), np.hstack([X, np.ones((n, 1))]))
    xy = (xh[:, :, :2] / xh[:, :, 2:]).transpose(1, 0, 2).reshape(-1, 2)  # track-major: point i's views 0, 1
    off, view = 2 * np.arange(n + 1), np.tile([0, 1], n)

    def cycle():
        t = ic.Triangulator(N, 2 * N, 2)
        t.set_cameras(P.reshape(2, 12))
        t.set_tracks(off, view, xy)
        t.run_async("dlt")
        out = t.wait()
        assert np.isfinite(out["pts"]).all() and not out["status"].any()
        del t

    # d_view, d_x, d_y: 4 bytes per observation each; d_in 36, d_out 56, d_off 8 bytes per point
    _check_returns_memory(cycle, 3 * 4 * 2 * N + (36 + 56 + 8) * N)


def test_alignment_engine():
    B, w, h = 1500, 64, 64
    rng = np.random.default_rng(2)
    img = np.kron(rng.integers(0, 256, (8, 8)), np.ones((8, 8))).astype(np.float32)
    pa, pb = ic.Pyramid(img, 1, 4, True), ic.Pyramid(np.roll(img, 1, 1), 1, 4, True)

    def cycle():
        g = icgn.AlignBatch("translation", w, h, 1, 0, 2, 0.0, nproblems=B)
        for k in range(B):
            g.set_frames(k, pa, pb)
        g.run_async()
        assert np.isfinite(g.results()[0]).all()
        del g

    # the H and b partials: 40 + 8 floats per workgroup, max(64, 8192 / B) workgroups per problem
    _check_returns_memory(cycle, 4 * B * max(64, 8192 // B) * 48)


def test_flow_grid(frames):
    pa, pb = ic.Pyramid(frames[0], 1, 8, True), ic.Pyramid(frames[1], 1, 8, True)
    K = W * H  # step 1: one node per pixel

    def cycle():
        g = pf.FlowGrid(W, H, 1).compute(pa, pb, psz=8, lv_f=1, maxiter=2)
        assert g.gather(np.array([[100.5, 200.25], [700.0, 300.0]])).shape == (2, 2)
        del g

    _check_returns_memory(cycle, 4 * 10 * K + K)  # the arena: eight f32 and two i32 per node, one lost byte


def test_point_tracker(frames):
    psz, lv_f, mc = 15, 3, 500

    def cycle():
        t = pf.PointTracker(W, H, bsize=2, maxcorners=mc, lv_f=lv_f, psz=psz, maxiter=3)
        for f in frames:
            t.push_frame(f)
        assert t.frcounter == 2
        tr, va, am = t.read_block(0)  # left the window with the third frame: read from its pinned store block
        assert len(tr) > 0 and tr.shape[1:] == (2, 2) and len(va) == len(am) == len(tr)
        del t

    # the two pyramids' level 0 and the corner picker's f64 response plane
    _check_returns_memory(cycle, 2 * _plane7(W, H, psz) + 8 * W * H)
