"""Every iteration's H and b of every launch form against the float64 judge of tests/iter_judge.py, at the device's own
traced pose.

What the rest of the suite pins after the first iteration is the solver turn on the device's OWN H and b
(parity_util.check_solver_turns) and the final pose; b from the second iteration on -- the warp at the updated pose, the
new-view mask, the bilinear taps of the current frame, the residual, the products and the sums -- was compared with
nothing, and Gauss-Newton's self-correction hides a lost patch or a stale window inside the pose tolerance. Here every
case first runs check_solver_turns, asserts its launch form through path_name(), checks the judge's preconditions bit
for bit (level projections = buffers 100 + level, T/Gx/Gy and coefficient lines = buffers 0, 1, 2, 7, the problem
record's G = the device build of se3_exp at the last p), then holds every record's b and H to the judge in the units of
iter_judge.py. The judge replays the f32 per-pixel arithmetic at the device's f32 pose with the device build of the exp
map, so frames wider than 256 px (tap-selection quirk, see test_gpu_parity.py) are judged step by step as well.

Bar per case, for b and for H separately: max(2, 2 x the worst units the C oracle's f32 Eigen-order run reaches on the
same scene and parameters, judged at its own poses), computed here on the CPU (iter_judge.yardstick); nothing in it
comes from the device. Where the C oracle cannot run a case (robustness options) the bar is the same scene's without
the options. Each case prints the device's worst units (pytest -s); DESIGN.md section 2 records them.

A batch records no trace; its problem 0 is followed through the problem record over runs of 1, 2, ... iterations at one
level (tests/iter_sums_child.py).

Not judged here: dopatchnorm (the patch mean is a 64-term f32 sum in another order and shifts every residual of a patch
by ~1e-4, about 170 units), the stale state across frame pairs (the C oracle owns it), the multi-rank forms.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import invcompcamtrack_amd as ic
import iter_judge as J
import iter_sums_child as child
import parity_util as pu
from parity_util import check_solver_turns, same_bits
from test_gpu_solver import FORMS, SE3_K

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HUBER_K = 6.0
CHILD_TIMEOUT = 120   # seconds; the child takes about one
_child_died = []      # why the child ended on a signal or at its time limit (then the session has been ended)
# form -> (what path_name() must say, what it must not say); teams exist for 8x8 patches only
PATHS = {"one_workgroup": ("k_track1", "workgroups per problem"), "teams16": ("workgroups per problem", "k_iter"),
         "graph": ("hipGraph", "k_track1"), "no_graph": ("k_iter", "hipGraph"), "any_size": ("hipGraph", "k_track1"),
         "h_by_setup": ("hipGraph", "k_track1")}


def _assert_path(form, psz, name):
    want, never = PATHS[form] if not (form == "teams16" and psz != 8) else PATHS["one_workgroup"]
    assert want in name and never not in name, (form, psz, name)


def _device_exp(p):
    return pu.device_se3(np.asarray(p, np.float32).reshape(1, 6), False)[0]


def _host_exp(p):
    return np.asarray(ic.util_SE3_coeff_to_group(np.ascontiguousarray(p, np.float32)), np.float32).reshape(12)


def _ic_cam(cam):
    get = (cam.getfx, cam.getfy, cam.getcx, cam.getcy, cam.getswo, cam.getsho)
    return lambda k, l: get[k](l)


def _preconditions(read, n, M, nv, lv_l):
    """on_setup for the judge: read(which, count) -> the device buffer of the judged problem."""
    def check(detail):
        for l, d in detail.items():
            g = read(100 + l, 2 * M)
            assert same_bits(g[:n], d["mx"]) and same_bits(g[M:M + n], d["my"]), ("projections of level", l)
        d = detail[lv_l]
        for w, key in ((0, "T"), (1, "Gx"), (2, "Gy")):
            assert np.array_equal(read(w, nv * n), d[key].reshape(-1)), ("patch buffer", key)
        coef = read(7, 16 * n).reshape(n, 16)
        assert np.array_equal(coef[:, :6], d["cx"]) and np.array_equal(coef[:, 6:12], d["cy"]), "coefficient lines"
    return check


def _hold(label, res, yard, nrec=None):
    b, H, zeros = J.worst(res)
    bar_b, bar_H = J.bars(*yard)
    print(f"[{label}] device worst b {b:.2f} (bar {bar_b:.2f}) H {H:.2f} (bar {bar_H:.2f}) units over {len(res)} records; "
          f"C oracle f32 order b {yard[0]:.2f} H {yard[1]:.2f}")
    print(f"[{label}] {J.report(res)}")
    assert nrec is None or len(res) == nrec, (label, len(res))
    assert zeros, (label, "an entry with unit 0 is not an exact zero")
    for r in res:
        assert r["H_units"] <= bar_H, (label, "H", r["level"], r["iter"], r["H_units"], bar_H)
        assert r["b_units"] <= bar_b, (label, "b", r["level"], r["iter"], r["b_units"], bar_b)
    return b, H


def _track(oracle, key, sc, form, psz, *, lv_f=2, lv_l=0, maxiter=6, ratio=0.0, donorm=0, robust=None, p0=None,
           variant=None, team=None, path=None, yard_key=None):
    """One tracking on the single-problem engine, judged. form names FORMS' bits unless variant / team / path
    (want, never) are given."""
    O = oracle
    n = sc["pts3d"].shape[1]
    p0 = sc["p_a"] if p0 is None else p0
    if variant is None:
        variant, team = FORMS[form]
    op = ic.optparam(lv_f, lv_l, psz, maxiter, ratio, donorm, 0, n)
    cam = ic.CamClass(lv_f + 1, sc["fc"], sc["cc"], sc["wh"], psz)
    pose = ic.PoseClass(cam, op)
    odo = ic.OdometerClass(pose, op)
    odo.set_variant(variant)
    if team is not None:
        odo.set_team(*team)
    robust = robust or {}
    if robust:
        odo.set_robust(**robust)
    odo.enable_trace()
    gpa, gpb = ic.Pyramid(sc["img_a"], lv_f, psz), ic.Pyramid(sc["img_b"], lv_f, psz)
    odo.Set3Dpoints(np.ascontiguousarray(sc["pts3d"].copy()))
    odo.SetPose(p0, gpa, gpb)
    p_start, G_start = pose.state()
    assert same_bits(G_start, _host_exp(p_start))  # exp0: the host build made the level projections
    pg = odo.TrackPose()
    name = odo.path_name()
    if path is None:
        _assert_path(form, psz, name)
    else:
        assert path[0] in name and (path[1] is None or path[1] not in name), (form, name)
    compose = None
    if robust.get("compositional"):
        e, l = ic.util_SE3_coeff_to_group, ic.util_SE3_group_to_coeff
        compose = (SE3_K, e, l, e, l)
    tr = check_solver_turns(odo, p_start, op, p_final=pg, compose=compose)
    M, nv = op.maxpttrack, op.novals
    st = odo.read_buffer(8, 18)
    assert same_bits(st[:6], tr[-1]["p"]), "the problem record's p is not the last record's"
    assert same_bits(st[6:18], _device_exp(tr[-1]["p"])), "the problem record's G is not the device exp of its p"
    pts = odo.read_buffer(4, 3 * M).reshape(3, M)[:, :n]
    opa, opb = O.Pyramid(sc["img_a"], lv_f, psz), O.Pyramid(sc["img_b"], lv_f, psz)
    res = J.judge(tr, pts, p_start, opa, opb, _ic_cam(cam), psz, _host_exp, _device_exp,
                  huber_k=robust.get("huber_k", 0.0), clean_invisible=bool(robust.get("clean_invisible")),
                  on_setup=_preconditions(odo.read_buffer, n, M, nv, lv_l))
    yard = J.yardstick(O, yard_key or key, sc, lv_f, lv_l, psz, maxiter, ratio, donorm, p0=p0)
    label = f"{key}/{form}/psz{psz}" + (f"/{name}" if path else "")
    _hold(label, res, yard)
    return res


def _named(name, n=None):
    w, h, n0, psz0, lv_f, seed, margin = J.SCENES[name]
    return J.make_scene(w, h, n0 if n is None else n, seed, margin), lv_f


# ------------------------------------------------------------------------------------------- a: every form, three sizes
@pytest.mark.parametrize("psz", [8, 4, 5])
@pytest.mark.parametrize("form", list(FORMS))
def test_every_form_every_iteration(oracle, form, psz):
    """256 x 224, 257 points (not a multiple of 4: the padding lanes), three levels of six iterations."""
    sc, _ = _named("psz8")
    res = _track(oracle, "psz8", sc, form, psz)
    assert len(res) == 18


# ------------------------------------------------------------------------------------------- b: coordinates beyond 256
@pytest.mark.parametrize("psz", [8, 4])
@pytest.mark.parametrize("form", ["one_workgroup", "teams16", "graph"])
def test_frames_wider_than_256_px_step_by_step(oracle, form, psz):
    sc, lv_f = _named("vga")
    res = _track(oracle, "vga", sc, form, psz, lv_f=lv_f)
    assert len(res) == 24
    assert sc["px_a"][:, 0].max() > 256.0


# ------------------------------------------------------------------------------------------- c: the new-view mask
@pytest.mark.parametrize("form", list(FORMS))
def test_points_crossing_the_border_of_the_new_view(oracle, form):
    """Points up to 6 px outside the frame: the count of points in the new view changes between the records
    (test_iter_judge_cpu.py holds the scene to that on the CPU; here the device's own records must show it too)."""
    sc, _ = _named("border")
    res = _track(oracle, "border", sc, form, 8)
    counts = [r["n_new"] for r in res]
    assert len(set(counts)) > 1 and max(counts) < sc["pts3d"].shape[1], counts


# ------------------------------------------------------------------------------------------- d: robustness options
@functools.lru_cache(maxsize=None)
def _occluded_scene():
    from test_gpu_robust_forms import _occluded_scene as f
    return f()


@functools.lru_cache(maxsize=None)
def _view_scene():
    from test_gpu_robust_forms import _view_scene as f
    return f(150, 2.0)


@pytest.mark.parametrize("form", ["one_workgroup", "graph"])
def test_huber_weights_on_outliers(oracle, form):
    sc, p0 = _occluded_scene()
    res = _track(oracle, "occluded", sc, form, 8, maxiter=5, robust=dict(huber_k=HUBER_K), p0=p0)
    assert len(res) == 15


@pytest.mark.parametrize("form", ["one_workgroup", "graph"])
def test_clean_invisible_with_a_third_outside_the_reference_view(oracle, form):
    sc, p0 = _view_scene()
    res = _track(oracle, "view", sc, form, 8, maxiter=5, robust=dict(clean_invisible=True), p0=p0)
    assert max(r["n_new"] for r in res) < 0.85 * sc["pts3d"].shape[1]


def test_compositional_update_b_at_the_traced_pose(oracle):
    sc = pu.scene(256, 224, 150, seed=41, margin=16.0)
    _track(oracle, "seed41", sc, "one_workgroup", 8, maxiter=5, robust=dict(compositional=True))


# ------------------------------------------------------------------------------------------- e: parameters
def test_cloud_normalisation(oracle):
    """donorm = 1: the points as Set3Dpoints left them, the pose in normalised units."""
    sc, _ = _named("psz8")
    _track(oracle, "psz8", sc, "graph", 8, donorm=1)


def test_coarse_last_level(oracle):
    sc, _ = _named("psz8")
    res = _track(oracle, "psz8", sc, "one_workgroup", 8, lv_l=1)
    assert {r["level"] for r in res} == {2, 1}


def test_loop_rule_records(oracle):
    """normdp_ratio = 0.01 with up to ten iterations per level, so that the rule and not maxiter ends every level (the C
    oracle runs 7, 7 and 8): the judge follows whatever records exist."""
    sc, _ = _named("psz8")
    res = _track(oracle, "psz8", sc, "teams16", 8, maxiter=10, ratio=0.01)
    per_level = [sum(r["level"] == l for r in res) for l in (2, 1, 0)]
    assert all(2 <= k < 10 for k in per_level), per_level


# ------------------------------------------------------------------------------------------- f: beyond one workgroup
def test_one_launch_tracker_with_templates_in_global_memory(oracle):
    """900 points: k_track1<false> re-reads T, Gx, Gy from the patch buffers."""
    sc, _ = _named("psz8", n=900)
    _track(oracle, "psz8x900", sc, "k_track1", 8, variant=ic.VARIANT_ONE_LAUNCH | ic.VARIANT_NO_TEAMS,
           path=("k_track1", "workgroups per problem"))


def test_one_launch_tracker_with_the_librarys_own_team(oracle):
    sc, _ = _named("psz8", n=2500)
    _track(oracle, "psz8x2500", sc, "team", 8, variant=ic.VARIANT_ONE_LAUNCH, path=("workgroups per problem", "k_iter"))


# ------------------------------------------------------------------------------------------- g: 8200 points
# Sixteen or thirty-two patches per wave: path_name() says k_level_resident for both and nothing else exposes the
# geometry. It follows from resident_plan (ictr_host.hip): sixteen only when all pairs of the batch are then in flight
# (slots >= B), so the single problem here runs with sixteen and the two pairs behind one slot (last case of this file)
# with thirty-two. A change of that plan must revisit both cases.
@pytest.mark.parametrize("psz,variant,path", [
    (8, 0, ("k_level_resident", None)),                                            # sixteen patches per wave
    (8, ic.VARIANT_NO_RESIDENT, ("hipGraph", "k_level_resident")),                  # k_iter8 under the graph
    (8, ic.VARIANT_LAUNCHES | ic.VARIANT_NO_GRAPH, ("k_iter", "hipGraph")),
    (4, 0, ("k_iter", "k_level_resident")),                                         # k_iter4
], ids=["resident", "no_resident", "launches", "psz4"])
def test_8200_points(oracle, psz, variant, path):
    sc, _ = _named("8200")
    res = _track(oracle, "8200", sc, "8200", psz, maxiter=5, variant=variant, path=path)
    assert len(res) == 15


# ------------------------------------------------------------------------------------------- h, i: batches
def _judge_batch(oracle, label, sc, inp, got, path_want):
    O = oracle
    name = str(got["path"])
    assert path_want in name, name
    psz, maxiter, n = int(inp["psz"]), int(inp["maxiter"]), sc["pts3d"].shape[1]
    p_start = np.asarray(inp["poses"][0], np.float32)  # host_setpose stores float32(p_in)
    p_prev, tr = p_start, []
    for m in range(maxiter):
        H, b, dp, p = got["H"][m], got["b"][m], got["dp"][m], got["p"][m]
        assert same_bits(H, H.T) and same_bits(H, got["H"][0]), ("H", m)
        assert same_bits(dp, ic.solve6(H, b)), ("dp is not the serial solve of the record's H, b", m)
        assert same_bits(p, (p_prev + dp).astype(np.float32)), ("p != f32(p of the shorter run + dp)", m)
        assert same_bits(got["G"][m], _device_exp(p)), ("the problem record's G", m)
        tr.append(dict(level=0, iter=m, H=H, b=b, dp=dp, p=p))
        p_prev = p
    cam = O.Tracker(O.make_op(0, 0, psz, maxiter, 0.0, 0, 0, n), sc["fc"], sc["cc"], sc["wh"])
    M = n  # (the buffers below are already cut to n points)
    bufs = {100: got["pt2d"].reshape(-1), 0: got["T"], 1: got["Gx"], 2: got["Gy"], 7: got["coef"]}
    read = lambda which, count: np.asarray(bufs[which]).reshape(-1)[:count]
    try:
        res = J.judge(tr, got["pts3d"], p_start, O.Pyramid(sc["img_a"], 0, psz), O.Pyramid(sc["img_b"], 0, psz),
                      cam.cam_get, psz, _host_exp, _device_exp, on_setup=_preconditions(read, n, M, psz * psz, 0))
    finally:
        cam.close()
    yard = J.yardstick(O, label, sc, 0, 0, psz, maxiter, p0=inp["poses"][0])
    _hold(f"{label}/{name.split(' ')[0]}", res, yard, nrec=maxiter)


def _batch_input(sc, B, maxiter):
    poses = sc["p_a"][None, :] + np.random.default_rng(4).normal(0, 1e-3, (B, 6))
    poses[0] = sc["p_a"]
    return dict(img_a=sc["img_a"], img_b=sc["img_b"], fc=sc["fc"], cc=sc["cc"], wh=sc["wh"], pts=sc["pts3d"], poses=poses,
                psz=np.int32(8), maxiter=np.int32(maxiter))


def test_big_batch_resident_form(oracle):
    """96 problems of 500 points (48 000 together): the resident form for batches of mid-size problems."""
    sc, _ = _named("psz8", n=500)
    inp = _batch_input(sc, 96, 4)
    _judge_batch(oracle, "500x96", sc, inp, child.run(inp), "k_level_resident")


def test_resident_form_32_patches_per_wave_one_slot_two_pairs(oracle, tmp_path):
    """Two pairs of 8200 points with one pair in flight per launch (ICTR_RESIDENT_SLOTS=1, read once per process: a
    fresh child): thirty-two patches per wave, and the slot walks through both pairs. The last case of this file: a
    child that ends on a signal or at its time limit may have faulted or hung the device, so nothing is started on it
    afterwards -- the whole session ends there."""
    sc, _ = _named("8200")
    inp = _batch_input(sc, 2, 4)
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, **inp)
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "iter_sums_child.py"), "1", src, dst],
                           env=dict(os.environ, ICTR_RESIDENT_SLOTS="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=CHILD_TIMEOUT)
        died = f"ended on signal {-r.returncode}:\n{r.stdout[-3000:]}" if r.returncode < 0 else None
    except subprocess.TimeoutExpired:
        died = f"ran into its time limit of {CHILD_TIMEOUT} s"
    if died:
        _child_died.append(died)
        pytest.exit(f"the ICTR_RESIDENT_SLOTS=1 child {died}\nno further GPU work is started in this session", returncode=1)
    assert r.returncode == 0, r.stdout[-4000:]
    _judge_batch(oracle, "8200x2/slots1", sc, inp, dict(np.load(dst)), "k_level_resident")
