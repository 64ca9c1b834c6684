"""Lockstep sets of coarse-to-fine flows on the device (patchflow.CoarseToFineFlowSet, ictr_c2fset_*; the kernels of
csrc/ictr_c2fflow.hip, ictr_c2fflow_robust.hip, ictr_frontend.hip, ictr_densify.hip and ictr_flowrefine.hip at members
1 .. 7, where a single object's run is member 0 alone).

The judge of a set is each member's own ``run`` on the same pyramids (an object of its own, made with the same parameters),
and the single objects keep their own judges, the f32 restatements of the other test files. Every comparison is bit for bit
and leaves nothing out: per level the field, the node displacements after the fill and the status bytes, the node bias
under patnorm, and the final field. Every member has content of its own (a seeded texture and shift per member), and the
single runs are asserted to differ from each other at every level, so that no mix-up between members can pass.

The device pyramids are built from the host pyramids' planes, as in the other coarse-to-fine tests."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import flowrefine_cases as FC
import invcompcamtrack_amd as ic
from invcompcamtrack_amd import _lib
from invcompcamtrack_amd import patchflow as pf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = 4
REFINE = dict(n_outer=1, n_sor=2)
SCRIPT = dict(patnorm=True, channels=3, cost="huber", huber_k=5.0, lv_l=1, refine=REFINE)  # the script's own settings

# (w, h, lv_f, psz, members, parameters). 33x17 at lv_f 1: level 1 is 16 x 8 with 4 x 2 nodes, fewer than one workgroup's;
# 67x53 halves oddly twice; psz 8 / 15 / 17 are the forms <1,1>, <4,1>, <8,2>; 1, 2, 3 and 8 members.
CASES = (
    (33, 17, 1, 8, 1, {}),
    (33, 17, 1, 8, 2, {}),
    (67, 53, 2, 17, 3, {}),
    (100, 77, 2, 15, 8, {}),
    (67, 53, 2, 15, 2, dict(patnorm=True)),
    (67, 53, 2, 8, 2, dict(x_only=True)),
    (33, 17, 1, 8, 2, dict(channels=3)),
    (67, 53, 2, 17, 2, dict(cost="huber", huber_k=5.0)),
    (67, 53, 2, 8, 3, dict(lv_l=1)),
    (67, 53, 2, 15, 2, dict(refine=REFINE)),
    (67, 53, 2, 8, 2, SCRIPT),
    (67, 53, 2, 15, 2, dict(SCRIPT, x_only=True)),
)


def case_id(case):
    w, h, lv_f, psz, n, kw = case
    return f"{w}x{h}-lv{lv_f}-psz{psz}-n{n}" + "".join(f"-{k}" for k in sorted(kw) if k != "huber_k")


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):  # the host pyramids are the oracle's
    return oracle


_pyrs = {}


def pyramid(w, h, lv_f, pad, seed, shift=(0.0, 0.0)):
    """A device pyramid of a seeded texture sampled at (x + shift), built from the host pyramid's planes; shared."""
    from oracle import oracle as O
    key = (w, h, lv_f, pad, seed, shift)
    if key not in _pyrs:
        img = FC._noisy(FC.texture(w, h, seed, lambda X, Y: (X + shift[0], Y + shift[1])), seed + 7, 0.5)
        o = O.Pyramid(img, lv_f, pad)
        _pyrs[key] = ic.Pyramid(lv_f=lv_f, imgpadding=pad, wh=(w, h), host_planes=(o.img, o.dx, o.dy))
    return _pyrs[key]


def member_pairs(case, base=0):
    """One (A, B) per member, every member a texture and a shift of its own; triples of pyramids on colour members."""
    w, h, lv_f, psz, n, kw = case
    out = []
    for m in range(n):
        shift = (0.9 + 0.45 * m, -0.6 + 0.35 * m)
        seeds = [900 + base + 10 * m + c for c in range(kw.get("channels", 1))]
        a = [pyramid(w, h, lv_f, psz + 1, s) for s in seeds]
        b = [pyramid(w, h, lv_f, psz + 1, s, shift) for s in seeds]
        out.append((a, b) if len(seeds) == 3 else (a[0], b[0]))
    return out


def flow(case, **over):
    w, h, lv_f, psz, _, kw = case
    return pf.CoarseToFineFlow(w, h, lv_f, STEP, psz, **dict(kw, **over))


def snapshot(c):
    """Everything a run leaves in an object, as bytes: per level the field, d and status (and the bias), and the result."""
    out = {}
    for l in range(c.lv_f, c.lv_l - 1, -1):
        f, d, st = c.level(l)
        out[l, "field"], out[l, "d"], out[l, "status"] = f.tobytes(), d.tobytes(), st.tobytes()
        if c.patnorm:
            out[l, "bias"] = c.level_bias(l).tobytes()
    out["dense"] = c.dense().tobytes()
    return out


_judged = {}


def judge(case, pairs, key):
    """The single runs' snapshots, one object per member; computed once per key and left unchanged."""
    if key not in _judged:
        _judged[key] = [snapshot(flow(case).run(a, b)) for a, b in pairs]
    return _judged[key]


def same_as_judge(flows, want, what):
    for m, (c, w) in enumerate(zip(flows, want)):
        got = snapshot(c)
        assert got.keys() == w.keys()
        for k in w:
            assert got[k] == w[k], (what, "member", m, k)


def members_differ(want):
    for i in range(len(want)):
        for j in range(i):
            for k in want[i]:
                if k != "dense" and k[1] in ("field", "d"):
                    assert want[i][k] != want[j][k], ("members agree", i, j, k)


# ---------------------------------------------------------------- the table, bit for bit
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_lockstep_run_has_every_members_own_bits(case):
    pairs = member_pairs(case)
    want = judge(case, pairs, case_id(case))
    members_differ(want)
    flows = [flow(case) for _ in pairs]
    s = pf.CoarseToFineFlowSet(flows)
    assert len(s) == case[4] and s.members == tuple(flows) and s.operations() == 0
    assert s.run(pairs) is s
    same_as_judge(flows, want, case_id(case))
    if case[5].get("lv_l"):
        assert all(c.lv_l == 1 and c.dense().shape == (case[1], case[0], 2) for c in flows)
    for c in flows:  # a member's own stage times are zeros behind a lockstep run
        assert not c.kernel_ms().any() and c.upsample_ms() == 0.0


def test_stereo_arrangement_on_shared_pyramids():
    """Three pyramids, four members (P0, P1), (P1, P0), (P1, P2), (P2, P1): A of one member is B of another."""
    case = (67, 53, 2, 8, 4, {})
    p = [pyramid(67, 53, 2, 9, 950, (1.1 * k, -0.4 * k)) for k in range(3)]
    pairs = [(p[0], p[1]), (p[1], p[0]), (p[1], p[2]), (p[2], p[1])]
    want = judge(case, pairs, "stereo arrangement")
    members_differ(want)
    flows = [flow(case) for _ in pairs]
    pf.CoarseToFineFlowSet(flows).run(pairs)
    same_as_judge(flows, want, "stereo arrangement")


# ---------------------------------------------------------------- run sequences, streams, counts and times
def test_twice_then_a_members_own_run_then_lockstep_again_and_on_a_stream():
    from test_gpu_flowrefine import _hip_runtime
    case = CASES[9]  # refined, <4,1>
    pairs, other = member_pairs(case), member_pairs(case, base=500)
    want, want_other = judge(case, pairs, case_id(case)), judge(case, other, case_id(case) + "-other")
    assert want[0]["dense"] != want_other[0]["dense"]
    flows = [flow(case) for _ in pairs]
    s = pf.CoarseToFineFlowSet(flows)
    same_as_judge(s.run(pairs).members, want, "first")
    same_as_judge(s.run(pairs).members, want, "twice")
    flows[0].set_timing(True)
    flows[0].run(*other[0])  # one member on other frames, on its own
    same_as_judge(flows, [want_other[0], want[1]], "a member's own run")
    assert flows[0].kernel_ms()[:, 0].all()
    same_as_judge(s.run(other).members, want_other, "lockstep on the other frames")
    assert not flows[0].kernel_ms().any()
    hip, stream = _hip_runtime(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and stream.value
    try:
        same_as_judge(s.run(pairs, stream=stream.value).members, want, "on a stream")
    finally:
        assert hip.hipStreamDestroy(stream) == 0


def test_a_set_of_one_and_the_objects_own_run_alternate_on_one_object():
    """33 x 17, lv_f 1, psz 8, refined: the set, the object's own timed run, the set again, all on one object and one
    pair: the same bytes each time, and stage times only behind the object's own run."""
    case = (33, 17, 1, 8, 1, dict(refine=REFINE))
    (pair,) = member_pairs(case)
    c = flow(case)
    c.set_timing(True)
    s = pf.CoarseToFineFlowSet([c])
    first = snapshot(s.run([pair]).members[0])
    assert not c.kernel_ms().any() and c.upsample_ms() == 0.0
    own = snapshot(c.run(*pair))
    ms = c.kernel_ms()
    print("own kernel_ms", ms.tolist())
    assert ms.shape == (2, 3) and (ms > 0).all()
    again = snapshot(s.run([pair]).members[0])
    assert not c.kernel_ms().any() and not s.kernel_ms().any()  # (the set's own timing is off)
    assert first == own == again
    assert first == judge(case, [pair], case_id(case))[0]


def test_operations_do_not_depend_on_the_member_count():
    """Kernel launches plus memsets of a run: per level the search, the memset of rowhas, the fill's two launches and the
    densifier, 5; refined, k_fr_init and k_fr_final and per outer iteration the warp, the coefficients and 2 n_sor
    half-sweeps more; above level 0 one up-sampling."""
    for case, per_level, up in ((CASES[3], 5, 0), (CASES[9], 5 + 2 + 1 * (2 + 2 * 2), 0), (CASES[8], 5, 1)):
        w, h, lv_f, psz, _, kw = case
        ops = []
        for n in (1, 8):
            c = (w, h, lv_f, psz, n, kw)
            flows = [flow(c) for _ in range(n)]
            ops.append(pf.CoarseToFineFlowSet(flows).run(member_pairs(c)).operations())
        assert ops[0] == ops[1] == per_level * (lv_f - kw.get("lv_l", 0) + 1) + up, (case_id(case), ops)


def test_kernel_ms_of_a_timed_run():
    case = CASES[10]  # lv_l = 1, refined
    pairs = member_pairs(case)
    flows = [flow(case) for _ in pairs]
    s = pf.CoarseToFineFlowSet(flows)
    assert not s.run(pairs).kernel_ms().any() and s.upsample_ms() == 0.0  # timing off
    s.set_timing(True)
    ms = s.run(pairs).kernel_ms()
    print("set kernel_ms", ms.tolist(), "upsample", s.upsample_ms())
    assert ms.shape == (3, 3) and (ms[1:] > 0).all() and not ms[0].any() and s.upsample_ms() > 0
    same_as_judge(flows, judge(case, pairs, case_id(case)), "timed")
    s.set_timing(False)
    assert not s.run(pairs).kernel_ms().any()


# ---------------------------------------------------------------- refusals
def test_refusals_name_the_member_and_the_field_and_change_nothing():
    case = CASES[4]  # patnorm, two members
    w, h, lv_f, psz, n, kw = case
    pairs = member_pairs(case)
    want = judge(case, pairs, case_id(case))
    flows = [flow(case) for _ in pairs]
    L = _lib.load()

    def create(objs, count=None):
        hs, arr = C.c_void_p(), (C.c_void_p * max(len(objs), 1))(*[o._h.value if o is not None else None for o in objs])
        rc = L.ictr_c2fset_create(C.byref(hs), arr, len(objs) if count is None else count)
        msg = L.ictr_last_error().decode() if rc else ""
        if not rc:
            L.ictr_c2fset_destroy(hs)
        return rc, msg

    nine = [flow(case) for _ in range(9)]
    for objs, count, why in (([], None, "n is 0 (1 .. 8)"), (nine, None, "n is 9 (1 .. 8)"),
                             ([flows[0], None], None, "member 1 is NULL"),
                             ([flows[0], flows[1], flows[0]], None, "member 2 is the same object as member 0")):
        rc, msg = create(objs, count)
        assert rc != 0 and why in msg, msg
    assert L.ictr_c2fset_create(None, None, 1) != 0
    assert L.ictr_c2fset_create(C.byref(C.c_void_p()), None, 1) != 0 and b"members is NULL" in L.ictr_last_error()
    differing = (("w", dict(), (w + 1, h)), ("h", dict(), (w, h + 1)), ("lv_f", dict(lv_f=1), None),
                 ("lv_l", dict(lv_l=1), None), ("step", dict(step=5), None), ("psz", dict(psz=9), None),
                 ("maxiter", dict(maxiter=9), None), ("eps", dict(eps=0.02), None),
                 ("the densifier's minerr", dict(densify=dict(minerr=3.0)), None),
                 ("the densifier's power", dict(densify=dict(power=2)), None), ("refine", dict(refine={}), None),
                 ("patnorm", dict(patnorm=False), None), ("x_only", dict(x_only=True), None),
                 ("channels", dict(channels=3), None), ("cost", dict(cost="huber"), None))
    for field, over, size in differing:
        p = dict(maxiter=10, eps=0.01, **kw)
        geom = dict(lv_f=lv_f, step=STEP, psz=psz)
        for k in list(over):
            if k in geom:
                geom[k] = over.pop(k)
        p.update(over)
        odd = pf.CoarseToFineFlow(*(size or (w, h)), geom["lv_f"], geom["step"], geom["psz"], **p)
        rc, msg = create([flows[0], odd])
        assert rc != 0 and f"member 1 differs from member 0 in {field} (" in msg, (field, msg)
    base = dict(kw, refine={})
    for name, value in (("alpha", 17.0), ("gamma", 12.0), ("delta", 4.0), ("n_outer", 7), ("n_sor", 4), ("omega", 1.5)):
        a, b = flow(case, **base), flow(case, **dict(base, refine={name: value}))
        rc, msg = create([a, b])
        assert rc != 0 and f"member 1 differs from member 0 in the refinement's {name} (" in msg, msg
    rc, msg = create([flow(case, cost="huber", huber_k=5.0), flow(case, cost="huber", huber_k=4.0)])
    assert rc != 0 and "member 1 differs from member 0 in huber_k (4, member 0 has 5)" in msg, msg
    with pytest.raises(ValueError, match="0 members"):
        pf.CoarseToFineFlowSet([])
    with pytest.raises(ValueError, match="member 1 is the same object as member 0"):
        pf.CoarseToFineFlowSet([flows[0], flows[0]])
    with pytest.raises(TypeError, match="member 1 is a int"):
        pf.CoarseToFineFlowSet([flows[0], 3])

    # at run: members are compared again, the channel count and the pyramids are checked; nothing is touched
    s = pf.CoarseToFineFlowSet(flows)
    tabs = [(C.c_void_p * n)(*[p[k]._h.value for p in pairs]) for k in (0, 1)]
    assert L.ictr_c2fset_run(None, tabs[0], tabs[1], None) != 0 and b"the set is NULL" in L.ictr_last_error()
    assert L.ictr_c2fset_run(s._h, None, tabs[1], None) != 0 and b"pyramid table is NULL" in L.ictr_last_error()
    assert L.ictr_c2fset_run_rgb(s._h, tabs[0], tabs[1], None) != 0
    assert b"the members have 1 channel; a grey run is ictr_c2fset_run" in L.ictr_last_error()
    flows[1].set_cost("huber", 3.0)  # a member's setter between create and run
    with pytest.raises(_lib.IctrError, match="c2fset_run: member 1 differs from member 0 in cost"):
        s.run(pairs)
    flows[1].set_cost("l2", 5.0)
    small = pyramid(33, 17, lv_f, psz + 1, 901)
    with pytest.raises(_lib.IctrError, match="c2fset_run: member 1: level 0 of the pyramids is 33 x 17, of the object 67 x 53"):
        s.run([pairs[0], (small, small)])
    with pytest.raises(ValueError, match="1 pairs for 2 members"):
        s.run(pairs[:1])
    with pytest.raises(ValueError, match="colour needs channels=3"):
        s.run([pairs[0], ([pairs[1][0]] * 3, [pairs[1][1]] * 3)])
    assert s.operations() == 0
    with pytest.raises(_lib.IctrError, match="no run yet"):
        flows[0].dense()
    with pytest.raises(_lib.IctrError, match="no run yet"):
        s.kernel_ms()
    colour = (33, 17, 1, 8, 2, dict(channels=3))
    cs = pf.CoarseToFineFlowSet([flow(colour) for _ in range(2)])
    grey = pyramid(33, 17, 1, 9, 902)
    t = (C.c_void_p * 6)(*[grey._h.value] * 6)
    assert L.ictr_c2fset_run(cs._h, t, t, None) != 0
    assert b"the members have 3 channels; a colour run is ictr_c2fset_run_rgb" in L.ictr_last_error()
    with pytest.raises(ValueError, match="with channels=3 a frame is three pyramids"):
        cs.run([(grey, grey)] * 2)
    # and the lockstep run behind all of it has the judge's bits
    same_as_judge(s.run(pairs).members, want, "after the refusals")


# ---------------------------------------------------------------- the stereo pipeline and the CLI
def _same(got, want):
    assert got[1].tobytes() == want[1].tobytes()
    assert got[0].tobytes() == want[0].tobytes()


def test_window_in_lockstep(tmp_path):
    """StereoPointTracker(lockstep=True) on test_gpu_c2fflow's rendered 64 x 96 stereo sequence (psz 8, lv_f 2, four
    frames): the window is lockstep=False's, bit for bit, with flow="c2f" and "c2f-1d"; and the CLI's file is."""
    from invcompcamtrack_amd import run_stereo_track as RS
    from invcompcamtrack_amd import stereotrack as S
    from test_gpu_stereotrack import _stereo_frames
    left, right = _stereo_frames()

    def window(**extra):
        t = S.StereoPointTracker(96, 64, 4, step=4, psz=8, lv_f=2, **extra)
        for a, b in zip(left, right):
            t.push_frames(a, b)
        return t, t.window()

    for kw in (dict(flow="c2f"), dict(flow="c2f-1d"), dict(flow="c2f", refine=REFINE, patnorm=True, keep_grids=True)):
        _, want = window(**kw)
        t, got = window(lockstep=True, **kw)
        assert t.lockstep and len(want[1]) > 100
        _same(got, want)
    assert not S.StereoPointTracker(96, 64, 4, flow="c2f").lockstep
    with pytest.raises(ValueError, match="lockstep=True needs flow='c2f' or 'c2f-1d'"):
        S.StereoPointTracker(96, 64, 4, flow="grid", lockstep=True)
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        for k, (a, b) in enumerate(zip(left, right)):
            np.save(str(tmp_path / f"l{k}.npy"), a)
            np.save(str(tmp_path / f"r{k}.npy"), b)
            f.write(f"{tmp_path / f'l{k}.npy'} {tmp_path / f'r{k}.npy'}\n")
    out = [str(tmp_path / "plain.npz"), str(tmp_path / "lockstep.npz")]
    for flow_name in ("c2f", "c2f-1d"):
        for o, extra in zip(out, ([], ["--lockstep"])):
            assert RS.main([lst, o, "--bsize", "4", "--psz", "8", "--lv_f", "2", "--flow", flow_name] + extra) == 0
        with np.load(out[0]) as a, np.load(out[1]) as b:
            assert len(a["rows"]) > 100
            _same((b["xy_t"], b["rows"]), (a["xy_t"], a["rows"]))
    with pytest.raises(SystemExit):
        RS.main([lst, out[1], "--bsize", "4", "--psz", "8", "--lv_f", "2", "--lockstep"])


# ---------------------------------------------------------------- the C++ facade
def test_cxx_driver(tmp_path):
    """tests/cxx/c2fset_driver.cpp (CTR::CoarseFlowSet of include/ctr_shim.hpp) checks the facade's refusals and prints the
    Python call's bits."""
    exe = str(tmp_path / "c2fset_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "c2fset_driver.cpp"),
                           "-L" + os.path.join(ROOT, "invcompcamtrack_amd"), "-l:libictr_hip.so",
                           "-Wl,-rpath," + os.path.join(ROOT, "invcompcamtrack_amd")], timeout=300)
    w, h, lv_f, n = 67, 53, 2, 3
    imgs = [FC._noisy(FC.texture(w, h, 970, lambda X, Y, k=k: (X + 1.2 * k, Y - 0.5 * k)), 971 + k, 0.5) for k in range(n + 1)]
    frames = str(tmp_path / "frames.f32")
    np.stack(imgs).astype(np.float32).tofile(frames)
    for psz, patnorm in ((8, 0), (17, 1)):
        pad = psz + 1
        r = subprocess.run([exe, frames, str(w), str(h), str(pad), str(lv_f), str(STEP), str(psz), str(n), str(patnorm)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.splitlines()
        pyr = [ic.Pyramid(np.ascontiguousarray(i), lv_f, pad, True) for i in imgs]
        flows = [pf.CoarseToFineFlow(w, h, lv_f, STEP, psz, patnorm=bool(patnorm)) for _ in range(n)]
        s = pf.CoarseToFineFlowSet(flows).run([(pyr[m], pyr[m + 1]) for m in range(n)])
        assert lines[0] == f"ops {s.operations()}"
        per = w * h + lv_f + 1
        assert len(lines) == 1 + n * per
        for m, c in enumerate(flows):
            mine = lines[1 + m * per:1 + (m + 1) * per]
            got = np.array([[float.fromhex(t) for t in ln.split()] for ln in mine[:w * h]], np.float32)
            assert got.reshape(h, w, 2).tobytes() == c.dense().tobytes(), (psz, m)
            for ln, level in zip(mine[w * h:], range(lv_f, -1, -1)):
                tok = ln.split()
                assert [int(t) for t in tok[1:7]] == [level] + np.bincount(c.level(level)[2].ravel(), minlength=5).tolist()
                d = np.array([float.fromhex(t) for t in tok[7:]], np.float32)
                assert d.tobytes() == c.level(level)[1].tobytes(), (psz, m, level)
