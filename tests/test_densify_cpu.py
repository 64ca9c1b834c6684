"""Densification of a flow grid without a GPU: the definition (patchflow.densify_flow_host), the f32 restatement of the
kernel (densify_f32.py) against it over the case table, the injectable defects, the exact properties of the rule and the
usefulness bars.

Every figure that densify_cases.py records is measured again here and printed; a figure above its record fails, and so
does one below half of it (the record is stale)."""
from __future__ import annotations

import numpy as np
import pytest

import densify_cases as DC
import densify_f32 as R
import flowrefine_cases as FC
from invcompcamtrack_amd import patchflow as pf


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):  # the "tracked" tables and the usefulness scenes are tracked by the host oracle
    return oracle


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _both(a, b, d, lost, step, psz, **kw):
    """(definition, restatement) on one table."""
    h, w = a.shape
    return (pf.densify_flow_host(a, b, d, lost, step, psz, **kw),
            R.densify(a, b, DC.filled(d, lost, w, h, step), lost, step, psz, **kw))


# ---------------------------------------------------------------- the restatement against the definition
def test_restatement_differences_are_within_their_records():
    worst = {p: [0.0, 0.0] for p in DC.POWERS}
    share = 0.0
    for case in DC.TABLE:
        got, st = DC.restated(*case)
        e_f, e_w, same = DC.differences(case, got, st)
        assert same, (case, "the vote counts differ outside the near pixels")
        w = worst[case[4]]
        w[0], w[1] = max(w[0], e_f), max(w[1], e_w)
        share = max(share, float(DC.host_run(*case)[2].mean()))
    print("differences per power (field px, summed weight relative):",
          {p: (float(f"{v[0]:.3g}"), float(f"{v[1]:.3g}")) for p, v in worst.items()}, "worst near share", f"{share:.4%}")
    assert share <= DC.BOUNDARY_SHARE and DC.NEAR_SHARE / 2 <= share <= DC.NEAR_SHARE, (share, DC.NEAR_SHARE)
    for p, (rf, rw) in DC.DIFF.items():
        assert worst[p][0] <= rf and worst[p][1] <= rw, (p, worst[p], (rf, rw))
        assert worst[p][0] >= rf / 2 and worst[p][1] >= rw / 2, (p, "the record is stale", worst[p], (rf, rw))


def test_the_table_covers_what_it_names():
    seen = {(c[1], c[2]) for c in DC.TABLE}
    assert seen == set(DC.GEOMS)
    for frame in DC.FRAMES:
        assert {(c[1], c[2]) for c in DC.TABLE if c[0] == frame} == set(DC.GEOMS)
    assert {c[3] for c in DC.TABLE} == set(DC.KINDS) and {c[4] for c in DC.TABLE} == set(DC.POWERS)
    out = 0
    for case in DC.TABLE:
        if case[3] != "outside" or case[0] == "9x7":
            continue
        # votes are dropped at each of the four sides: fewer votes than the same table takes without the inside test
        cnt = DC.host_run(*case)[1]["count"]
        free = {}
        a, b = FC.pair(case[0])
        d, lost = DC.nodes(case[0], case[1], "outside")
        h, w = a.shape
        R.densify(a, b, DC.filled(d, lost, w, h, case[1]), lost, case[1], case[2], defect="inside", stages=free)
        less = free["count"] > cnt
        if case[2] >= case[1]:
            assert less[:, :w // 4].any() and less[:, -(w // 4):].any() and less[:h // 4].any() and less[-(h // 4):].any(), case
            out += 1
    assert out >= 8


# ---------------------------------------------------------------- every injectable defect is seen
DEFECT_CASES = tuple(c for c in DC.TABLE if c[0] in ("100x77", "67x53") and (c[1], c[2]) in ((4, 15), (5, 4), (8, 8))
                     and c[3] in ("smooth", "outside", "toprows"))


def _checks(defect):
    """{check: passed}: the CPU module's checks against the definition, and the GPU module's (the clean restatement's bits,
    which is what the device is held to), applied to the restatement with a defect."""
    out = {}
    for case in DEFECT_CASES:
        got, st = DC.restated(*case, defect=defect)
        e_f, e_w, same = DC.differences(case, got, st)
        name = " ".join(map(str, case))
        out[f"field {name}"] = e_f <= DC.DIFF[case[4]][0]
        out[f"wsum {name}"] = e_w <= DC.DIFF[case[4]][1]
        out[f"count {name}"] = same
        ref, rst = DC.restated(*case)
        out[f"bits {name}"] = bool(np.array_equal(_bits(got), _bits(ref)) and np.array_equal(st["count"], rst["count"])
                                   and np.array_equal(_bits(st["wsum"]), _bits(rst["wsum"])))
    return out


def test_the_checks_pass_without_a_defect():
    assert len(DEFECT_CASES) >= 6
    res = _checks(None)
    assert all(res.values()), res


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_each_defect_is_seen(defect):
    res = _checks(defect)
    seen = sorted(k for k, ok in res.items() if not ok)
    against_definition = [k for k in seen if not k.startswith("bits")]
    print(defect, "seen by", len(seen), "checks,", len(against_definition), "of them against the definition:", seen[:6])
    assert any(k.startswith("bits") for k in seen), (defect, "the device's check does not see it")
    if defect != "order":  # a reversed order is a rounding difference: only the bits show it
        assert against_definition, (defect, "no check against the definition sees it")


# ---------------------------------------------------------------- the exact properties of the rule
FRAME = "67x53"


def _pair_table(step, kind="lost0"):
    a, b = FC.pair(FRAME)
    d, lost = DC.nodes(FRAME, step, kind)
    return a, b, d, lost


@pytest.mark.parametrize("step,psz", DC.GEOMS)
def test_every_node_lost_gives_dense_flows_bits(step, psz):
    a, b, d, _ = _pair_table(step)
    lost = np.ones(d.shape[:2], bool)
    h, w = a.shape
    want = pf._dense_from_nodes(d.copy(), lost, w, h, step)
    for got in _both(a, b, d, lost, step, psz):
        assert np.array_equal(_bits(got), _bits(want))
    assert not want.any()  # nothing to fill from


@pytest.mark.parametrize("step", (8, 4, 2))
@pytest.mark.parametrize("kind", ("lost0", "smooth", "outside"))
def test_a_tiling_gives_each_pixel_its_nodes_bits(step, kind):
    """psz = step, even: one vote per pixel; it takes its node's displacement bits where the node is not lost and the vote
    is inside, the fallback elsewhere."""
    a, b, d, lost = _pair_table(step, kind)
    h, w = a.shape
    ny, nx = lost.shape
    yy, xx = np.mgrid[0:h, 0:w]
    j, i = np.minimum(yy // step, ny - 1), np.minimum(xx // step, nx - 1)
    covered = (yy // step < ny) & (xx // step < nx)
    dn = d[j, i]
    px, py = xx + dn[..., 0].astype(np.float64), yy + dn[..., 1].astype(np.float64)
    takes = covered & ~lost[j, i] & (px >= 0) & (px <= w - 1) & (py >= 0) & (py <= h - 1)
    up = pf._dense_from_nodes(d.copy(), lost, w, h, step)
    assert takes.any() and (kind == "lost0" or (~takes).any())
    for got in _both(a, b, d, lost, step, step):
        assert np.array_equal(_bits(got)[takes], _bits(dn)[takes])
        assert np.array_equal(_bits(got)[~takes], _bits(up)[~takes])


def test_stripes_take_the_fallback():
    """psz < step: the pixels no footprint reaches take dense_flow's value."""
    step, psz = 5, 4
    a, b, d, lost = _pair_table(step)
    h, w = a.shape
    up = pf._dense_from_nodes(d.copy(), lost, w, h, step)
    yy, xx = np.mgrid[0:h, 0:w]
    stripe = (xx % step == step - 1) | (yy % step == step - 1)  # a node at 2 + 5 i covers 5 i .. 5 i + 3
    st = {}
    got = pf.densify_flow_host(a, b, d, lost, step, psz, _stages=st)
    assert (st["count"][stripe] == 0).all() and (st["count"][~stripe] <= 1).all() and (st["count"][~stripe] == 1).any()
    rs = {}
    res = R.densify(a, b, d, lost, step, psz, stages=rs)
    assert np.array_equal(rs["count"], st["count"])
    for f in (got, res):
        assert np.array_equal(_bits(f)[stripe], _bits(up)[stripe])
        assert not np.array_equal(_bits(f)[~stripe], _bits(up)[~stripe])


@pytest.mark.parametrize("step,psz", ((4, 15), (5, 4), (8, 8)))
def test_a_zero_y_table_gives_plus_zero_in_v(step, psz):
    """d[..., 1] = +0.0 everywhere, as after compute_x: the v plane is +0.0 to the bit, in the votes and in the fallback."""
    a, b, d, lost = _pair_table(step, "smooth")
    d = d.copy()
    d[..., 1] = 0.0
    for got in _both(a, b, d, lost, step, psz, power=2):
        assert not _bits(got[..., 1]).any()
        assert got[..., 0].any()


def test_a_constant_table_comes_back():
    """A constant displacement on all nodes comes back wherever a vote exists: to the bit from the definition (an f64
    quotient rounded once), "within 2 ulp" from the f32 form, as the rule states it. The f32 form takes the mean about the
    first vote, d0 + sum(wgt (d - d0)) / sum(wgt), and returns the constant's bits too. (The plain f32 form,
    sum(wgt d) / sum(wgt), measured 2, 5, 10 and 18 ulp at the four geometries, 4, 16, 36 and 64 votes per pixel.)"""
    worst = _constant_ulps(DC.CONST_GEOMS)
    assert worst == DC.CONST_ULP, ("the record is not the measured figure", worst, DC.CONST_ULP)
    assert worst["definition"] == 0
    assert worst["restatement"] <= 2, worst


def _constant_ulps(geoms):
    """{form: worst distance in ulps from the constant, over the pixels that took a vote}; each geometry printed."""
    a, b = FC.pair(FRAME)
    total = {"definition": 0, "restatement": 0}
    for step, psz in geoms:
        _, lost = DC.nodes(FRAME, step, "smooth")
        worst = {"definition": 0, "restatement": 0}
        for c in DC.CONSTANTS:
            dc = np.empty(lost.shape + (2,), np.float32)
            dc[...] = np.float32(c)
            for power in DC.POWERS:
                st = {}
                pf.densify_flow_host(a, b, dc, lost, step, psz, power=power, _stages=st)
                voted = st["count"] > 0
                assert voted.any()
                for name, got in zip(("definition", "restatement"), _both(a, b, dc, lost, step, psz, power=power)):
                    ulps = np.abs(_bits(got).astype(np.int64) - _bits(dc[0, 0]).astype(np.int64))[voted]
                    worst[name] = max(worst[name], int(ulps.max()))
        print(f"constant table, step {step} psz {psz}: worst distance in ulps", worst)
        total = {k: max(total[k], v) for k, v in worst.items()}
    return total


def test_a_nan_node_does_not_vote():
    """A position that is not a number is not inside: the node's vote is dropped, its neighbours' stand."""
    step, psz = 4, 15
    a, b, d, lost = _pair_table(step)
    dn = d.copy()
    dn[5, 7] = np.nan
    sd, sn = {}, {}
    pf.densify_flow_host(a, b, d, lost, step, psz, _stages=sd)
    got = pf.densify_flow_host(a, b, dn, lost, step, psz, _stages=sn)
    assert np.isfinite(got).all()
    fewer = sd["count"] - sn["count"]
    assert set(np.unique(fewer)) == {0, 1} and fewer.sum() > 100
    rs = {}
    res = R.densify(a, b, dn, lost, step, psz, stages=rs)
    assert np.isfinite(res).all() and np.array_equal(rs["count"], sn["count"])


def test_host_refuses():
    a, b, d, lost = _pair_table(4)
    for bad in (dict(psz=0), dict(psz=33), dict(power=0), dict(power=5), dict(power=1.5), dict(minerr=0.0),
                dict(minerr=-1.0), dict(minerr=float("nan")), dict(minerr=float("inf")), dict(step=0), dict(step=5)):
        kw = dict(step=4, psz=15, minerr=2.0, power=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            pf.densify_flow_host(a, b, d, lost, **kw)
    with pytest.raises(ValueError):
        pf.densify_flow_host(a, b[:-1], d, lost, 4, 15)
    with pytest.raises(ValueError):
        pf.densify_flow_host(a, b, d[:-1], lost, 4, 15)
    with pytest.raises(ValueError):
        pf.densify_flow_host(a, b, d, lost[:, :-1], 4, 15)


# ---------------------------------------------------------------- usefulness, on the definition alone
@pytest.mark.parametrize("kind,power", sorted(DC.USEFUL))
def test_host_usefulness(kind, power):
    worst = 0.0
    for seed in FC.SEEDS:
        a, b, d, lost, f, truth, mask = DC.useful_inputs(kind, seed)
        h, w = a.shape
        assert np.array_equal(_bits(pf._dense_from_nodes(d.copy(), lost, w, h, DC.USEFUL_STEP)), _bits(f))
        out = pf.densify_flow_host(a, b, d, lost, DC.USEFUL_STEP, DC.USEFUL_PSZ, power=power)
        before, after = FC.epe(f, truth, mask), FC.epe(out, truth, mask)
        print(f"{kind} power {power} seed {seed}: {before:.4f} -> {after:.4f} px ({after / before:.3f}), "
              f"bar {DC.useful_bar(kind, power):.3f}")
        assert after <= DC.useful_bar(kind, power) * before
        worst = max(worst, after / before)
    ratio = DC.USEFUL[kind, power]
    assert ratio - 0.01 <= worst <= ratio, ("the recorded ratio is not the measured one", worst, ratio)


def test_host_densified_then_refined_is_recorded():
    """Densified (power 1) + refined against refined alone on "layers": recorded in densify_cases.REFINED, no bar."""
    got = {}
    for seed in FC.SEEDS:
        a, b, d, lost, f, truth, mask = DC.useful_inputs("layers", seed)
        z = pf.densify_flow_host(a, b, d, lost, DC.USEFUL_STEP, DC.USEFUL_PSZ)
        got[seed] = (FC.epe(pf.refine_flow_host(a, b, f), truth, mask), FC.epe(pf.refine_flow_host(a, b, z), truth, mask))
        print(f"layers seed {seed}: refined alone {got[seed][0]:.4f} px, densified + refined {got[seed][1]:.4f} px")
    for seed, rec in DC.REFINED.items():
        assert max(abs(got[seed][0] - rec[0]), abs(got[seed][1] - rec[1])) < 5e-4, ("the record is not the measured figure",
                                                                                   seed, got[seed], rec)
    assert set(DC.REFINED) == set(FC.SEEDS)
