"""The per-iteration judge of tests/iter_judge.py, checked on the CPU before the device is held to it
(tests/test_gpu_iter_sums.py).

Identity: on np_oracle.track's own trace (float64 sums rounded to f32) the judge finds b and H within 0.5 units: the
  f32 rounding of the float64 sum, nothing else.
Yardstick: on the C oracle's trace, judged at the oracle's own poses with the oracle's exp map. With float64 sums
  (orc_set_sum_mode(1)) within 0.5 units; with the f32 Eigen-order sums the worst units are printed: the bars of the GPU
  cases are made of them (iter_judge.bars). As measured with this file (maxiter 6, ratio 0), worst b / H:
      psz8    f32 1.03 / 2.18   f64 0.43 / 0.36        vga     f32 1.05 / 1.70   f64 0.31 / 0.47
      psz4    f32 0.55 / 1.15   f64 0.34 / 0.40        8200    f32 13.3 / 32.7   f64 0.26 / 0.45
      border  f32 1.09 / 1.53   f64 0.36 / 0.39
Sensitivity, of the judge alone: a b_ref that leaves one patch of the new view out from the second iteration of a level
  on, or that takes one iteration's mask and taps at the previous iteration's pose, puts at least one record of every
  scene beyond that scene's bar.
Visibility: the `border` scene (margin -6: points up to 6 px outside the frame) changes its count of points in the new
  view between records, so the case built on it exercises the mask.
"""
import functools

import numpy as np
import pytest

import iter_judge as J
from oracle import np_oracle as N

NAMES = list(J.SCENES)


def _scene(name):
    w, h, n, psz, lv_f, seed, margin = J.SCENES[name]
    return J.make_scene(w, h, n, seed, margin), psz, lv_f


@functools.lru_cache(maxsize=None)
def _run(name, sum_mode):
    from oracle import oracle as O
    O.build()
    sc, psz, lv_f = _scene(name)
    return O, J.oracle_run(O, sc, lv_f, 0, psz, J.MAXITER, sum_mode=sum_mode), psz


@functools.lru_cache(maxsize=None)
def _f32_figures(name):
    O, run, psz = _run(name, 0)
    res = J.judge_oracle_run(O, run, psz)
    b, H, zeros = J.worst(res)
    assert zeros
    return b, H, res


@pytest.mark.parametrize("name", ["psz8", "psz4", "border"])
def test_identity_on_the_numpy_restatements_own_trace(oracle, name):
    sc, psz, lv_f = _scene(name)
    run = J.oracle_run(oracle, sc, lv_f, 0, psz, 1)  # (for the pyramids and the camera)
    p, trace = N.track(sc["pts3d"], sc["p_a"], run["pyr_ref"], run["pyr_new"], run["cam"], lv_f, 0, psz, J.MAXITER,
                       oracle.solve6, exp=oracle.se3_exp)
    res = J.judge(trace, sc["pts3d"], np.asarray(sc["p_a"], np.float32), run["pyr_ref"], run["pyr_new"], run["cam"], psz,
                  oracle.se3_exp, oracle.se3_exp)
    b, H, zeros = J.worst(res)
    print(f"[{name}] identity: worst b {b:.3f} H {H:.3f} units")
    assert len(res) == (lv_f + 1) * J.MAXITER and zeros
    assert b <= 0.5 and H <= 0.5, J.report(res)
    assert [r["n_new"] for r in res] == [int(t["vis_new"].sum()) for t in trace]


@pytest.mark.parametrize("name", NAMES)
def test_yardstick_c_oracle_at_its_own_poses(oracle, name):
    O, run, psz = _run(name, 1)
    res = J.judge_oracle_run(O, run, psz)
    b64, H64, zeros = J.worst(res)
    b32, H32, _ = _f32_figures(name)
    print(f"[{name}] C oracle at its own poses: f32 Eigen-order sums worst b {b32:.2f} H {H32:.2f} units "
          f"(bars {J.bars(b32, H32)}); float64 sums worst b {b64:.2f} H {H64:.2f}")
    assert len(res) == (J.SCENES[name][4] + 1) * J.MAXITER and zeros
    assert b64 <= 0.5 and H64 <= 0.5, J.report(res)


@pytest.mark.parametrize("fault", [("drop_patch",), ("stale_G", 2)])
@pytest.mark.parametrize("name", NAMES)
def test_judge_sees_a_lost_patch_and_a_stale_pose(oracle, name, fault):
    """The faulted b_ref against the C oracle's (correct) b: what a kernel with that fault would show."""
    O, run, psz = _run(name, 0)
    b32, H32, clean = _f32_figures(name)
    bar_b, _ = J.bars(b32, H32)
    res = J.judge_oracle_run(O, run, psz, fault=fault)
    hit = [(r["level"], r["iter"], round(r["b_units"])) for r in res if not r["b_units"] <= bar_b]
    print(f"[{name}] {fault}: bar {bar_b:.2f}, records beyond it {hit}")
    assert hit, J.report(res)
    faulted = (lambda it: it >= 1) if fault[0] == "drop_patch" else (lambda it: it == fault[1])
    for r, c in zip(res, clean):  # ... and no other record moves
        if not faulted(r["iter"]):
            assert r["b_units"] == c["b_units"]
    if fault[0] == "drop_patch":  # every faulted record is caught, not just one
        assert len(hit) == sum(faulted(r["iter"]) for r in res)


def test_border_scene_changes_its_new_view_count_between_records(oracle):
    _, _, res = _f32_figures("border")
    counts = [r["n_new"] for r in res]
    print("points in the new view per record:", counts)
    assert len(set(counts)) > 1 and max(counts) < J.SCENES["border"][2]
