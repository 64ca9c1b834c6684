"""The 1-D stereo search against the 2-D tracker on the same pyramids and nodes -> profiles/patchdisp_bench.json.

  python tools/patchdisp_bench.py [--reps 7] [--out profiles/patchdisp_bench.json] [--parent parent_run.json]

Per shape (1242x375 and 1920x1080, step 4, psz 15, lv_f 3, the defaults maxiter 10 and eps 0.01): the HIP-event time of
the k_patchdisp launch (track_disparity) and of the k_patchflow launch (track_points) on the nodes of the step grid,
interleaved, `reps` runs each after a warm-up of both; and the wall time per stereo frame of
StereoPointTracker.push_frames with disparity "2d" and "1d" (4 frames pushed and the window counted, which waits for the
device, over 4), interleaved likewise. Minimum, median and maximum of each. The frames are seeded sums of gratings of all
directions; the right frame is the left one shifted by 6.3 px, a later frame is moved by (1.2, 0.4) px per frame.
The x error against the true -6.3 px is taken over all tracked nodes, and separately (signed median) over the nodes
with x or y >= 256 and over the others: both kernels take their first tap at floor(x) + 1, the pair their weights are
taken for at every x. (Before that rule the first tap was the reference's ceil(x + 1e-5f); at an integer coordinate of
256 or more that sum rounds back to x in float32, the template sat one pixel to the left or up, and both kernels
reported the shift less one pixel there.)
The bar: the median of the 1-D launch is not above the median of the 2-D launch of the same run (exit status 1 if it is).
--parent: the file another build's run of this tool wrote (its "shapes" are copied into the output as "parent_shapes");
then a second bar holds: each kernel's median is not above that run's median by more than that run's own max - min.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import invcompcamtrack_amd as ic  # noqa: E402
from invcompcamtrack_amd import patchflow as pf  # noqa: E402
from invcompcamtrack_amd import stereotrack as S  # noqa: E402

STEP, PSZ, LV_F, NFRAMES, DISP = 4, 15, 3, 4, 6.3


def frames(w, h, seed=5):
    """(left[k], right[k]) float32 for k < NFRAMES."""
    rng = np.random.default_rng(seed)
    n = 24
    th, lam = rng.uniform(0, np.pi, n), rng.uniform(6, 60, n)
    amp, ph = rng.uniform(2, 6, n), rng.uniform(0, 2 * np.pi, n)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)

    def img(dx, dy):
        out = np.full((h, w), 128.0, np.float32)
        for k in range(n):
            out += np.float32(amp[k]) * np.sin(np.float32(2 * np.pi / lam[k]) * (np.float32(np.cos(th[k])) * (x + np.float32(dx))
                                                                              + np.float32(np.sin(th[k])) * (y + np.float32(dy)))
                                               + np.float32(ph[k]))
        return out

    return [(img(1.2 * k, 0.4 * k), img(1.2 * k + DISP, 0.4 * k)) for k in range(NFRAMES)]


def stats(v):
    v = np.asarray(v, np.float64)
    return {"min": round(float(v.min()), 4), "median": round(float(np.median(v)), 4), "max": round(float(v.max()), 4)}


def kernel_times(pa, pb, pts, reps):
    calls = {"1d": (pf.track_disparity, pf.disparity_last_kernel_ms), "2d": (pf.track_points, pf.last_kernel_ms)}
    ms, res = {"1d": [], "2d": []}, {}
    for rep in range(reps + 1):  # the first round warms both up
        for name, (fn, last) in calls.items():
            res[name] = fn(pa, pb, pts, psz=PSZ, lv_f=LV_F)
            t = last()
            if t is None:
                raise RuntimeError("no kernel time: the HIP events failed")
            if rep:
                ms[name].append(t)
    return ms, res


def wall_times(w, h, fr, reps):
    ms = {"2d": [], "1d": []}
    kept = {}
    for rep in range(reps + 1):
        for mode in ms:
            t = S.StereoPointTracker(w, h, NFRAMES, STEP, PSZ, LV_F, disparity=mode)
            t0 = time.perf_counter()
            for left, right in fr:
                t.push_frames(left, right)
            kept[mode] = t.win.count()  # waits for the device
            if rep:
                ms[mode].append((time.perf_counter() - t0) * 1e3 / NFRAMES)
    return ms, kept


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patchdisp_bench.json"))
    ap.add_argument("--parent", default=None, help="the output of another build's run, to compare the kernel medians with")
    a = ap.parse_args()
    if a.reps < 7:
        ap.error("at least 7 runs each")
    if ic.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    out = {"bench": "patchdisp", "step": STEP, "psz": PSZ, "lv_f": LV_F, "maxiter": 10, "eps": 0.01, "reps": a.reps,
           "frames_per_window": NFRAMES, "true_disparity_px": -DISP, "shapes": []}
    ok = True
    parent = None
    if a.parent:
        with open(a.parent) as f:
            parent = {(r["w"], r["h"]): r for r in json.load(f)["shapes"]}
        out["parent_shapes"] = list(parent.values())
    for w, h in ((1242, 375), (1920, 1080)):
        fr = frames(w, h)
        pa, pb = ic.Pyramid(fr[0][0], LV_F, PSZ, True), ic.Pyramid(fr[0][1], LV_F, PSZ, True)
        gx, gy = np.meshgrid(np.arange(STEP // 2, w, STEP, dtype=np.float32), np.arange(STEP // 2, h, STEP, dtype=np.float32))
        pts = np.stack([gx.ravel(), gy.ravel()], 1)
        kms, res = kernel_times(pa, pb, pts, a.reps)
        wms, kept = wall_times(w, h, fr, a.reps)
        rec = {"w": w, "h": h, "nodes": len(pts), "form_1d": pf.disparity_last_form(), "form_2d": pf.last_form()}
        for name in ("1d", "2d"):
            new, st, it = res[name]
            e = (new[:, 0] - pts[:, 0] + DISP).astype(np.float64)
            far = st & ((pts[:, 0] >= 256) | (pts[:, 1] >= 256))  # (see the module docstring)
            near = st & ~far
            rec[f"kernel_ms_{name}"] = stats(kms[name])
            rec[f"tracked_{name}"] = int(st.sum())
            rec[f"mean_iters_{name}"] = round(float(it[st].mean()), 3)
            rec[f"median_abs_x_error_px_{name}"] = round(float(np.median(np.abs(e[st]))), 4)
            rec[f"median_x_error_px_from_256_{name}"] = round(float(np.median(e[far])), 4)
            rec[f"median_x_error_px_below_256_{name}"] = round(float(np.median(e[near])), 4)
            rec[f"push_frames_wall_ms_per_stereo_frame_{name}"] = stats(wms[name])
            rec[f"window_survivors_{name}"] = int(kept[name])
        rec["kernel_median_ratio_1d_over_2d"] = round(rec["kernel_ms_1d"]["median"] / rec["kernel_ms_2d"]["median"], 4)
        rec["push_frames_wall_ms_difference_2d_minus_1d"] = round(
            rec["push_frames_wall_ms_per_stereo_frame_2d"]["median"] - rec["push_frames_wall_ms_per_stereo_frame_1d"]["median"], 4)
        rec["bar_1d_median_not_above_2d_median"] = rec["kernel_ms_1d"]["median"] <= rec["kernel_ms_2d"]["median"]
        ok &= rec["bar_1d_median_not_above_2d_median"]
        if parent:
            for name in ("1d", "2d"):
                p = parent[w, h][f"kernel_ms_{name}"]
                rec[f"bar_{name}_median_within_parent_spread"] = bool(
                    rec[f"kernel_ms_{name}"]["median"] <= p["median"] + (p["max"] - p["min"]))
                ok &= rec[f"bar_{name}_median_within_parent_spread"]
        out["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
