"""The variational refinement at frame sizes a user runs -> profiles/flowrefine_bench.json.

  python tools/flowrefine_bench.py [--reps 7] [--out profiles/flowrefine_bench.json] [--parent-root DIR]

Per shape (1242x375 and 1920x1080), with the default parameters (alpha 16, gamma 13, delta 4.5, 8 outer iterations, 5 SOR
sweeps, omega 1.6) and a FlowGrid (step 4, psz 15, lv_f 3) of the pair as the source, `reps` runs after a warm-up, HIP
events throughout, minimum / median / maximum of each:
  - the refiner's own events: k_fr_warp, k_fr_coef, k_fr_sor summed over the outer iterations, k_fr_init + k_fr_final,
    and their sum (the marks are consecutive records on the stream, so the sum is the run less the grid's dense field);
  - the launch count;
  - the algorithmic bytes of one half-sweep and of the coefficient kernel (each plane element that must be read or written
    counted once, BYTES_* below), the rate they give over the measured time, and next to it the rate of a plain
    device-to-device copy that moves the same number of bytes (half read, half written), timed in the same run;
  - FlowGrid.compute + FlowGrid.dense (on the device) of the same pair, and the refinement's ratio to it;
  - the wall time per stereo frame of StereoPointTracker.push_frames (4 frames pushed and the window counted, which waits
    for the device) with refine=None and with refine={}.
--parent-root: a built checkout of the parent commit. push_frames with refine=None is then measured in child processes of
this tree and of that one in turn (two each, `reps` windows per child after a warm-up). The one bar (exit status 1): this
tree's median is not above the parent's median by more than the parent's own max - min.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP, PSZ, LV_F, NFRAMES = 4, 15, 3, 4
SHAPES = ((1242, 375), (1920, 1080))
# f32 plane elements per pixel that one launch must move, each counted once:
#   half-sweep  reads a11 a12 a22 b1 b2 at its colour (5/2), u v du dv whole (the pixel and its four neighbours: 4), the
#               two edge-weight planes whole (2); writes du dv at its colour (1)
#   coef        reads Bw A u v (4); writes a11 a12 a22 b1 b2 wr wd du dv (9)
BYTES_HALF_SWEEP, BYTES_COEF = 4 * 9.5, 4 * 13.0


def push_child(root, reps):
    """Runs in a child process: wall ms per stereo frame of push_frames with the default (refine=None) path."""
    sys.path.insert(0, root)
    from invcompcamtrack_amd import stereotrack as S
    from tools.patchdisp_bench import frames
    out = {}
    for w, h in SHAPES:
        fr = frames(w, h)
        ms = []
        for rep in range(reps + 1):
            t = S.StereoPointTracker(w, h, NFRAMES, STEP, PSZ, LV_F)
            t0 = time.perf_counter()
            for left, right in fr:
                t.push_frames(left, right)
            t.win.count()  # waits for the device
            if rep:
                ms.append((time.perf_counter() - t0) * 1e3 / NFRAMES)
        out[f"{w}x{h}"] = ms
    print("PUSH " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flowrefine_bench.json"))
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--push-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.push_child:
        return push_child(a.push_child, a.reps)
    if a.reps < 7:
        ap.error("at least 7 runs each")
    sys.path.insert(0, ROOT)
    import torch

    import invcompcamtrack_amd as ic
    from invcompcamtrack_amd import patchflow as pf
    from invcompcamtrack_amd import stereotrack as S
    from tools.patchdisp_bench import frames, stats
    if ic.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    p = pf.REFINE_DEFAULTS
    out = {"bench": "flowrefine", "params": p, "step": STEP, "psz": PSZ, "lv_f": LV_F, "reps": a.reps,
           "launches_per_run": 2 + p["n_outer"] * (2 + 2 * p["n_sor"]),
           "bytes_per_pixel": {"half_sweep": BYTES_HALF_SWEEP, "coef": BYTES_COEF}, "shapes": []}
    ok = True
    for w, h in SHAPES:
        fr = frames(w, h)
        n = w * h
        pa, pb = ic.Pyramid(fr[0][0], LV_F, PSZ, True), ic.Pyramid(fr[1][0], LV_F, PSZ, True)
        grid = pf.FlowGrid(w, h, STEP)
        ref = pf.FlowRefiner(w, h)
        ref.set_timing(True)
        dense = torch.empty((h, w, 2), dtype=torch.float32, device="cuda")
        sweeps = 2 * p["n_sor"] * p["n_outer"]
        copies = {}
        for name, bpp in (("half_sweep", BYTES_HALF_SWEEP), ("coef", BYTES_COEF)):
            k = int(bpp * n / 2) // 4  # floats copied: as many bytes read as written, bpp * n in all
            copies[name] = (torch.zeros(k, dtype=torch.float32, device="cuda"),
                            torch.empty(k, dtype=torch.float32, device="cuda"))
        ms = {k: [] for k in ("warp", "coef", "sor", "init_final", "run", "grid", "copy_half_sweep", "copy_coef")}
        for rep in range(a.reps + 1):  # the first round warms everything up
            tg = timed(lambda: (grid.compute(pa, pb, psz=PSZ, lv_f=LV_F), grid.dense(out=dense.data_ptr(), on_device=True)))
            ref.run(pa, pb, grid)
            k = ref.kernel_ms()
            tc = {name: timed(lambda: dst.copy_(src)) for name, (src, dst) in copies.items()}
            if rep:
                for key, v in zip(("warp", "coef", "sor", "init_final"), k):
                    ms[key].append(float(v))
                ms["run"].append(float(k.sum()))
                ms["grid"].append(tg)
                for name in copies:
                    ms["copy_" + name].append(tc[name])
        moved = ref.dense() - grid.dense()
        rec = {"w": w, "h": h, "mean_abs_change_px": round(float(np.abs(moved).mean()), 4)}
        for key, v in ms.items():
            rec[key + "_ms"] = stats(v)
        gb = lambda bpp, count, t: round(bpp * n * count / (t * 1e-3) / 1e9, 1)
        rec["sor_GBps"] = gb(BYTES_HALF_SWEEP, sweeps, rec["sor_ms"]["median"])
        rec["copy_half_sweep_GBps"] = gb(BYTES_HALF_SWEEP, 1, rec["copy_half_sweep_ms"]["median"])
        rec["half_sweep_us"] = round(rec["sor_ms"]["median"] * 1e3 / sweeps, 2)
        rec["coef_GBps"] = gb(BYTES_COEF, p["n_outer"], rec["coef_ms"]["median"])
        rec["copy_coef_GBps"] = gb(BYTES_COEF, 1, rec["copy_coef_ms"]["median"])
        rec["run_over_grid_compute_and_dense"] = round(rec["run_ms"]["median"] / rec["grid_ms"]["median"], 2)
        wall = {"none": [], "refine": []}
        kept = {}
        for rep in range(a.reps + 1):
            for name, refine in (("none", None), ("refine", {})):
                t = S.StereoPointTracker(w, h, NFRAMES, STEP, PSZ, LV_F, refine=refine)
                t0 = time.perf_counter()
                for left, right in fr:
                    t.push_frames(left, right)
                kept[name] = t.win.count()
                if rep:
                    wall[name].append((time.perf_counter() - t0) * 1e3 / NFRAMES)
        for name in wall:
            rec[f"push_frames_wall_ms_per_stereo_frame_{name}"] = stats(wall[name])
            rec[f"window_survivors_{name}"] = int(kept[name])
        out["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
    if a.parent_root:
        runs = {"this": {}, "parent": {}}
        for _ in range(2):
            for side, root in (("parent", os.path.abspath(a.parent_root)), ("this", ROOT)):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--push-child", root, "--reps", str(a.reps)],
                                   capture_output=True, text=True, timeout=600, cwd=root)
                if r.returncode != 0:
                    raise SystemExit(f"the {side} child failed:\n{r.stdout}\n{r.stderr}")
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("PUSH ")][-1]
                for key, v in json.loads(line[5:]).items():
                    runs[side].setdefault(key, []).extend(v)
        out["push_frames_default_path"] = {}
        for key in runs["this"]:
            t, q = stats(runs["this"][key]), stats(runs["parent"][key])
            bar = bool(t["median"] <= q["median"] + (q["max"] - q["min"]))
            out["push_frames_default_path"][key] = {"this_tree_ms": t, "parent_ms": q, "bar_median_within_parent_spread": bar}
            ok &= bar
        print(json.dumps(out["push_frames_default_path"]), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
