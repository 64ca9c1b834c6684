"""The densification of a flow grid at frame sizes a user runs -> profiles/densify_bench.json.

  python tools/densify_bench.py [--reps 7] [--out profiles/densify_bench.json] [--parent-root DIR]

Per shape (1242x375 and 1920x1080) and patch size (15 and 8) at step 4, with the default parameters (minerr 2, power 1) and
a FlowGrid (lv_f 3) of the pair, `reps` runs after a warm-up, HIP events throughout, minimum / median / maximum of each:
  - k_densify (the object's own events around its one launch);
  - FlowGrid.dense (k_fg_dense into device memory) and FlowGrid.compute of the same pair;
  - one default FlowRefiner.run on the densifier's field (the refiner's own events, summed);
  - the algorithmic bytes of k_densify (A once, B once, the field written: 16 B per pixel), the rate they give over the
    measured time, and next to it the rate of a plain device-to-device copy that moves the same number of bytes (half read,
    half written), timed in the same run;
  - the votes and B taps (4 per vote) per pixel from the count plane, and the taps per second they give;
  - the wall time per stereo frame of StereoPointTracker.push_frames (4 frames pushed and the window counted, which waits
    for the device) with neither, with densify={} and with densify={}, refine={} (psz 15 only).
--parent-root: a built checkout of the parent commit. push_frames with densify=None, refine=None is then measured in child
processes of this tree and of that one in turn (two each, `reps` windows per child after a warm-up). The one bar (exit
status 1): this tree's median is not above the parent's median by more than the parent's own max - min.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP, LV_F, NFRAMES = 4, 3, 4
PSZS = (15, 8)
SHAPES = ((1242, 375), (1920, 1080))
BYTES_DENSIFY = 4 * 4.0  # f32 elements per pixel that the launch must move: A, B read once, (u, v) written


def push_child(root, reps):
    """Runs in a child process: wall ms per stereo frame of push_frames with the default path (nothing densified or
    refined); `root` may be a checkout without the densifier."""
    sys.path.insert(0, root)
    from invcompcamtrack_amd import stereotrack as S
    from tools.patchdisp_bench import frames
    out = {}
    for w, h in SHAPES:
        fr = frames(w, h)
        ms = []
        for rep in range(reps + 1):
            t = S.StereoPointTracker(w, h, NFRAMES, STEP, PSZS[0], LV_F)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "densify_bench.json"))
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

    out = {"bench": "densify", "params": pf.DENSIFY_DEFAULTS, "step": STEP, "lv_f": LV_F, "reps": a.reps,
           "bytes_per_pixel": BYTES_DENSIFY, "shapes": []}
    ok = True
    for w, h in SHAPES:
        fr = frames(w, h)
        n = w * h
        for psz in PSZS:
            pa, pb = ic.Pyramid(fr[0][0], LV_F, psz, True), ic.Pyramid(fr[1][0], LV_F, psz, True)
            grid = pf.FlowGrid(w, h, STEP)
            dz = pf.FlowDensifier(w, h)
            dz.set_timing(True)
            ref = pf.FlowRefiner(w, h)
            ref.set_timing(True)
            dense = torch.empty((h, w, 2), dtype=torch.float32, device="cuda")
            k = int(BYTES_DENSIFY * n / 2) // 4  # floats copied: as many bytes read as written
            src, dst = torch.zeros(k, dtype=torch.float32, device="cuda"), torch.empty(k, dtype=torch.float32, device="cuda")
            ms = {key: [] for key in ("densify", "grid_dense", "grid_compute", "refine_run", "copy")}
            for rep in range(a.reps + 1):  # the first round warms everything up
                tc = timed(lambda: grid.compute(pa, pb, psz=psz, lv_f=LV_F))
                td = timed(lambda: grid.dense(out=dense.data_ptr(), on_device=True))
                dz.run(grid, pa, pb, psz)
                tz = dz.kernel_ms()
                tr = float(ref.run(pa, pb, dz).kernel_ms().sum())
                tcopy = timed(lambda: dst.copy_(src))
                if rep:
                    for key, v in zip(("densify", "grid_dense", "grid_compute", "refine_run", "copy"), (tz, td, tc, tr, tcopy)):
                        ms[key].append(float(v))
            votes = float(dz.stage("count").mean())
            rec = {"w": w, "h": h, "psz": psz, "votes_per_pixel": round(votes, 2), "taps_per_pixel": round(4 * votes, 1),
                   "lost_nodes": round(float(grid.nodes()[1].mean()), 4),
                   "mean_abs_change_px": round(float(np.abs(dz.dense() - grid.dense()).mean()), 4)}
            for key, v in ms.items():
                rec[key + "_ms"] = stats(v)
            t = rec["densify_ms"]["median"] * 1e-3
            rec["densify_GBps"] = round(BYTES_DENSIFY * n / t / 1e9, 1)
            rec["copy_GBps"] = round(BYTES_DENSIFY * n / (rec["copy_ms"]["median"] * 1e-3) / 1e9, 1)
            rec["densify_Gtaps_per_s"] = round(4 * votes * n / t / 1e9, 1)
            rec["densify_over_grid_dense"] = round(rec["densify_ms"]["median"] / rec["grid_dense_ms"]["median"], 2)
            rec["densify_over_refine_run"] = round(rec["densify_ms"]["median"] / rec["refine_run_ms"]["median"], 4)
            if psz == PSZS[0]:
                modes = (("none", {}), ("densify", dict(densify={})), ("densify_refine", dict(densify={}, refine={})))
                wall, kept = {name: [] for name, _ in modes}, {}
                for rep in range(a.reps + 1):
                    for name, kw in modes:
                        tk = S.StereoPointTracker(w, h, NFRAMES, STEP, psz, LV_F, **kw)
                        t0 = time.perf_counter()
                        for left, right in fr:
                            tk.push_frames(left, right)
                        kept[name] = tk.win.count()
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
