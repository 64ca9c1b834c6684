"""The coarse-to-fine dense flow at frame sizes a user runs -> profiles/c2fflow_bench.json.

  python tools/c2fflow_bench.py [--reps 7] [--out profiles/c2fflow_bench.json] [--parent-root DIR]

Per shape (1242x375 and 1920x1080) and patch size (8 and 15) at step 4, lv_f 3, with the default parameters and no
refinement, `reps` runs after a warm-up, HIP events throughout, minimum / median / maximum of each:
  - per level the search (k_c2f_level and the grid's fill) and the densification (the object's own events), and the
    whole run (events around CoarseToFineFlow.run);
  - in the same run FlowGrid.compute + FlowDensifier.run of the same pair (what the stage is an alternative to), and a
    device-to-device copy of 16 B per pixel (half read, half written).
These are recorded without a bar: the stage does more work per pair than the grid path, by construction.
--parent-root: a built checkout of the parent commit. The untouched default paths, FlowGrid.compute (HIP events) and
StereoPointTracker.push_frames with flow="grid" (wall time per stereo frame, 4 frames and the window counted), are then
measured in child processes of this tree and of that one in turn (two each, `reps` runs per child after a warm-up). The one
bar (exit status 1): this tree's median is not above the parent's own maximum; whether it is below the parent's minimum is
recorded too.

  python tools/c2fflow_bench.py --patnorm [--reps 7] [--out profiles/c2fflow_patnorm_bench.json] [--parent-root DIR]

The cost of patch-mean normalisation instead: per shape and patch size two CoarseToFineFlow objects, patnorm off and on, run
in turn; per level the search and densification medians of each and their ratio, and the whole runs. Recorded without a bar.
--parent-root then measures the default paths this option must leave alone, CoarseToFineFlow.run with patnorm off (psz 8
and 15) and FlowDensifier.run (psz 15), in child processes of the two builds in turn (two each). The bar (exit status 1):
this tree's median exceeds the parent's by at most the parent's own max - min spread.

  python tools/c2fflow_bench.py --x-only [--reps 7] [--out profiles/c2fflow_xonly_bench.json] [--parent-root DIR]

The 1-D form against the 2-D one in the same way, on a stereo pair (the gratings move along x only): two objects per shape
and patch size, x_only off and on, run in turn. Recorded without a bar. --parent-root measures CoarseToFineFlow.run with
x_only and patnorm off (psz 8 and 15) and FlowGrid.compute_x (psz 15) on the same pair, with the same bar.

  python tools/c2fflow_bench.py --lv-l [--reps 7] [--out profiles/c2fflow_lvl_bench.json] [--parent-root DIR]

A finest level above 0: per shape and patch size three objects with lv_l 0, 1 and 2, run in turn; the whole runs of each,
their ratios to lv_l = 0, and k_flow_upsample's own time (the object's event) next to the 16 B per pixel copy of the same
round. Recorded without a bar. --parent-root measures CoarseToFineFlow.run at lv_l = 0 (psz 8 and 15), with the same bar.

  python tools/c2fflow_bench.py --colour [--reps 7] [--out profiles/c2fflow_rgb_bench.json] [--parent-root DIR]

Colour frames next to grey ones: per shape and patch size two objects, channels 1 and 3, run in turn (the colour frame's
channel 0 is the grey frame, the other two channels are textures of their own under the same motion); per level the search
and densification medians of each and their ratio, and the whole runs. Recorded without a bar. --parent-root measures the
default paths colour must leave alone, CoarseToFineFlow.run grey (psz 8 and 15) and FlowDensifier.run (psz 15), with the
same bar.

  python tools/c2fflow_bench.py --fold --parent-root DIR [--reps 7] [--out profiles/c2fflow_fold_bench.json]

Nothing but the comparison with the parent, for a change that must leave every path as fast as it was: CoarseToFineFlow.run
grey (psz 8 and 15), FlowDensifier.run (psz 15), FlowRefiner.run at its defaults on the densifier's field, and
CoarseToFineFlow(channels=3).run with patnorm and the refinement on (psz 8 and 15), in child processes of the two builds in
turn (two each), with the same bar.

  python tools/c2fflow_bench.py --cost [--reps 7] [--out profiles/c2fflow_cost_bench.json] [--parent-root DIR]

The Huber patch cost next to L2: per shape and patch size, with patnorm off and on, two objects, cost "l2" and "huber"
(huber_k 5), run in turn; per level the search medians of each with the Huber / L2 ratio of every round (minimum / median /
maximum), and the whole runs likewise. Recorded without a bar. --parent-root measures the paths the cost must leave alone:
CoarseToFineFlow.run at L2 (psz 8 and 15, patnorm off and on) and FlowGrid.compute and compute_x (psz 15), whose kernels
include the changed header, with the same bar.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP, LV_F, NFRAMES = 4, 3, 4
PSZS = (8, 15)
SHAPES = ((1242, 375), (1920, 1080))
BYTES_COPY = 4 * 4.0  # bytes per pixel of the copy that the totals are set against


def _timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def default_child(root, reps):
    """Runs in a child process: the default paths of the tree at `root`, which may be a checkout without the stage."""
    sys.path.insert(0, root)
    import torch

    import invcompcamtrack_amd as ic
    from invcompcamtrack_amd import patchflow as pf
    from invcompcamtrack_amd import stereotrack as S
    from tools.patchdisp_bench import frames
    out = {}
    for w, h in SHAPES:
        fr = frames(w, h)
        psz = PSZS[1]
        pa, pb = ic.Pyramid(fr[0][0], LV_F, psz, True), ic.Pyramid(fr[1][0], LV_F, psz, True)
        grid = pf.FlowGrid(w, h, STEP)
        compute, push = [], []
        for rep in range(reps + 1):
            tc = _timed(torch, lambda: grid.compute(pa, pb, psz=psz, lv_f=LV_F))
            t = S.StereoPointTracker(w, h, NFRAMES, STEP, psz, LV_F)
            t0 = time.perf_counter()
            for left, right in fr:
                t.push_frames(left, right)
            t.win.count()  # waits for the device
            if rep:
                compute.append(float(tc))
                push.append((time.perf_counter() - t0) * 1e3 / NFRAMES)
        out[f"{w}x{h}"] = {"flowgrid_compute_ms": compute, "push_frames_wall_ms_per_stereo_frame": push}
    print("DEFAULT " + json.dumps(out), flush=True)


def option_child(root, reps, option):
    """Runs in a child process: CoarseToFineFlow.run (no keyword of the option: the parent has none) and, for "cost", the
    same with patnorm on and FlowGrid.compute and compute_x, for "patnorm",
    FlowDensifier.run, for "x_only" FlowGrid.compute_x on the stereo pair (for "lv_l" nothing more), for "fold"
    FlowDensifier.run, FlowRefiner.run and the colour run with patnorm and the refinement (the parent has them), of the
    tree at `root`, HIP events around each."""
    sys.path.insert(0, root)
    import torch

    import invcompcamtrack_amd as ic
    from invcompcamtrack_amd import patchflow as pf
    from tools.patchdisp_bench import frames
    out = {}
    for w, h in SHAPES:
        fr = frames(w, h)
        rec = {}
        for psz in PSZS:
            second = fr[0][1] if option == "x_only" else fr[1][0]
            pa, pb = ic.Pyramid(fr[0][0], LV_F, psz, True), ic.Pyramid(second, LV_F, psz, True)
            c = pf.CoarseToFineFlow(w, h, LV_F, STEP, psz)
            rec[f"c2f_run_psz{psz}_ms"] = [float(_timed(torch, lambda: c.run(pa, pb))) for _ in range(reps + 1)][1:]
            if option == "cost":
                cp = pf.CoarseToFineFlow(w, h, LV_F, STEP, psz, patnorm=True)
                rec[f"c2f_patnorm_run_psz{psz}_ms"] = [float(_timed(torch, lambda: cp.run(pa, pb)))
                                                       for _ in range(reps + 1)][1:]
                if psz == PSZS[1]:
                    grid = pf.FlowGrid(w, h, STEP)
                    rec["flowgrid_compute_ms"] = [float(_timed(torch, lambda: grid.compute(pa, pb, psz=psz, lv_f=LV_F)))
                                                  for _ in range(reps + 1)][1:]
                    rec["flowgrid_compute_x_ms"] = [float(_timed(torch, lambda: grid.compute_x(pa, pb, psz=psz, lv_f=LV_F)))
                                                    for _ in range(reps + 1)][1:]
            elif psz == PSZS[1] and option == "x_only":
                grid = pf.FlowGrid(w, h, STEP)
                rec["flowgrid_compute_x_ms"] = [float(_timed(torch, lambda: grid.compute_x(pa, pb, psz=psz, lv_f=LV_F)))
                                                for _ in range(reps + 1)][1:]
            elif psz == PSZS[1] and option in ("patnorm", "colour", "fold"):
                grid, dz = pf.FlowGrid(w, h, STEP), pf.FlowDensifier(w, h)
                grid.compute(pa, pb, psz=psz, lv_f=LV_F)
                rec["flowdensifier_run_ms"] = [float(_timed(torch, lambda: dz.run(grid, pa, pb, psz)))
                                               for _ in range(reps + 1)][1:]
                if option == "fold":
                    rf = pf.FlowRefiner(w, h)
                    rec["flowrefiner_run_ms"] = [float(_timed(torch, lambda: rf.run(pa, pb, dz)))
                                                 for _ in range(reps + 1)][1:]
            if option == "fold":  # channel 0 is the grey run's frame; the other two have textures of their own
                tri = [[ic.Pyramid(f[k][0], LV_F, psz, True) for f in (fr, frames(w, h, seed=6), frames(w, h, seed=7))]
                       for k in (0, 1)]
                c3 = pf.CoarseToFineFlow(w, h, LV_F, STEP, psz, channels=3, patnorm=True, refine={})
                rec[f"c2f_colour_patnorm_refine_run_psz{psz}_ms"] = [float(_timed(torch, lambda: c3.run(*tri)))
                                                                     for _ in range(reps + 1)][1:]
        out[f"{w}x{h}"] = rec
    print("DEFAULT " + json.dumps(out), flush=True)


def _option_against_parent(a, option, out):
    """The default paths an option must leave alone, in child processes of the parent's build and of this one in turn (two
    each), into out["default_paths"]. True when every median of this tree exceeds the parent's by at most the parent's own
    max - min spread."""
    from tools.patchdisp_bench import stats
    ok = True
    runs = {"this": {}, "parent": {}}
    for _ in range(2):
        for side, root in (("parent", os.path.abspath(a.parent_root)), ("this", ROOT)):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--option-child", root, "--option", option,
                                "--reps", str(a.reps)],
                               capture_output=True, text=True, timeout=600, cwd=root)
            if r.returncode != 0:
                raise SystemExit(f"the {side} child failed:\n{r.stdout}\n{r.stderr}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("DEFAULT ")][-1]
            for shape, d in json.loads(line[8:]).items():
                for key, v in d.items():
                    runs[side].setdefault((shape, key), []).extend(v)
    out["default_paths"] = {}
    for (shape, key), v in runs["this"].items():
        t, q = stats(v), stats(runs["parent"][shape, key])
        bar = bool(t["median"] <= q["median"] + (q["max"] - q["min"]))
        out["default_paths"].setdefault(shape, {})[key] = {
            "this_tree": t, "parent": q, "bar_median_within_parent_median_plus_spread": bar}
        ok &= bar
    print(json.dumps(out["default_paths"]), flush=True)
    return ok


def fold_main(a):
    """--fold: the comparison with the parent alone."""
    sys.path.insert(0, ROOT)
    if not a.parent_root:
        raise SystemExit("--fold compares with --parent-root")
    out = {"bench": "c2fflow_fold", "step": STEP, "lv_f": LV_F, "reps": a.reps}
    ok = _option_against_parent(a, "fold", out)
    with open(a.out or os.path.join(ROOT, "profiles", "c2fflow_fold_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


def lvl_main(a):
    """--lv-l: objects with lv_l 0, 1, 2 in turn, the up-sampling kernel against the copy, then lv_l = 0 against the
    parent's."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import invcompcamtrack_amd as ic
    from invcompcamtrack_amd import patchflow as pf
    from tools.patchdisp_bench import frames, stats
    if ic.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    lv_ls = (0, 1, 2)
    out = {"bench": "c2fflow_lvl", "step": STEP, "lv_f": LV_F, "lv_l": list(lv_ls), "reps": a.reps,
           "densify": pf.DENSIFY_DEFAULTS, "refine": None, "copy_bytes_per_pixel": BYTES_COPY,
           "upsample_bytes_written_per_pixel": 8, "shapes": []}
    ok = True
    for w, h in SHAPES:
        fr = frames(w, h)
        n = w * h
        for psz in PSZS:
            pa, pb = ic.Pyramid(fr[0][0], LV_F, psz, True), ic.Pyramid(fr[1][0], LV_F, psz, True)
            cs = {k: pf.CoarseToFineFlow(w, h, LV_F, STEP, psz, lv_l=k) for k in lv_ls}
            nf = int(BYTES_COPY * n / 2) // 4  # floats copied: as many bytes read as written
            src, dst = torch.zeros(nf, dtype=torch.float32, device="cuda"), torch.empty(nf, dtype=torch.float32, device="cuda")
            total, up, copy = {k: [] for k in lv_ls}, {k: [] for k in lv_ls[1:]}, []
            for rep in range(a.reps + 1):  # the first round warms everything up
                for lv_l, c in cs.items():
                    c.set_timing(True)
                    tt = _timed(torch, lambda: c.run(pa, pb))
                    if rep:
                        total[lv_l].append(float(tt))
                        if lv_l:
                            up[lv_l].append(c.upsample_ms())
                tcopy = _timed(torch, lambda: dst.copy_(src))
                if rep:
                    copy.append(float(tcopy))
            rec = {"w": w, "h": h, "psz": psz, "total_ms": {str(k): stats(total[k]) for k in lv_ls},
                   "upsample_ms": {str(k): stats(up[k]) for k in lv_ls[1:]}, "copy_ms": stats(copy)}
            rec["total_over_lv_l_0"] = {str(k): round(rec["total_ms"][str(k)]["median"] / rec["total_ms"]["0"]["median"], 3)
                                        for k in lv_ls[1:]}
            rec["upsample_over_copy"] = {str(k): round(rec["upsample_ms"][str(k)]["median"] / rec["copy_ms"]["median"], 2)
                                         for k in lv_ls[1:]}
            rec["mean_abs_difference_to_lv_l_0_px"] = {
                str(k): round(float(np.abs(cs[k].dense() - cs[0].dense()).mean()), 4) for k in lv_ls[1:]}
            out["shapes"].append(rec)
            print(json.dumps(rec), flush=True)
    if a.parent_root:
        ok &= _option_against_parent(a, "lv_l", out)
    with open(a.out or os.path.join(ROOT, "profiles", "c2fflow_lvl_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


def cost_main(a):
    """--cost: L2 and Huber objects in turn, with patnorm off and on, then the L2 paths against the parent's."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import invcompcamtrack_amd as ic
    from invcompcamtrack_amd import patchflow as pf
    from tools.patchdisp_bench import frames, stats
    if ic.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    out = {"bench": "c2fflow_cost", "step": STEP, "lv_f": LV_F, "reps": a.reps, "huber_k": 5.0,
           "densify": pf.DENSIFY_DEFAULTS, "refine": None, "shapes": []}
    ratio = lambda hu, l2: {k: round(float(f(np.asarray(hu) / np.asarray(l2))), 3)
                            for k, f in (("min", np.min), ("median", np.median), ("max", np.max))}
    ok = True
    for w, h in SHAPES:
        fr = frames(w, h)
        for psz in PSZS:
            pa, pb = ic.Pyramid(fr[0][0], LV_F, psz, True), ic.Pyramid(fr[1][0], LV_F, psz, True)
            for patnorm in (False, True):
                cs = {cost: pf.CoarseToFineFlow(w, h, LV_F, STEP, psz, patnorm=patnorm, cost=cost) for cost in ("l2", "huber")}
                levels, total = {c: [] for c in cs}, {c: [] for c in cs}
                for rep in range(a.reps + 1):  # the first round warms everything up
                    for cost, c in cs.items():
                        c.set_timing(True)
                        tt = _timed(torch, lambda: c.run(pa, pb))
                        if rep:
                            levels[cost].append(c.kernel_ms())
                            total[cost].append(float(tt))
                lv = {c: np.stack(v) for c, v in levels.items()}  # [rep][level][search, densify, refine]
                rec = {"w": w, "h": h, "psz": psz, "patnorm": patnorm, "levels": [],
                       "total_ms": {c: stats(total[c]) for c in cs},
                       "total_huber_over_l2": ratio(total["huber"], total["l2"])}
                for l in range(LV_F, -1, -1):
                    lw, lh, nx, ny = cs["l2"].level_dims(l)
                    rec["levels"].append({"level": l, "w": lw, "h": lh, "nodes": nx * ny,
                                          "search_ms": {c: stats(lv[c][:, l, 0]) for c in cs},
                                          "search_huber_over_l2": ratio(lv["huber"][:, l, 0], lv["l2"][:, l, 0])})
                out["shapes"].append(rec)
                print(json.dumps(rec), flush=True)
    if a.parent_root:
        ok &= _option_against_parent(a, "cost", out)
    with open(a.out or os.path.join(ROOT, "profiles", "c2fflow_cost_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


def option_main(a, option):
    """--patnorm / --x-only: the option off and on in turn, then the default paths against the parent's."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import invcompcamtrack_amd as ic
    from invcompcamtrack_amd import patchflow as pf
    from tools.patchdisp_bench import frames, stats
    if ic.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    name = {"patnorm": "c2fflow_patnorm", "x_only": "c2fflow_xonly", "colour": "c2fflow_rgb"}[option]
    out = {"bench": name, "step": STEP, "lv_f": LV_F, "reps": a.reps, "densify": pf.DENSIFY_DEFAULTS,
           "refine": None, "shapes": []}
    ok = True
    for w, h in SHAPES:
        fr = frames(w, h)
        more = (frames(w, h, seed=6), frames(w, h, seed=7)) if option == "colour" else None
        for psz in PSZS:
            second = fr[0][1] if option == "x_only" else fr[1][0]
            pa, pb = ic.Pyramid(fr[0][0], LV_F, psz, True), ic.Pyramid(second, LV_F, psz, True)
            args = {False: (pa, pb), True: (pa, pb)}
            if option == "colour":  # channel 0 is the grey run's frame; the other two have textures of their own
                tri = [[ic.Pyramid(f[k][0], LV_F, psz, True) for f in (fr, more[0], more[1])] for k in (0, 1)]
                args[True] = (tri[0], tri[1])
                cs = {on: pf.CoarseToFineFlow(w, h, LV_F, STEP, psz, channels=3 if on else 1) for on in (False, True)}
            else:
                cs = {on: pf.CoarseToFineFlow(w, h, LV_F, STEP, psz, **{option: on}) for on in (False, True)}
            levels, total = {False: [], True: []}, {False: [], True: []}
            for rep in range(a.reps + 1):  # the first round warms everything up
                for on, c in cs.items():
                    c.set_timing(True)
                    tt = _timed(torch, lambda: c.run(*args[on]))
                    if rep:
                        levels[on].append(c.kernel_ms())
                        total[on].append(float(tt))
            lv = {on: np.stack(v) for on, v in levels.items()}  # [rep][level][search, densify, refine]
            rec = {"w": w, "h": h, "psz": psz, "levels": [],
                   "total_ms": {"off": stats(total[False]), "on": stats(total[True])}}
            for l in range(LV_F, -1, -1):
                lw, lh, nx, ny = cs[True].level_dims(l)
                e = {"level": l, "w": lw, "h": lh, "nodes": nx * ny}
                for k, name in enumerate(("search_ms", "densify_ms")):
                    off, on = stats(lv[False][:, l, k]), stats(lv[True][:, l, k])
                    e[name] = {"off": off, "on": on, "on_over_off": round(on["median"] / off["median"], 3)}
                rec["levels"].append(e)
            rec["total_on_over_off"] = round(rec["total_ms"]["on"]["median"] / rec["total_ms"]["off"]["median"], 3)
            out["shapes"].append(rec)
            print(json.dumps(rec), flush=True)
    if a.parent_root:
        ok &= _option_against_parent(a, option, out)
    with open(a.out or os.path.join(ROOT, "profiles", name + "_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="default: profiles/c2fflow_bench.json (c2fflow_patnorm_bench.json, c2fflow_xonly_bench.json, c2fflow_lvl_bench.json)")
    ap.add_argument("--patnorm", action="store_true", help="measure the cost of patch-mean normalisation instead")
    ap.add_argument("--x-only", action="store_true", help="measure the 1-D form against the 2-D one instead")
    ap.add_argument("--lv-l", dest="lv_l", action="store_true", help="measure a finest level above 0 instead")
    ap.add_argument("--colour", action="store_true", help="measure colour frames against grey ones instead")
    ap.add_argument("--option-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--fold", action="store_true", help="compare every flow path with the parent's instead")
    ap.add_argument("--cost", action="store_true", help="measure the Huber patch cost against L2 instead")
    ap.add_argument("--option", default="patnorm", choices=("patnorm", "x_only", "lv_l", "colour", "fold", "cost"),
                    help=argparse.SUPPRESS)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--default-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.default_child:
        return default_child(a.default_child, a.reps)
    if a.option_child:
        return option_child(a.option_child, a.reps, a.option)
    if a.reps < 7:
        ap.error("at least 7 runs each")
    if a.fold:
        return fold_main(a)
    if a.lv_l:
        return lvl_main(a)
    if a.cost:
        return cost_main(a)
    if a.patnorm or a.x_only or a.colour:
        return option_main(a, "x_only" if a.x_only else "colour" if a.colour else "patnorm")
    a.out = a.out or os.path.join(ROOT, "profiles", "c2fflow_bench.json")
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import invcompcamtrack_amd as ic
    from invcompcamtrack_amd import patchflow as pf
    from tools.patchdisp_bench import frames, stats
    if ic.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")

    out = {"bench": "c2fflow", "step": STEP, "lv_f": LV_F, "reps": a.reps, "densify": pf.DENSIFY_DEFAULTS, "refine": None,
           "copy_bytes_per_pixel": BYTES_COPY, "shapes": []}
    ok = True
    for w, h in SHAPES:
        fr = frames(w, h)
        n = w * h
        for psz in PSZS:
            pa, pb = ic.Pyramid(fr[0][0], LV_F, psz, True), ic.Pyramid(fr[1][0], LV_F, psz, True)
            c = pf.CoarseToFineFlow(w, h, LV_F, STEP, psz)
            c.set_timing(True)
            grid, dz = pf.FlowGrid(w, h, STEP), pf.FlowDensifier(w, h)
            k = int(BYTES_COPY * n / 2) // 4  # floats copied: as many bytes read as written
            src, dst = torch.zeros(k, dtype=torch.float32, device="cuda"), torch.empty(k, dtype=torch.float32, device="cuda")
            ms = {key: [] for key in ("total", "grid_densify", "copy")}
            levels = []
            for rep in range(a.reps + 1):  # the first round warms everything up
                tt = _timed(torch, lambda: c.run(pa, pb))
                per = c.kernel_ms()
                tg = _timed(torch, lambda: dz.run(grid.compute(pa, pb, psz=psz, lv_f=LV_F), pa, pb, psz))
                tcopy = _timed(torch, lambda: dst.copy_(src))
                if rep:
                    levels.append(per)
                    for key, v in zip(("total", "grid_densify", "copy"), (tt, tg, tcopy)):
                        ms[key].append(float(v))
            levels = np.stack(levels)  # [rep][level][search, densify, refine]
            rec = {"w": w, "h": h, "psz": psz, "levels": []}
            for l in range(LV_F, -1, -1):
                lw, lh, nx, ny = c.level_dims(l)
                status = np.bincount(c.level(l)[2].ravel(), minlength=5)
                rec["levels"].append({"level": l, "w": lw, "h": lh, "nodes": nx * ny, "status_counts": status.tolist(),
                                      "search_ms": stats(levels[:, l, 0]), "densify_ms": stats(levels[:, l, 1])})
            for key, v in ms.items():
                rec[key + "_ms"] = stats(v)
            rec["sum_of_stage_events_ms"] = round(float(np.median(levels[:, :, :2].sum(axis=(1, 2)))), 4)
            rec["total_over_grid_densify"] = round(rec["total_ms"]["median"] / rec["grid_densify_ms"]["median"], 2)
            rec["total_over_copy"] = round(rec["total_ms"]["median"] / rec["copy_ms"]["median"], 1)
            rec["mean_abs_difference_to_grid_densify_px"] = round(float(np.abs(c.dense() - dz.dense()).mean()), 4)
            out["shapes"].append(rec)
            print(json.dumps(rec), flush=True)
    if a.parent_root:
        runs = {"this": {}, "parent": {}}
        for _ in range(2):
            for side, root in (("parent", os.path.abspath(a.parent_root)), ("this", ROOT)):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--default-child", root, "--reps", str(a.reps)],
                                   capture_output=True, text=True, timeout=600, cwd=root)
                if r.returncode != 0:
                    raise SystemExit(f"the {side} child failed:\n{r.stdout}\n{r.stderr}")
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("DEFAULT ")][-1]
                for shape, d in json.loads(line[8:]).items():
                    for key, v in d.items():
                        runs[side].setdefault((shape, key), []).extend(v)
        out["default_paths"] = {}
        for (shape, key), v in runs["this"].items():
            t, q = stats(v), stats(runs["parent"][shape, key])
            bar = bool(t["median"] <= q["max"])
            out["default_paths"].setdefault(shape, {})[key] = {
                "this_tree": t, "parent": q, "bar_median_not_above_parent_max": bar,
                "median_below_parent_min": bool(t["median"] < q["min"])}
            ok &= bar
        print(json.dumps(out["default_paths"]), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
