"""A lockstep set of six coarse-to-fine flows against the six objects' own runs (DESIGN.md §4 "Lockstep sets"):

  python tools/c2fset_bench.py [--reps 7] [--out profiles/c2fset_bench.json] [--shapes 1242x375,1920x1080] [--no-push]

One MI355X, step 4, lv_f 3, 1242x375 and 1920x1080, psz 8 and 15, six members on six different seeded grating pairs, three
variants: plain, the refinement's defaults, and the script's settings (patnorm, lv_l = 1, the refinement). Each round
measures CoarseToFineFlowSet.run and the six objects' run one after the other on the same stream in the same process, HIP
events around each of the two; the order of the two alternates from round to round; --reps rounds after a warm-up round.
Reported: the median (minimum - maximum) of each side and of the per-round ratio set / six runs, and the set's operations.

The bar (exit status 1), at 1242x375 on the rows plain at psz 8, plain at psz 15 and the refinement's defaults at psz 15:
the set's median lies below the six single runs' minimum. The other rows are recorded without a bar.

Then, without a bar (skipped with --no-push): StereoPointTracker.push_frames wall time per stereo frame with lockstep=True
against False in turn, flow="c2f", psz 15, refine=None and refine={}, medians of --reps windows of four frames.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP, LV_F, NFRAMES, MEMBERS = 4, 3, 4, 6
PSZS = (8, 15)
VARIANTS = (("plain", {}), ("refine", dict(refine={})), ("script", dict(patnorm=True, lv_l=1, refine={})))
BARRED = (("1242x375", 8, "plain"), ("1242x375", 15, "plain"), ("1242x375", 15, "refine"))


def _timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


_FRAMES = {}  # (w, h, member) -> the member's frame pair, rendered once


def measure(torch, ic, pf, frames, stats, w, h, psz, kw, reps):
    pairs = []
    for m in range(MEMBERS):  # a grating pair of its own per member
        if (w, h, m) not in _FRAMES:
            fr = frames(w, h, seed=20 + m)
            _FRAMES[w, h, m] = (fr[0][0], fr[1][0])
        a, b = _FRAMES[w, h, m]
        pairs.append((ic.Pyramid(a, LV_F, psz, True), ic.Pyramid(b, LV_F, psz, True)))
    mine = [pf.CoarseToFineFlow(w, h, LV_F, STEP, psz, **kw) for _ in range(MEMBERS)]
    single = [pf.CoarseToFineFlow(w, h, LV_F, STEP, psz, **kw) for _ in range(MEMBERS)]
    s = pf.CoarseToFineFlowSet(mine)

    def six():
        for c, (a, b) in zip(single, pairs):
            c.run(a, b)

    t_set, t_six = [], []
    for rep in range(reps + 1):  # the first round warms both up
        order = (("set", lambda: s.run(pairs)), ("six", six))
        got = {}
        for name, fn in (order if rep % 2 else order[::-1]):
            got[name] = float(_timed(torch, fn))
        if rep:
            t_set.append(got["set"])
            t_six.append(got["six"])
    same = all(a.dense().tobytes() == b.dense().tobytes() for a, b in zip(mine, single))
    return {"set_ms": stats(t_set), "six_runs_ms": stats(t_six),
            "ratio_set_over_six": stats([a / b for a, b in zip(t_set, t_six)]), "operations": s.operations(),
            "same_bits": bool(same)}


def push_frames(S, frames, stats, w, h, psz, refine, reps):
    fr = frames(w, h)
    ms = {False: [], True: []}
    for rep in range(reps + 1):
        for lockstep in ((False, True) if rep % 2 else (True, False)):
            t = S.StereoPointTracker(w, h, NFRAMES, STEP, psz, LV_F, flow="c2f", refine=refine, lockstep=lockstep)
            t0 = time.perf_counter()
            for left, right in fr:
                t.push_frames(left, right)
            t.win.count()  # waits for the device
            if rep:
                ms[lockstep].append((time.perf_counter() - t0) * 1e3 / NFRAMES)
    return {"lockstep_false_ms": stats(ms[False]), "lockstep_true_ms": stats(ms[True])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "c2fset_bench.json"))
    ap.add_argument("--shapes", default="1242x375,1920x1080")
    ap.add_argument("--no-push", action="store_true", help="leave the push_frames wall times out")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    import invcompcamtrack_amd as ic
    from invcompcamtrack_amd import patchflow as pf
    from invcompcamtrack_amd import stereotrack as S
    from tools.patchdisp_bench import frames, stats
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    out = {"device": torch.cuda.get_device_name(0), "step": STEP, "lv_f": LV_F, "members": MEMBERS, "reps": a.reps,
           "rows": {}, "bars": {}}
    ok = True
    for w, h in shapes:
        for psz in PSZS:
            for name, kw in VARIANTS:
                r = measure(torch, ic, pf, frames, stats, w, h, psz, kw, a.reps)
                key = (f"{w}x{h}", psz, name)
                if key in BARRED:
                    r["bar_set_median_below_six_runs_min"] = bool(r["set_ms"]["median"] < r["six_runs_ms"]["min"])
                    out["bars"]["%s psz %d %s" % key] = r["bar_set_median_below_six_runs_min"]
                    ok &= r["bar_set_median_below_six_runs_min"]
                ok &= r["same_bits"]
                out["rows"].setdefault(key[0], {}).setdefault(f"psz{psz}", {})[name] = r
                print("%s psz %d %s" % key, json.dumps(r), flush=True)
    if not a.no_push:
        out["push_frames_wall_ms_per_stereo_frame"] = {}
        for w, h in shapes:
            for name, refine in (("refine_none", None), ("refine_defaults", {})):
                r = push_frames(S, frames, stats, w, h, PSZS[1], refine, a.reps)
                out["push_frames_wall_ms_per_stereo_frame"].setdefault(f"{w}x{h}", {})[name] = r
                print(f"push_frames {w}x{h} psz {PSZS[1]} {name}", json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("bars:", json.dumps(out["bars"]), "->", "ok" if ok else "MISSED", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
