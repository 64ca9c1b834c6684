"""Time per frame pair of the point-track front end, device against host, on the same machine in the same run:

  python tools/frontend_bench.py [--reps 3] [--out profiles/frontend_bench.json] [--no-host] [--no-trace]

Workload: ten rendered 1920x1080 frames (synth.make_sequence, integer grey levels) that start in host memory, step 4,
psz 15, lv_f 3, 1000 corners, bsize 10 -- the defaults of run_OF_point_track.

  device_ms_per_pair  run_OF_point_track_hip, wall time from the first push_frame to the oftrack object (the device is idle
                      then), over the nine pairs; min of --reps runs after a warm-up run
  host_ms_per_pair    run_OF_point_track once (its node tracking is k_patchflow too; corners, fill, up-sampling and addframe
                      are NumPy), with the time of one good_features and one dense_flow call next to it
  kernels             per kernel name: dispatches and total / mean time of ONE `rocprofv3 --kernel-trace --stats` run of this
                      script's --child mode (the device loop once after a warm-up loop; tracing slows the host, so no wall
                      time is taken from that run)
  same_tracks         the two oftrack objects are equal, block by block
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, NFRAMES = 1920, 1080, 10
KW = dict(bsize=10, psz=15, lv_f=3, step=4, maxcorners=1000)
FRONTEND_KERNELS = ("k_gf_", "k_fg_", "k_pt_", "k_patchflow", "k_pyr_level")


def frames():
    from invcompcamtrack_amd import synth
    step = np.array([0.01, -0.006, 0.008, 0.001, -0.0008, 0.0015])
    base = np.array([0.3, -0.2, 0.5, 0.02, -0.03, 0.01])
    return synth.make_sequence(W, H, [base + k * step for k in range(NFRAMES)], 0, 10, seed=2)["frames"]


def device_loop(fr):
    from invcompcamtrack_amd import patchflow as pf
    t0 = time.perf_counter()
    o = pf.run_OF_point_track_hip(fr, **KW)  # ends in tracks(): every block is read back, the device is idle
    return o, time.perf_counter() - t0


def child(path):
    fr = list(np.load(path))
    device_loop(fr)
    device_loop(fr)


def kernel_split(fr):
    """{kernel name: dispatches, total_us, mean_us} of the second device loop of child(), or None without rocprofv3."""
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "frames.npy"), np.stack(fr))
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "frontend", "--",
               sys.executable, os.path.abspath(__file__), "--child", os.path.join(d, "frames.npy")]
        try:
            subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900, cwd=ROOT)
        except (OSError, subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
            print(f"frontend_bench: no kernel trace ({e})", file=sys.stderr)
            return None
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            return None
        rows = []
        with open(files[0]) as f:
            for r in csv.DictReader(f):
                name = r["Kernel_Name"].split("(")[0].split("<")[0].split("::")[-1].split(" ")[-1]
                if name.startswith(FRONTEND_KERNELS):
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    rows.sort()
    rows = rows[len(rows) // 2:]  # the two loops launch the same kernels: the second half is the warm loop
    out = {}
    for s, e, name in rows:
        k = out.setdefault(name, dict(dispatches=0, total_us=0.0))
        k["dispatches"] += 1
        k["total_us"] += (e - s) / 1e3
    for k in out.values():
        k["total_us"] = round(k["total_us"], 1)
        k["mean_us"] = round(k["total_us"] / k["dispatches"], 2)
        k["us_per_pair"] = round(k["total_us"] / (NFRAMES - 1), 1)
    return out


def same(a, b):
    if a.frcounter != b.frcounter:
        return False
    for x, y in zip(a.tracks + a.tracks_valid + a.tracks_absmovement, b.tracks + b.tracks_valid + b.tracks_absmovement):
        if (x is None) != (y is None) or (x is not None and not np.array_equal(x, y, equal_nan=True)):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import invcompcamtrack_amd as ic
    from invcompcamtrack_amd import patchflow as pf
    if ic.device_count() < 1:
        raise SystemExit("frontend_bench: no HIP device (timings are only taken on the GPU)")
    if a.child:
        child(a.child)
        return
    fr = frames()
    kernels = None if a.no_trace else kernel_split(fr)
    npairs = NFRAMES - 1
    dev, _ = device_loop(fr)  # warm-up: code objects, allocations
    ts = [device_loop(fr)[1] for _ in range(a.reps)]
    out = dict(bench="frontend", workload=dict(w=W, h=H, frames=NFRAMES, **KW),
               device_ms_per_pair=round(min(ts) / npairs * 1e3, 3),
               device_ms_per_pair_all=[round(t / npairs * 1e3, 3) for t in ts])
    if not a.no_host:
        t0 = time.perf_counter()
        host = pf.run_OF_point_track(fr, **KW)
        out["host_ms_per_pair"] = round((time.perf_counter() - t0) / npairs * 1e3, 1)
        out["speedup"] = round(out["host_ms_per_pair"] / out["device_ms_per_pair"], 1)
        out["same_tracks"] = same(host, dev)
        pa, pb = ic.Pyramid(fr[0], KW["lv_f"], KW["psz"], True), ic.Pyramid(fr[1], KW["lv_f"], KW["psz"], True)
        t0 = time.perf_counter()
        pf.good_features(fr[0], KW["maxcorners"], 0.001, 5)
        t1 = time.perf_counter()
        pf.dense_flow(pa, pb, step=KW["step"], psz=KW["psz"], lv_f=KW["lv_f"])
        t2 = time.perf_counter()
        out["host_good_features_ms"] = round((t1 - t0) * 1e3, 1)
        out["host_dense_flow_ms"] = round((t2 - t1) * 1e3, 1)
    if kernels is not None:
        out["kernels"] = kernels
        out["kernel_ms_per_pair"] = round(sum(k["total_us"] for k in kernels.values()) / npairs / 1e3, 3)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
