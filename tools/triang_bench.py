"""Triangulation timings: one JSON line (and profiles/triang_bench.json with --out).

  python tools/triang_bench.py [--reps 3] [--no-host] [--no-trace] [--out profiles/triang_bench.json]

For 10^4 and 10^5 tracks at a mean of 7 (2..12) and of 20 (8..32) views, each mode:
  device_ms   triangulate_tracks wall time: create, upload, repack, launch, read-back (min of reps after a warm-up)
  kernel_us   k_triang alone, from one `rocprofv3 --kernel-trace --stats` run of this script's --child mode
  host_ms     the NumPy restatement tests/triang_np.py on this machine (one run)
  read_gbs    bytes the kernel reads per sweep over the views (12 B of observations + 48 B of camera per view) x the
              sweeps of the mode x iterations run, over the kernel time; hbm_share = that over 8 TB/s. These working sets
              (<= 30 MB) sit in the Infinity Cache: the share says how far the kernel is from a streaming bound, not that
              it streams from HBM.
The iterative modes start from the device's DLT points (their upload is part of device_ms, the DLT run is not).
"""
from __future__ import annotations

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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from invcompcamtrack_amd import triang as T  # noqa: E402

FC, CC = np.array([1000.0, 1200.0]), np.array([660.0, 390.0])
CONFIGS = [(10000, 2, 12), (10000, 8, 32), (100000, 2, 12), (100000, 8, 32)]
MODES = ("dlt", "gn", "lm", "depth")
CHILD_REPS = 3
HBM_PEAK = 8.0e12
# sweeps over a point's views per iteration (LM: 2 for the normal equations, 1 for the trial point; a rejected trial adds 3)
SWEEPS = dict(dlt=2, gn=2, lm=3, depth=1)


def scene(n, lmin, lmax, nf=64, seed=17):
    rng = np.random.default_rng(seed)
    poses = np.zeros((nf, 6))
    poses[:, 0] = -0.2 * np.arange(nf) + rng.normal(0, 0.01, nf)
    poses[:, 1:3] = rng.normal(0, 0.02, (nf, 2))
    poses[:, 3:] = rng.normal(0, 0.02, (nf, 3))
    cam = dict(fc=FC, cc=CC)
    P = T.cameras_from_poses(cam, poses)
    lens = rng.integers(lmin, lmax + 1, n)
    first = (rng.uniform(0, 1, n) * (nf - lens + 1)).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    view = (np.repeat(first, lens) + np.arange(off[-1]) - np.repeat(off[:-1], lens)).astype(np.int32)
    X = np.stack([rng.uniform(-3, 14, n), rng.uniform(-2, 2, n), rng.uniform(8, 14, n)], 1)
    Pv = P[view].astype(np.float64).reshape(-1, 3, 4)
    h = np.einsum("mij,mj->mi", Pv[:, :, :3], np.repeat(X, lens, 0)) + Pv[:, :, 3]
    xy = (h[:, :2] / h[:, 2:3] + rng.normal(0, 0.5, (len(h), 2))).astype(np.float32)
    campos, ptdir = T.rays_from_first_view(cam, poses, off, view, xy)
    return dict(P=P, off=off, view=view, xy=xy, campos=campos, ptdir=ptdir)


def child():
    """Under rocprofv3: per configuration and mode CHILD_REPS launches of k_triang, in CONFIGS x MODES order."""
    for n, lmin, lmax in CONFIGS:
        sc = scene(n, lmin, lmax)
        t = T.Triangulator(n, int(sc["off"][-1]), len(sc["P"]))
        t.set_cameras(sc["P"])
        t.set_tracks(sc["off"], sc["view"], sc["xy"])
        init = None
        for mode in MODES:
            for _ in range(CHILD_REPS):
                t.run_async(mode, init=init, campos=sc["campos"], ptdir=sc["ptdir"])
                r = t.wait()
            if mode == "dlt":
                init = r["pts"]


def kernel_times():
    """{(config index, mode): min kernel time in us} from one traced run of child(), or None when rocprofv3 is absent."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "triang", "--",
               sys.executable, os.path.abspath(__file__), "--child"]
        try:
            subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600, cwd=ROOT)
        except (OSError, subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
            print(f"triang_bench: no kernel trace ({e})", file=sys.stderr)
            return None
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            return None
        rows = []
        with open(files[0]) as f:
            for r in csv.DictReader(f):
                if "k_triang" in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort()
    if len(rows) != len(CONFIGS) * len(MODES) * CHILD_REPS:
        print(f"triang_bench: {len(rows)} k_triang dispatches in the trace, expected "
              f"{len(CONFIGS) * len(MODES) * CHILD_REPS}", file=sys.stderr)
        return None
    out, q = {}, 0
    for ci in range(len(CONFIGS)):
        for mode in MODES:
            out[(ci, mode)] = min(e - s for s, e in rows[q:q + CHILD_REPS]) / 1e3
            q += CHILD_REPS
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import invcompcamtrack_amd as ic
    if ic.device_count() < 1:
        raise SystemExit("triang_bench: no HIP device (timings are only taken on the GPU)")
    if a.child:
        child()
        return
    import triang_np as TN
    ktimes = None if a.no_trace else kernel_times()
    rows = []
    for ci, (n, lmin, lmax) in enumerate(CONFIGS):
        sc = scene(n, lmin, lmax)
        nobs = int(sc["off"][-1])
        lens = np.diff(sc["off"])
        init = T.triangulate_tracks(sc["P"], sc["off"], sc["view"], sc["xy"], "dlt")["pts"]
        for mode in MODES:
            kw = dict(init=None if mode == "dlt" else init, campos=sc["campos"], ptdir=sc["ptdir"])
            ts = []
            for _ in range(a.reps + 1):
                t0 = time.perf_counter()
                r = T.triangulate_tracks(sc["P"], sc["off"], sc["view"], sc["xy"], mode, **kw)
                ts.append(time.perf_counter() - t0)
            row = dict(points=n, views_mean=round(nobs / n, 2), observations=nobs, mode=mode,
                       device_ms=round(min(ts[1:]) * 1e3, 3), iters_mean=round(float(r["iters"].mean()), 2))
            if ktimes is not None:
                kus = ktimes[(ci, mode)]
                its = np.maximum(r["iters"], 1) if mode != "dlt" else np.ones(n)
                nbytes = float((lens * its).sum()) * 60.0 * SWEEPS[mode]
                row.update(kernel_us=round(kus, 1), read_gbs=round(nbytes / (kus * 1e-6) / 1e9, 1),
                           hbm_share=round(nbytes / (kus * 1e-6) / HBM_PEAK, 4))
            if not a.no_host:
                t0 = time.perf_counter()
                h = TN.triangulate(sc["P"], sc["off"], sc["view"], sc["xy"][:, 0], sc["xy"][:, 1], mode, **kw)
                row["host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                row["speedup"] = round(row["host_ms"] / row["device_ms"], 1)
                row["same_bits_as_host"] = bool(TN.same_bits(r["pts"], h["pts"]).all())
            rows.append(row)
    out = dict(bench="triang", what="triangulate_tracks wall time (min of reps), k_triang time from one rocprofv3 "
               "--kernel-trace --stats run, tests/triang_np.py on the same machine", rows=rows)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
