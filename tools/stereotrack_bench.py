"""Stereo track window timings: one JSON line, also written to profiles/stereotrack_bench.json.

  python tools/stereotrack_bench.py [--reps 7] [--out profiles/stereotrack_bench.json]

KITTI size 1242 x 375, bsize 14, every pixel (465 750 start points), dense float32 fields (two planes and four flows per
step, 18.6 MB). Reported: wall_ms_host_fields, stereo_track_window with the fields starting in host memory (create, every
upload and launch, both read-backs; the host clock stops after the rows are back), and wall_ms_device_fields, the same with
the fields resident in device memory beforehand: after a warm-up run, --reps runs, as minimum, median and maximum
(the caller holds the previous result while the next is made; *_result_released: it drops it first); kernel_ms, the device time of the open / advance launches and of the compaction launches from events around them (runs of
their own with set_timing, device fields); host_ms, stereo_track_window_host in the same process on all 14 frames, one
run, not scaled; phases_ms_median_*, the same window through open / advance / count / read with the host clock read
between them. The device result is checked against the host's.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from invcompcamtrack_amd import stereotrack as S  # noqa: E402

W, H, BSIZE = 1242, 375, 14


def scene(seed=0):
    """A disparity plane of 12 .. 28 px carried along by a translation of about 3 px per frame, the right disparity and the
    backward flows to first order, 0.2 % of the pixels of every field disturbed."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)

    def D(x, y):
        return 20.0 + 8.0 * np.sin(x / 300.0) * np.cos(y / 200.0)
    ang = rng.uniform(0, 2 * np.pi, BSIZE)
    step = np.stack([3.0 * np.cos(ang), 1.5 * np.sin(ang)], 1)
    shift = np.concatenate([[np.zeros(2)], np.cumsum(step, 0)])
    lr, rl, fl, fr = [], [], [], []
    for k in range(BSIZE):
        d = D(xx - shift[k, 0], yy - shift[k, 1])
        back = D(xx + d - shift[k, 0], yy - shift[k, 1])
        f = np.empty((2, H, W, 2), np.float32)
        f[0] = step[k]
        f[1] = -step[k]
        g = f.copy()
        for a in (d, back, f[0, :, :, 0], f[1, :, :, 1], g[0, :, :, 1], g[1, :, :, 0]):
            a += np.where(rng.uniform(size=a.shape) < 0.002, 2.0, 0.0).astype(np.float32)
        lr.append(d.astype(np.float32))
        rl.append(back.astype(np.float32))
        fl.append(f)
        fr.append(g)
    return np.stack(lr), np.stack(rl), np.stack(fl), np.stack(fr)


def phases(win, f):
    """One window through the object's own calls: seconds spent in open + advances (uploads of host fields and the
    launches), in count (the wait for the kernels and M) and in read (the transposition and the copy of the M rows)."""
    lr, rl, fl, fr = f
    t0 = time.perf_counter()
    win.open(S.field(lr[0], -1), rl[0])
    for k in range(1, BSIZE):
        win.advance(fl[k - 1][0], fl[k - 1][1], fr[k - 1][0], fr[k - 1][1], S.field(lr[k], -1), rl[k])
    t1 = time.perf_counter()
    win.count()
    t2 = time.perf_counter()
    win.read()
    return t1 - t0, t2 - t1, time.perf_counter() - t2


def spread(ts):
    ts = sorted(ts)
    return dict(min=round(ts[0] * 1e3, 3), median=round(statistics.median(ts) * 1e3, 3), max=round(ts[-1] * 1e3, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stereotrack_bench.json"))
    a = ap.parse_args()
    import invcompcamtrack_amd as ic
    if ic.device_count() < 1:
        raise SystemExit("stereotrack_bench: no HIP device (timings are only taken on the GPU)")
    import torch
    args = scene()
    dev_args = [torch.from_numpy(x).cuda() for x in args]
    torch.cuda.synchronize()
    win = S.StereoTrackWindow(W, H, BSIZE)
    out = {}
    for name, fields in (("wall_ms_host_fields", args), ("wall_ms_device_fields", dev_args)):
        got = S.stereo_track_window(*fields, window=win)  # warm-up: the window's buffers exist afterwards
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            got = S.stereo_track_window(*fields, window=win)
            ts.append(time.perf_counter() - t0)
        out[name] = spread(ts)
        ts = []
        for _ in range(a.reps):  # the same with the previous result released first, so that its pages can be used again
            got = None
            t0 = time.perf_counter()
            got = S.stereo_track_window(*fields, window=win)
            ts.append(time.perf_counter() - t0)
        out[name + "_result_released"] = spread(ts)
        got = None  # the phases too land their result in pages that were just released
        ph = [phases(win, fields) for _ in range(a.reps)]
        out[name.replace("wall_ms", "phases_ms_median")] = dict(
            open_and_advances=round(statistics.median(p[0] for p in ph) * 1e3, 3),
            count=round(statistics.median(p[1] for p in ph) * 1e3, 3), read=round(statistics.median(p[2] for p in ph) * 1e3, 3))
    got = S.stereo_track_window(*dev_args, window=win)
    win.set_timing(True)
    ks = []
    for _ in range(a.reps):
        S.stereo_track_window(*dev_args, window=win)
        ks.append(win.kernel_times())
    win.set_timing(False)
    t0 = time.perf_counter()
    host = S.stereo_track_window_host(*args)
    host_s = time.perf_counter() - t0
    same = bool(got[0].tobytes() == host[0].tobytes() and got[1].tobytes() == host[1].tobytes())
    step_bytes = 4 * W * H * (2 + 4 * 2)
    out = dict(bench="stereotrack", w=W, h=H, bsize=BSIZE, points=W * H, kept=int(len(host[1])), reps=a.reps,
               field_bytes_per_step=step_bytes, field_bytes_total=step_bytes * (BSIZE - 1) + 4 * W * H * 2,
               state_bytes=32 * W * H * BSIZE, result_bytes=int(host[0].nbytes + host[1].nbytes), launches=BSIZE + 4, **out,
               kernel_ms=dict(track_min=round(min(k[0] for k in ks), 4), track_median=round(statistics.median(k[0] for k in ks), 4),
                              compact_min=round(min(k[1] for k in ks), 4),
                              compact_median=round(statistics.median(k[1] for k in ks), 4)),
               host_ms=round(host_s * 1e3, 1), host_frames=BSIZE, host_scaled=False,
               speedup_host_fields_median=round(host_s * 1e3 / out["wall_ms_host_fields"]["median"], 1),
               speedup_device_fields_median=round(host_s * 1e3 / out["wall_ms_device_fields"]["median"], 1),
               same_as_host=same)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
