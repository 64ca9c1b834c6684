"""Frame-to-frame sequence: ms per frame of the device chain (SequenceTracker), of the same loop on the host through the
public per-pair API (track_sequence_host_loop) and of the CPU oracle chain, at the script's 4 0 8 10 0.01 1 1.
Two workloads: 1920x1080 with ~2000 selected points per pair (the team form) and 640x480 with ~100 (one workgroup).
Both GPU paths are timed from the same frame residency, with their engines made before the clock starts:
  *_host_frames:   frames in host memory; the chain's one copy of all frames and the host loop's per-frame uploads are
                   inside the timed region;
  *_device_frames: frames already in device memory (a torch tensor); the chain borrows them, the host loop builds its
                   pyramids from them.
Prints one JSON line.

  python tools/seq_bench.py [--frames N] [--reps R] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import invcompcamtrack_amd as ic  # noqa: E402
from invcompcamtrack_amd import sequence as sq  # noqa: E402
from seq_scene import make_pan  # noqa: E402


def cpu_chain(sc, args, cap, stride, nframes):
    from oracle import oracle as O
    O.build()
    oop = O.make_op(*args, cap)
    poses = [sc["poses"][0]]
    pyr = [O.Pyramid(sc["frames"][0], args[0], args[2]), None]
    t0 = time.perf_counter()
    for t in range(nframes - 1):
        pyr[1] = O.Pyramid(sc["frames"][t + 1], args[0], args[2])
        sel = sq.select_points(sc["pts3d"], poses[t], sc["cam"], stride, cap)
        tr = O.Tracker(oop, sc["cam"]["fc"], sc["cam"]["cc"], sc["cam"]["wh"])
        tr.set3dpoints(np.ascontiguousarray(sc["pts3d"][:, sel]))
        tr.setpose(poses[t], pyr[0], pyr[1])
        poses.append(tr.trackpose())
        tr.close()
        pyr[0] = pyr[1]
    return (time.perf_counter() - t0) * 1e3 / (nframes - 1)


def run(w, h, nworld, cap, stride, nframes, reps, cpu):
    args = (4, 0, 8, 10, 0.01, 1, 1)
    sc = make_pan(w, h, nframes, nworld, step=-0.25 * w / 320.0, seed=5)
    op = ic.optparam(*args, cap)
    cam = ic.CamClass(5, sc["cam"]["fc"], sc["cam"]["cc"], sc["cam"]["wh"], 8)
    import torch
    frames_dev = torch.from_numpy(sc["frames"]).cuda()
    torch.cuda.synchronize()
    st = sq.SequenceTracker(cam, op, sc["pts3d"], stride)
    eng = ic.TrackBatch(cam, op, 1)

    def chain(frames):
        st.track_async(frames, sc["poses"][0])
        return st.wait()

    def loop(frames):
        return sq.track_sequence_host_loop(cam, op, sc["pts3d"], frames, sc["poses"][0], stride, engine=eng)

    def timed(fn, frames):
        fn(frames)  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            r = fn(frames)
        return (time.perf_counter() - t0) * 1e3 / reps / (nframes - 1), r

    ms = {}
    for key, frames in (("host_frames", sc["frames"]), ("device_frames", frames_dev)):
        ms["chain_" + key], r = timed(chain, frames)
        ms["host_loop_" + key], _ = timed(loop, frames)
    out = dict(size=f"{w}x{h}", team=st.last_team, npts_mean=float(r["npts"].mean()),
               **{"ms_per_frame_" + k: round(v, 4) for k, v in ms.items()})
    if cpu:
        out["ms_per_frame_cpu"] = round(cpu_chain(sc, args, cap, stride, min(nframes, 6)), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    res = [run(1920, 1080, 52000, 2400, 10, a.frames, a.reps, not a.no_cpu),
           run(640, 480, 2000, 128, 10, a.frames, a.reps, not a.no_cpu)]
    print(json.dumps(dict(metric="sequence_ms_per_frame", params="4 0 8 10 0.01 1 1", results=res)))


if __name__ == "__main__":
    main()
