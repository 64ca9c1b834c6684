"""Triangulates the tracks of a text file on the GPU:

  python -m invcompcamtrack_amd.run_triangulate in.txt out.txt [--mode dlt|gn|lm|depth]

The file format is this project's own (the reference has none). Blank lines are ignored; numbers are separated by blanks:

  F                                    cameras
  F lines of 12 numbers                row-major 3x4 camera matrices
  n                                    tracks
  n lines `L v0 x0 y0 v1 x1 y1 ...`    L >= 2 observations: camera index, pixel x, pixel y
  noiter minres damp_init damp_fct maxdamp
  has_init has_rays                    0 / 1 each
  n lines `X Y Z`                      when has_init: the start points of gn / lm / depth
  n lines `cx cy cz dx dy dz`          when has_rays: centre and unit ray of the depth-only mode

Without start points an iterative mode starts from the DLT points (a DLT run first). out.txt has one line per point:
`X Y Z`, the covariance (9 numbers row-major; depth: 1), the iteration count and the status word (bit 0 non-finite, bit
1 behind the first view), floats as %.9g, NaN as `nan`. tests/cxx/triang_driver.cpp reads and writes the same files
through CTR::TriangClass.
"""
from __future__ import annotations

import argparse
import math
import sys

import numpy as np

from .triang import MODES, triangulate_tracks


def _fmt(v):
    v = float(v)
    return "nan" if math.isnan(v) else "%.9g" % v


def write_triang_input(path, P, offsets, view, xy, noiter=10, minres=1e-5, damp_init=2.0, damp_fct=10.0, maxdamp=1e10,
                       init=None, campos=None, ptdir=None):
    P = np.asarray(P, np.float32).reshape(-1, 12)
    off = np.asarray(offsets, np.int64)
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    with open(path, "w") as f:
        f.write("%d\n" % len(P))
        for row in P:
            f.write(" ".join(_fmt(v) for v in row) + "\n")
        f.write("%d\n" % (len(off) - 1))
        for i in range(len(off) - 1):
            s = ["%d" % (off[i + 1] - off[i])]
            for j in range(off[i], off[i + 1]):
                s += ["%d" % view[j], _fmt(xy[j, 0]), _fmt(xy[j, 1])]
            f.write(" ".join(s) + "\n")
        f.write("%d %s %s %s %s\n" % (noiter, _fmt(np.float32(minres)), _fmt(np.float32(damp_init)),
                                      _fmt(np.float32(damp_fct)), _fmt(np.float32(maxdamp))))
        rays = campos is not None and ptdir is not None
        f.write("%d %d\n" % (init is not None, rays))
        if init is not None:
            for r in np.asarray(init, np.float32).reshape(-1, 3):
                f.write(" ".join(_fmt(v) for v in r) + "\n")
        if rays:
            for c, d in zip(np.asarray(campos, np.float32).reshape(-1, 3), np.asarray(ptdir, np.float32).reshape(-1, 3)):
                f.write(" ".join(_fmt(v) for v in list(c) + list(d)) + "\n")


def read_triang_input(path):
    with open(path) as f:
        lines = [ln.split() for ln in f if ln.strip()]
    it = iter(lines)
    F = int(next(it)[0])
    P = np.array([[float(t) for t in next(it)[:12]] for _ in range(F)], np.float32).reshape(F, 12)
    n = int(next(it)[0])
    off, view, xy = [0], [], []
    for _ in range(n):
        t = next(it)
        L = int(t[0])
        if len(t) < 1 + 3 * L:
            raise ValueError(f"{path}: a track line announces {L} observations and holds fewer")
        for k in range(L):
            view.append(int(t[1 + 3 * k]))
            xy.append((float(t[2 + 3 * k]), float(t[3 + 3 * k])))
        off.append(len(view))
    t = next(it)
    opt = dict(noiter=int(t[0]), minres=float(t[1]), damp_init=float(t[2]), damp_fct=float(t[3]), maxdamp=float(t[4]))
    t = next(it)
    has_init, has_rays = int(t[0]), int(t[1])
    init = np.array([[float(v) for v in next(it)[:3]] for _ in range(n)], np.float32) if has_init else None
    campos = ptdir = None
    if has_rays:
        r = np.array([[float(v) for v in next(it)[:6]] for _ in range(n)], np.float32)
        campos, ptdir = r[:, :3].copy(), r[:, 3:].copy()
    return dict(P=P, offsets=np.array(off, np.int64), view=np.array(view, np.int32),
                xy=np.array(xy, np.float32).reshape(-1, 2), init=init, campos=campos, ptdir=ptdir, **opt)


def write_triang_result(path, res):
    cov = np.asarray(res["cov"], np.float32).reshape(len(res["pts"]), -1)
    with open(path, "w") as f:
        for i in range(len(res["pts"])):
            s = [_fmt(v) for v in res["pts"][i]] + [_fmt(v) for v in cov[i]]
            f.write(" ".join(s) + " %d %d\n" % (res["iters"][i], res["status"][i]))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m invcompcamtrack_amd.run_triangulate",
                                 description=__doc__.split("\n")[0])
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--mode", choices=sorted(MODES), default="dlt")
    a = ap.parse_args(sys.argv[1:] if argv is None else list(argv))
    inp = read_triang_input(a.input)
    if a.mode == "depth" and inp["campos"] is None:
        print("[run_triangulate] the depth-only mode needs the rays section of the input", file=sys.stderr)
        return 2
    res = triangulate_tracks(inp["P"], inp["offsets"], inp["view"], inp["xy"], a.mode, inp["noiter"], inp["minres"],
                             inp["damp_init"], inp["damp_fct"], inp["maxdamp"], inp["init"], inp["campos"], inp["ptdir"])
    write_triang_result(a.output, res)
    print(f"[run_triangulate] {len(res['pts'])} points, mode {a.mode}: {int((res['status'] & 1).sum())} non-finite, "
          f"{int((res['status'] >> 1 & 1).sum())} behind their first view")
    return 0


if __name__ == "__main__":
    sys.exit(main())
