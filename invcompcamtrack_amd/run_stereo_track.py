"""The checked stereo track window of a sequence (run_test_OF_track.py:170-223):

  python -m invcompcamtrack_amd.run_stereo_track listfile out.npz [--bsize 14] [--fields in.npz] [--host]
         [--psz 15] [--lv_f 3] [--step 4] [--th_ratio 0.2] [--th_abs 1.0] [--disparity 2d|1d]
         [--refine [alpha,gamma,delta,outer,sor,omega]] [--densify [minerr,power]] [--flow grid|c2f|c2f-1d]
         [--patnorm] [--lv-l N] [--colour] [--cost l2|huber] [--huber-k K] [--lockstep]

listfile holds a left and a right image path per line (PGM or .npy), the frames in order; the first bsize lines are read.
Per frame the stereo flow grids and per frame pair the temporal ones are computed on the device and handed to the window
(StereoPointTracker); --disparity 1d computes the stereo grids with the 1-D search along x (FlowGrid.compute_x) instead of
the 2-D tracker with y dropped. --refine refines every grid's dense field per pixel on the device before the window reads it
(patchflow.FlowRefiner; without a value its defaults 16,13,4.5,8,5,1.6; the stereo fields move along x only). --densify
densifies every grid photometrically first (patchflow.FlowDensifier; without a value its defaults 2,1): grid -> densify
-> refine. --flow c2f computes every field coarse to fine instead (patchflow.CoarseToFineFlow: search, densification and,
with --refine, refinement per pyramid level; --densify and --refine then give the per-level parameters; not with
--disparity 1d). --flow c2f-1d is --flow c2f with the stereo pair searched along x only (CoarseToFineFlow's x_only; the
temporal fields stay 2-D; --disparity is not consulted). --patnorm switches on the coarse-to-fine flow's patch-mean normalisation, for cameras or frames of
differing brightness (with --flow c2f or c2f-1d only). --lv-l N stops every coarse-to-fine object at level N and up-samples that
level's field to the frame (CoarseToFineFlow's lv_l; default 0; with --flow c2f or c2f-1d only). --colour reads the frames
as three channels (io_formats.read_image_rgb: .npy of (h, w, 3), binary .ppm, else PIL) and computes every field on colour
frames (CoarseToFineFlow's channels=3; with --flow c2f or c2f-1d only). --cost huber searches every coarse-to-fine field with
the Huber patch cost, the residuals clipped to +-K grey levels (CoarseToFineFlow's cost and huber_k; --huber-k K, default 5;
with --flow c2f or c2f-1d only; --cost l1 is refused: L1 is not built). --lockstep runs a frame's coarse-to-fine objects in
lockstep, one launch per level and stage for all of them (patchflow.CoarseToFineFlowSet; with --flow c2f or c2f-1d only):
the same fields and the same file, bit for bit; with --host it changes nothing. With --fields the dense fields come from in.npz as the script reads them from .flo / .pfm files
instead (listfile is not read and may be ``-``): ``disp_lr``, ``disp_rl`` (bsize, H, W), ``flow_l``, ``flow_r``
(>= bsize-1, 2 = fwd / bwd, H, W, 2) and optionally ``xy0`` (N, 2). out.npz: ``xy_t`` (M, 4, bsize) and ``rows`` (M,), the
keys that run_static_split --stereo and run_fit_cameras --stereo read. The window runs on the GPU; --host runs the host
restatement on the same fields instead (same bits; from a listfile the grids' dense fields are formed for it).
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from . import io_formats as iof
from . import stereotrack as S


def dense_fields_of(tracker):
    """The dense fields of a StereoPointTracker built with keep_grids=True, in the host function's layout: of its
    coarse-to-fine objects with flow="c2f" or "c2f-1d", else of its refiners when it refines, else of its densifiers when it
    densifies, else of its grids."""
    g = (tracker.flows if tracker.flow in ("c2f", "c2f-1d") else tracker.refiners if tracker.refine is not None else
         tracker.densifiers if tracker.densify is not None else tracker.grids)
    lr = [-x["lr"].dense()[:, :, 0] for x in g]  # a left -> right grid is the script's -imgs_d[fr][0]
    rl = [np.ascontiguousarray(x["rl"].dense()[:, :, 0]) for x in g]
    fl = [(x["l_fwd"].dense(), x["l_bwd"].dense()) for x in g[1:]]
    fr = [(x["r_fwd"].dense(), x["r_bwd"].dense()) for x in g[1:]]
    return lr, rl, fl, fr


def refine_params(text):
    """'alpha,gamma,delta,outer,sor,omega' (a prefix will do; '' for the defaults) -> the dict StereoPointTracker takes."""
    from .patchflow import REFINE_DEFAULTS
    names = ("alpha", "gamma", "delta", "n_outer", "n_sor", "omega")
    vals = [v for v in text.split(",") if v.strip()] if text else []
    if len(vals) > len(names):
        raise argparse.ArgumentTypeError("--refine takes at most alpha,gamma,delta,outer,sor,omega")
    try:
        return {n: type(REFINE_DEFAULTS[n])(float(v)) for n, v in zip(names, vals)}
    except ValueError:
        raise argparse.ArgumentTypeError(f"--refine: not a number in {text!r}")


def densify_params(text):
    """'minerr,power' (a prefix will do; '' for the defaults) -> the dict StereoPointTracker takes."""
    vals = [v for v in text.split(",") if v.strip()] if text else []
    if len(vals) > 2:
        raise argparse.ArgumentTypeError("--densify takes at most minerr,power")
    try:
        return {n: t(v) for (n, t), v in zip((("minerr", float), ("power", int)), vals)}
    except ValueError:
        raise argparse.ArgumentTypeError(f"--densify: not a number in {text!r}")


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m invcompcamtrack_amd.run_stereo_track", description=__doc__.split("\n")[0])
    ap.add_argument("listfile")
    ap.add_argument("output")
    ap.add_argument("--bsize", type=int, default=14)
    ap.add_argument("--fields")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--psz", type=int, default=15)
    ap.add_argument("--lv_f", type=int, default=3)
    ap.add_argument("--step", type=int, default=4)
    ap.add_argument("--th_ratio", type=float, default=0.2)
    ap.add_argument("--th_abs", type=float, default=1.0)
    ap.add_argument("--disparity", choices=("2d", "1d"), default="2d")
    ap.add_argument("--refine", nargs="?", const="", default=None, type=refine_params)
    ap.add_argument("--densify", nargs="?", const="", default=None, type=densify_params)
    ap.add_argument("--flow", choices=("grid", "c2f", "c2f-1d"), default="grid")
    ap.add_argument("--patnorm", action="store_true")
    ap.add_argument("--lv-l", dest="lv_l", type=int, default=0)
    ap.add_argument("--colour", action="store_true")
    ap.add_argument("--cost", default="l2")
    ap.add_argument("--huber-k", dest="huber_k", type=float, default=None)
    ap.add_argument("--lockstep", action="store_true",
                    help="run a frame's coarse-to-fine objects in lockstep, one launch per level and stage for all of them "
                         "(--flow c2f or c2f-1d): the same output bit for bit; with --host it changes nothing")
    a = ap.parse_args(sys.argv[1:] if argv is None else list(argv))
    if a.colour and a.flow not in ("c2f", "c2f-1d"):
        ap.error("--colour needs --flow c2f or c2f-1d: colour frames are built for the coarse-to-fine flow alone")
    if a.colour and a.fields:
        ap.error("--colour reads frames; --fields brings fields that are computed already")
    if a.flow == "c2f" and a.disparity == "1d":
        ap.error("--flow c2f with --disparity 1d: the 1-D form of the coarse-to-fine flow is --flow c2f-1d")
    if a.patnorm and a.flow not in ("c2f", "c2f-1d"):
        ap.error("--patnorm needs --flow c2f: patch-mean normalisation is built for the coarse-to-fine flow alone")
    if a.lv_l and a.flow not in ("c2f", "c2f-1d"):
        ap.error("--lv-l needs --flow c2f or c2f-1d: a finest level above 0 is built for the coarse-to-fine flow alone")
    if (a.cost != "l2" or a.huber_k is not None) and a.flow not in ("c2f", "c2f-1d"):
        ap.error("--cost and --huber-k need --flow c2f or c2f-1d: the patch cost is built for the coarse-to-fine flow alone")
    lockstep = a.lockstep and not a.host  # (--host: nothing changes)
    if lockstep and a.flow not in ("c2f", "c2f-1d"):
        ap.error("--lockstep needs --flow c2f or c2f-1d: lockstep sets are built for the coarse-to-fine flow alone")
    try:
        from .patchflow import _c2f_cost
        _c2f_cost(a.cost, 5.0 if a.huber_k is None else a.huber_k, "--cost")
    except ValueError as e:
        ap.error(str(e))
    cost = dict(cost=a.cost, huber_k=5.0 if a.huber_k is None else a.huber_k) if a.flow in ("c2f", "c2f-1d") else {}
    th = dict(th_ratio=a.th_ratio, th_abs=a.th_abs)
    if a.fields:
        with np.load(a.fields) as z:
            b = min(a.bsize, len(z["disp_lr"]))
            lr, rl, fl, fr = z["disp_lr"][:b], z["disp_rl"][:b], z["flow_l"], z["flow_r"]
            xy0 = z["xy0"] if "xy0" in z else None
        xy_t, rows = (S.stereo_track_window_host if a.host else S.stereo_track_window)(lr, rl, fl, fr, xy0=xy0, **th)
    else:
        pairs = [ln.split() for ln in iof.read_image_list(a.listfile)][:a.bsize]
        if not pairs or any(len(p) != 2 for p in pairs):
            print("the list needs a left and a right path per line", file=sys.stderr)
            return 2
        read = iof.read_image_rgb if a.colour else iof.read_image_gray
        frames = [[np.asarray(read(fn), np.float32) for fn in p] for p in pairs]
        h, w = frames[0][0].shape[:2]
        t = S.StereoPointTracker(w, h, len(frames), a.step, a.psz, a.lv_f, keep_grids=a.host, disparity=a.disparity,
                                 refine=a.refine, densify=a.densify, flow=a.flow, patnorm=a.patnorm, lv_l=a.lv_l,
                                 colour=a.colour, lockstep=lockstep, **cost, **th)
        for left, right in frames:
            t.push_frames(left, right)
        xy_t, rows = S.stereo_track_window_host(*dense_fields_of(t), **th) if a.host else t.window()
    np.savez(a.output, xy_t=xy_t, rows=rows)
    print("kept %d points in %d frames" % (len(rows), xy_t.shape[2]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
