"""A stereo track window to one camera per frame without leaving the device: misc_src/run_test_OF_track.py:170-223 (the
checked window), 309-343 (the static split) and 360-411 (depth, camera fit, the two reprojection means) as one pipeline.

The window's history stays where ``StereoTrackWindow.count`` left it; kernels write the split's view pairs and the fit's
points and observations from it (``ictr_*_from_window``), the split's inlier words reach the fit on the device, and what
comes back is what the script prints and plots: poses, statuses, the mask words, two vectors of means.

  window_cameras_host    the definition: the host stages of stereotrack, fsplit and camfit in the script's order
  cameras_from_window    a counted StereoTrackWindow -> the result, on the device
  window_cameras         fields in -> the result, on the device
  cameras_from_tracks    a read-back xy_t -> the result through the host-array device stages (split_static, fit_cameras,
                         reprojection_errors): the way without the hand-over, same bits
  window_bundle_host     window_cameras_host, then the bundle adjustment (bundle.adjust_window_host) of the fit's poses and
                         the inliers' points over both cameras
  bundle_from_window     cameras_from_window, then the same adjustment on the device from the window's own buffers
  window_ransac_cameras_host   the window, then the window camera RANSAC (camransac.window_ransac_host) over both sides, the
                         fit started from the RANSAC poses on the RANSAC inliers, both means; bundle=True: the adjustment too
  ransac_cameras_from_window   the same from a counted StereoTrackWindow, on the device
  ransac_cameras         fields in -> the same result, on the device

The result is a dict: ``m``; the split's ``words``, ``mask``, ``inliers``, ``best_trial``, ``best_count``, ``draws``,
``F``, ``dd``; the fit's ``G``, ``p``, ``cost``, ``damp``, ``iters``, ``status``, ``n``; ``err_left`` and ``err_right``
(bsize,), the mean reprojection distance per frame in the left camera and, with ``offset`` (default (baseline, 0, 0))
added to every translation, against the right observations. Limits (DESIGN.md §4 "Window hand-over"): 2 <= bsize <= 65,
8 <= M <= 2^22.

The three RANSAC functions keep ``m``, the fit's keys, ``err_left`` and ``err_right``; in place of the split's keys they
carry the RANSAC's ``words``, ``mask``, ``inliers``, ``best_trial``, ``best_count``, ``draws``, ``dd`` and its poses as
``G_ransac``, ``p_ransac``. If no trial succeeded nothing is fitted: every status is FEW_OBS (3), the poses, costs and means
are NaN. With ``bundle=True`` they add ``ba``, ``err_left_ba``, ``err_right_ba`` (None and NaN then). bsize <= 64.

The two bundle functions add ``ba`` (the result of the adjustment: G, p, X, cost, damp, iters, status, n) and ``err_left_ba``,
``err_right_ba``, the two means at the adjusted poses and points. The adjustment starts from the fit's poses (12 bsize
doubles that cross the host) and takes 2 <= bsize <= 32.
"""
from __future__ import annotations

import numpy as np

from . import bundle as B
from . import camfit as F
from . import camransac as R
from . import fsplit as S
from . import stereotrack as T

__all__ = ["window_cameras_host", "window_cameras", "cameras_from_window", "cameras_from_tracks", "window_bundle_host",
           "bundle_from_window", "window_ransac_cameras_host", "ransac_cameras_from_window", "ransac_cameras", "MAX_BSIZE",
           "MIN_POINTS", "MAX_POINTS"]

MAX_BSIZE = 65          # 2 (bsize // 2) view pairs, the split holds 64
MIN_POINTS = 8          # one draw of the split
MAX_POINTS = 1 << 22    # the split's and the fit's

_SPLIT_KEYS = ("words", "mask", "inliers", "best_trial", "best_count", "draws", "F", "dd")
_FIT_KEYS = ("G", "p", "cost", "damp", "iters", "status", "n")
_RANSAC_KEYS = ("words", "mask", "inliers", "best_trial", "best_count", "draws", "dd")


def _check_size(m, bsize):
    if bsize < 2 or bsize > MAX_BSIZE:
        raise ValueError(f"a window of {bsize} frames cannot be split: bsize 2 .. {MAX_BSIZE}")
    if m < MIN_POINTS or m > MAX_POINTS:
        raise ValueError(f"the window kept {m} points: the split and the fit take {MIN_POINTS} .. 2^22")


def _offset(offset, baseline):
    return [float(baseline), 0.0, 0.0] if offset is None else [float(v) for v in np.asarray(offset, np.float64).reshape(3)]


def _result(m, split, fit, err_left, err_right):
    out = dict(m=int(m))
    out.update({k: split[k] for k in _SPLIT_KEYS})
    out.update({k: fit[k] for k in _FIT_KEYS})
    out.update(err_left=np.asarray(err_left, np.float64), err_right=np.asarray(err_right, np.float64))
    return out


def _from_tracks(xy_t, cam, baseline, ntrials, thresh, seed, offset, init, schedule, split_fn, fit_fn, reproj_fn):
    xy_t = np.asarray(xy_t, np.float64)
    if xy_t.ndim != 3 or xy_t.shape[1] != 4:
        raise ValueError(f"xy_t must be (M, 4, bsize), got {xy_t.shape}")
    pairs, rows = S.pairs_from_stereo_tracks(xy_t)
    _check_size(len(rows), xy_t.shape[2])
    split = split_fn(pairs, ntrials, thresh, seed)
    xy = xy_t[rows]
    X = F.points_from_first_view(xy, cam, F.depth_from_disparity(xy, F._as_cam(cam)[0], baseline))
    left, right = F.observations_from_stereo_tracks(xy)
    fit = fit_fn(X, left, cam, mask=split["words"], init=init, **schedule)
    err_l, _ = reproj_fn(X, left, cam, fit["G"], mask=split["words"])
    err_r, _ = reproj_fn(X, right, cam, fit["G"], mask=split["words"], offset=_offset(offset, baseline))
    return _result(len(rows), split, fit, err_l, err_r)


def cameras_from_tracks(xy_t, cam, baseline, ntrials=100, thresh=2.0, seed=0, offset=None, init=None, **schedule):
    """The result from a read-back block xy_t (M, 4, bsize) through the host-array device stages: NumPy repacks, the split,
    the fit and the means run on the device."""
    return _from_tracks(xy_t, cam, baseline, ntrials, thresh, seed, offset, init, schedule, S.split_static, F.fit_cameras,
                        F.reprojection_errors)


def window_cameras_host(disp_lr, disp_rl, flow_l, flow_r, cam, baseline, xy0=None, th_ratio=0.2, th_abs=1.0, ntrials=100,
                        thresh=2.0, seed=0, offset=None, init=None, tracks=False, **schedule):
    """The definition: stereo_track_window_host -> pairs_from_stereo_tracks -> split_static_host -> depth_from_disparity
    -> points_from_first_view -> observations_from_stereo_tracks -> fit_cameras_host on the inliers -> both
    reprojection_errors_host. tracks=True adds ``xy_t`` and ``rows``."""
    xy_t, rows = T.stereo_track_window_host(disp_lr, disp_rl, flow_l, flow_r, xy0=xy0, th_ratio=th_ratio, th_abs=th_abs)
    out = _from_tracks(xy_t, cam, baseline, ntrials, thresh, seed, offset, init, schedule, S.split_static_host,
                       F.fit_cameras_host, F.reprojection_errors_host)
    if tracks:
        out.update(xy_t=xy_t, rows=rows)
    return out


def cameras_from_window(win, cam, baseline, ntrials=100, thresh=2.0, seed=0, offset=None, init=None, objects=None,
                        **schedule):
    """The result from a StereoTrackWindow whose frames are all in (count() runs here if it has not): the hand-over, the
    split, the fit and the means on the device, everything on the null stream. ``objects``: a dict that keeps the
    StaticSplitter and the CameraFitter between calls; they are reused when the next window keeps the same M and bsize.
    ValueError for fewer than 8 survivors, more than 2^22, or bsize outside 2 .. 65; nothing is launched then."""
    m = win.survivors if win.survivors is not None else win.count()
    _check_size(m, win.bsize)
    F._params(schedule)
    key = (m, win.bsize)
    if objects is not None and objects.get("key") == key:
        split, fit = objects["split"], objects["fit"]
    else:
        split, fit = S.StaticSplitter(m, 2 * (win.bsize // 2)), F.CameraFitter(m, win.bsize)
        if objects is not None:
            objects.update(key=key, split=split, fit=fit)
    split.set_pairs_from_window(win)
    split.run_async(ntrials, thresh, seed)
    fit.set_camera(cam)
    fit.set_points_from_window(win, baseline)
    fit.set_observations_from_window(win, right=False)
    fit.set_mask_from_fsplit(split)
    fit.run_async(init, **schedule)
    s, f = split.wait(), fit.wait()
    err_l, _ = fit.reprojection_errors(f["G"])
    fit.set_observations_from_window(win, right=True)
    err_r, _ = fit.reprojection_errors(f["G"], _offset(offset, baseline))
    return _result(m, s, f, err_l, err_r)


def window_cameras(disp_lr, disp_rl, flow_l, flow_r, cam, baseline, xy0=None, th_ratio=0.2, th_abs=1.0, window=None,
                   tracks=False, ntrials=100, thresh=2.0, seed=0, offset=None, init=None, objects=None, **schedule):
    """window_cameras_host on the device, bit for bit: the fields of stereo_track_window (float32 in host memory or torch
    tensors on the device) in, the result out; xy_t is formed only with tracks=True, which adds ``xy_t`` and ``rows``.
    ``window``: a StereoTrackWindow of the right size to reuse; ``objects``: see cameras_from_window."""
    bsize = len(disp_lr)
    if bsize < 1 or len(disp_rl) != bsize:
        raise ValueError("disp_lr and disp_rl need one plane per frame, at least one frame")
    if len(flow_l) < bsize - 1 or len(flow_r) < bsize - 1:
        raise ValueError("flow_l and flow_r need bsize - 1 (fwd, bwd) pairs")
    if bsize < 2 or bsize > MAX_BSIZE:
        raise ValueError(f"a window of {bsize} frames cannot be split: bsize 2 .. {MAX_BSIZE}")
    h, w = tuple(disp_lr[0].shape)
    win = window if window is not None else T.StereoTrackWindow(w, h, bsize, th_ratio, th_abs)
    win.open(T.field(disp_lr[0], -1), disp_rl[0], xy0)
    for fr in range(1, bsize):
        win.advance(flow_l[fr - 1][0], flow_l[fr - 1][1], flow_r[fr - 1][0], flow_r[fr - 1][1], T.field(disp_lr[fr], -1),
                    disp_rl[fr])
    win.count()
    out = cameras_from_window(win, cam, baseline, ntrials, thresh, seed, offset, init, objects, **schedule)
    if tracks:
        xy_t, rows = win.read()
        out.update(xy_t=xy_t, rows=rows)
    return out


def _check_bundle(bsize, ba_schedule):
    if bsize > B.MAX_FRAMES:
        raise ValueError(f"a window of {bsize} frames cannot be adjusted: bsize 2 .. {B.MAX_FRAMES}")
    return F._params(dict(ba_schedule or {}))


def window_bundle_host(disp_lr, disp_rl, flow_l, flow_r, cam, baseline, xy0=None, th_ratio=0.2, th_abs=1.0, ntrials=100,
                       thresh=2.0, seed=0, offset=None, init=None, tracks=False, ba_schedule=None, **schedule):
    """The definition of bundle_from_window: window_cameras_host as it is, then adjust_window_host over the left and the
    right observations with the split's words as the mask, started from the fit's poses, and both
    reprojection_errors_host at the adjusted poses and points. ba_schedule: the adjustment's schedule (a dict)."""
    _check_bundle(len(disp_lr), ba_schedule)
    out = window_cameras_host(disp_lr, disp_rl, flow_l, flow_r, cam, baseline, xy0=xy0, th_ratio=th_ratio, th_abs=th_abs,
                              ntrials=ntrials, thresh=thresh, seed=seed, offset=offset, init=init, tracks=True, **schedule)
    _, keep = S.pairs_from_stereo_tracks(out["xy_t"])
    xy = out["xy_t"][keep]
    X = F.points_from_first_view(xy, cam, F.depth_from_disparity(xy, F._as_cam(cam)[0], baseline))
    left, right = F.observations_from_stereo_tracks(xy)
    off = _offset(offset, baseline)
    ba = B.adjust_window_host(X, np.stack([left, right]), cam, offset=off, mask=out["words"], init=out["G"],
                              **dict(ba_schedule or {}))
    err_l, _ = F.reprojection_errors_host(ba["X"], left, cam, ba["G"], mask=out["words"])
    err_r, _ = F.reprojection_errors_host(ba["X"], right, cam, ba["G"], mask=out["words"], offset=off)
    out.update(ba=ba, err_left_ba=err_l, err_right_ba=err_r)
    if not tracks:
        del out["xy_t"], out["rows"]
    return out


def bundle_from_window(win, cam, baseline, ntrials=100, thresh=2.0, seed=0, offset=None, init=None, objects=None,
                       ba_schedule=None, **schedule):
    """cameras_from_window as it is, then the adjustment on the device: the adjuster's points, both sides of its
    observations and its mask come from the window's and the split's device buffers, its start poses from the fit. The
    means at the adjusted poses and points are the fitter's, on the adjusted points. ``objects`` also keeps the
    BundleAdjuster."""
    _check_bundle(win.bsize, ba_schedule)
    objects = {} if objects is None else objects
    out = cameras_from_window(win, cam, baseline, ntrials, thresh, seed, offset, init, objects, **schedule)
    split, fit = objects["split"], objects["fit"]
    if objects.get("ba_key") != objects["key"]:
        objects.update(ba_key=objects["key"], ba=B.BundleAdjuster(out["m"], win.bsize, 2))
    ba = objects["ba"]
    off = _offset(offset, baseline)
    ba.set_camera(cam)
    ba.set_offset(off)
    ba.set_points_from_window(win, baseline)
    ba.set_observations_from_window(win)
    ba.set_mask_from_fsplit(split)
    ba.run_async(out["G"], **dict(ba_schedule or {}))
    res = ba.wait()
    fit.set_points(res["X"])
    fit.set_observations_from_window(win, right=False)
    err_l, _ = fit.reprojection_errors(res["G"])
    fit.set_observations_from_window(win, right=True)
    err_r, _ = fit.reprojection_errors(res["G"], off)
    out.update(ba=res, err_left_ba=err_l, err_right_ba=err_r)
    return out


# ---------------------------------------------------------------- the window camera RANSAC in front of the fit
def _check_ransac(m, bsize, bundle, schedule, ba_schedule):
    _check_size(m, bsize)
    if bsize > R.MAX_FRAMES:
        raise ValueError(f"a window of {bsize} frames cannot go through the camera RANSAC: bsize 2 .. {R.MAX_FRAMES}")
    F._params(schedule)
    if bundle:
        _check_bundle(bsize, ba_schedule)


def _no_fit(bsize, schedule):
    """The fit's keys when no trial succeeded: nothing was fitted."""
    nan = np.full(bsize, np.nan)
    return dict(G=np.full((bsize, 3, 4), np.nan), p=np.full((bsize, 6), np.nan), cost=nan.copy(),
                damp=np.full(bsize, F._params(schedule)["damp_init"]), iters=np.zeros(bsize, np.int32),
                status=np.full(bsize, F.FEW_OBS, np.int32), n=np.zeros(bsize, np.int64))


def _ransac_result(m, ran, fit, err_left, err_right):
    out = dict(m=int(m))
    out.update({k: ran[k] for k in _RANSAC_KEYS})
    out.update(G_ransac=ran["G"], p_ransac=ran["p"])
    out.update({k: fit[k] for k in _FIT_KEYS})
    out.update(err_left=np.asarray(err_left, np.float64), err_right=np.asarray(err_right, np.float64))
    return out


def window_ransac_cameras_host(disp_lr, disp_rl, flow_l, flow_r, cam, baseline, xy0=None, th_ratio=0.2, th_abs=1.0,
                               ntrials=100, thresh=2.0, seed=0, offset=None, bundle=False, tracks=False, ba_schedule=None,
                               **schedule):
    """The definition: stereo_track_window_host -> depth_from_disparity -> points_from_first_view ->
    observations_from_stereo_tracks -> window_ransac_host over both sides -> fit_cameras_host from the RANSAC poses on the
    RANSAC inliers -> both reprojection_errors_host; bundle=True: adjust_window_host from the fit's poses and the two means
    at its result. tracks=True adds ``xy_t`` and ``rows``."""
    xy_t, rows = T.stereo_track_window_host(disp_lr, disp_rl, flow_l, flow_r, xy0=xy0, th_ratio=th_ratio, th_abs=th_abs)
    keep = np.nonzero(~np.isnan(xy_t).any(axis=(1, 2)))[0]
    bsize = xy_t.shape[2]
    _check_ransac(len(keep), bsize, bundle, schedule, ba_schedule)
    xy = xy_t[keep]
    X = F.points_from_first_view(xy, cam, F.depth_from_disparity(xy, F._as_cam(cam)[0], baseline))
    left, right = F.observations_from_stereo_tracks(xy)
    off = _offset(offset, baseline)
    ran = R.window_ransac_host(X, np.stack([left, right]), cam, off, None, ntrials, thresh, seed)
    nan = np.full(bsize, np.nan)
    if ran["best_trial"] < 0:
        out = _ransac_result(len(keep), ran, _no_fit(bsize, schedule), nan, nan)
        if bundle:
            out.update(ba=None, err_left_ba=nan.copy(), err_right_ba=nan.copy())
    else:
        fit = F.fit_cameras_host(X, left, cam, mask=ran["words"], init=ran["G"], **schedule)
        err_l, _ = F.reprojection_errors_host(X, left, cam, fit["G"], mask=ran["words"])
        err_r, _ = F.reprojection_errors_host(X, right, cam, fit["G"], mask=ran["words"], offset=off)
        out = _ransac_result(len(keep), ran, fit, err_l, err_r)
        if bundle:
            ba = B.adjust_window_host(X, np.stack([left, right]), cam, offset=off, mask=ran["words"], init=fit["G"],
                                      **dict(ba_schedule or {}))
            err_l, _ = F.reprojection_errors_host(ba["X"], left, cam, ba["G"], mask=ran["words"])
            err_r, _ = F.reprojection_errors_host(ba["X"], right, cam, ba["G"], mask=ran["words"], offset=off)
            out.update(ba=ba, err_left_ba=err_l, err_right_ba=err_r)
    if tracks:
        out.update(xy_t=xy_t, rows=rows)
    return out


def ransac_cameras_from_window(win, cam, baseline, ntrials=100, thresh=2.0, seed=0, offset=None, bundle=False,
                               objects=None, ba_schedule=None, **schedule):
    """window_ransac_cameras_host from a StereoTrackWindow whose frames are all in (count() runs here if it has not), on
    the device and on the null stream: the RANSAC's points and both sides of its observations come from the window, its
    winner's words reach the fit (and the adjuster) on the device, its 12 bsize start poses cross the host. ``objects``: a
    dict that keeps the CameraRansac, the CameraFitter and the BundleAdjuster between calls of one M and bsize."""
    m = win.survivors if win.survivors is not None else win.count()
    bsize = win.bsize
    _check_ransac(m, bsize, bundle, schedule, ba_schedule)
    objects = {} if objects is None else objects
    if objects.get("ransac_key") != (m, bsize):
        objects.update(ransac_key=(m, bsize), ransac=R.CameraRansac(m, bsize, 2), ransac_fit=F.CameraFitter(m, bsize))
        objects.pop("ransac_ba", None)
    ran, fit = objects["ransac"], objects["ransac_fit"]
    off = _offset(offset, baseline)
    ran.set_camera(cam)
    ran.set_offset(off)
    ran.set_points_from_window(win, baseline)
    ran.set_observations_from_window(win)
    ran.set_mask(None)
    ran.run_async(ntrials, thresh, seed)
    r = ran.wait()
    nan = np.full(bsize, np.nan)
    if r["best_trial"] < 0:
        out = _ransac_result(m, r, _no_fit(bsize, schedule), nan, nan)
        if bundle:
            out.update(ba=None, err_left_ba=nan.copy(), err_right_ba=nan.copy())
        return out
    fit.set_camera(cam)
    fit.set_points_from_window(win, baseline)
    fit.set_observations_from_window(win, right=False)
    fit.set_mask_from_camransac(ran)
    fit.run_async(r["G"], **schedule)
    f = fit.wait()
    err_l, _ = fit.reprojection_errors(f["G"])
    fit.set_observations_from_window(win, right=True)
    err_r, _ = fit.reprojection_errors(f["G"], off)
    out = _ransac_result(m, r, f, err_l, err_r)
    if bundle:
        if "ransac_ba" not in objects:
            objects["ransac_ba"] = B.BundleAdjuster(m, bsize, 2)
        ba = objects["ransac_ba"]
        ba.set_camera(cam)
        ba.set_offset(off)
        ba.set_points_from_window(win, baseline)
        ba.set_observations_from_window(win)
        ba.set_mask_from_camransac(ran)
        ba.run_async(f["G"], **dict(ba_schedule or {}))
        res = ba.wait()
        fit.set_points(res["X"])
        fit.set_observations_from_window(win, right=False)
        err_l, _ = fit.reprojection_errors(res["G"])
        fit.set_observations_from_window(win, right=True)
        err_r, _ = fit.reprojection_errors(res["G"], off)
        out.update(ba=res, err_left_ba=err_l, err_right_ba=err_r)
    return out


def ransac_cameras(disp_lr, disp_rl, flow_l, flow_r, cam, baseline, xy0=None, th_ratio=0.2, th_abs=1.0, window=None,
                   tracks=False, ntrials=100, thresh=2.0, seed=0, offset=None, bundle=False, objects=None, ba_schedule=None,
                   **schedule):
    """window_ransac_cameras_host on the device, bit for bit: the fields of stereo_track_window in, the result out; see
    window_cameras for ``window`` and ``tracks``, ransac_cameras_from_window for ``objects``."""
    bsize = len(disp_lr)
    if bsize < 2 or bsize > R.MAX_FRAMES or len(disp_rl) != bsize:
        raise ValueError(f"disp_lr and disp_rl need one plane per frame, 2 .. {R.MAX_FRAMES} frames")
    if len(flow_l) < bsize - 1 or len(flow_r) < bsize - 1:
        raise ValueError("flow_l and flow_r need bsize - 1 (fwd, bwd) pairs")
    h, w = tuple(disp_lr[0].shape)
    win = window if window is not None else T.StereoTrackWindow(w, h, bsize, th_ratio, th_abs)
    win.open(T.field(disp_lr[0], -1), disp_rl[0], xy0)
    for fr in range(1, bsize):
        win.advance(flow_l[fr - 1][0], flow_l[fr - 1][1], flow_r[fr - 1][0], flow_r[fr - 1][1], T.field(disp_lr[fr], -1),
                    disp_rl[fr])
    win.count()
    out = ransac_cameras_from_window(win, cam, baseline, ntrials, thresh, seed, offset, bundle, objects, ba_schedule,
                                     **schedule)
    if tracks:
        xy_t, rows = win.read()
        out.update(xy_t=xy_t, rows=rows)
    return out
