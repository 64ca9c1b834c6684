"""A plain-loop restatement of the stereo track window (misc_src/run_test_OF_track.py:170-223): one point at a time, Python
floats, no array operation. It judges invcompcamtrack_amd.stereotrack.stereo_track_window_host at the edges in
tests/test_stereotrack_cpu.py. Python's float arithmetic, math.sqrt and / are the correctly rounded f64 operations."""
import math

import numpy as np

NAN = float("nan")


def gather(x, y, du, dv=None):
    """func_get_transf_position for one point; du, dv: 2-D float64 arrays (dv None: x only)."""
    h, w = du.shape
    if math.isnan(x) or math.isnan(y) or math.isinf(x) or math.isinf(y):
        return NAN, NAN
    x0, y0 = math.floor(x), math.floor(y)
    x1, y1 = x0 + 1, y0 + 1
    if x0 < 0 or x1 < 0 or y0 < 0 or y1 < 0 or x0 >= w or x1 >= w or y0 >= h or y1 >= h:
        return NAN, NAN
    fx, fy = x - x0, y - y0
    w0, w1, w2, w3 = fx * fy, (1 - fx) * fy, fx * (1 - fy), (1 - fx) * (1 - fy)

    def blend(d):
        return float(d[y1, x1]) * w0 + float(d[y1, x0]) * w1 + float(d[y0, x1]) * w2 + float(d[y0, x0]) * w3
    return x + blend(du), (y if dv is None else y + blend(dv))


def norm(ax, ay, bx, by):
    dx, dy = ax - bx, ay - by
    return math.sqrt(dx * dx + dy * dy)


def less(num, den, bound):
    """num / den < bound with NumPy's rules: x / 0 is inf or NaN and NaN compares false."""
    if math.isnan(num) or math.isnan(den):
        return False
    if den == 0.0:
        return False  # +inf or NaN, neither below a finite bound (and inf < inf is false)
    return num / den < bound


def window(disp_lr, disp_rl, flow_l, flow_r, xy0=None, th_ratio=0.2, th_abs=1.0):
    bsize = len(disp_lr)
    d = lambda a: np.asarray(a, np.float64)  # noqa: E731
    h, w = d(disp_lr[0]).shape
    if xy0 is None:
        xy0 = [(float(x), float(y)) for y in range(h) for x in range(w)]
    rows, out = [], []
    for i, (xl, yl) in enumerate(xy0):
        xl, yl = float(xl), float(yl)
        xr, yr = gather(xl, yl, -d(disp_lr[0]))
        xb, yb = gather(xr, yr, d(disp_rl[0]))
        err = norm(xl, yl, xb, yb)
        if not (less(err, norm(xr, yr, xl, yl), th_ratio) and err < th_abs):
            continue
        row = [[xl], [yl], [xr], [yr]]
        ok = True
        for fr in range(1, bsize):
            lf, lb, rf, rb = d(flow_l[fr - 1][0]), d(flow_l[fr - 1][1]), d(flow_r[fr - 1][0]), d(flow_r[fr - 1][1])
            xlf, ylf = gather(xl, yl, lf[:, :, 0], lf[:, :, 1])
            xrf, yrf = gather(xr, yr, rf[:, :, 0], rf[:, :, 1])
            xrd, yrd = gather(xlf, ylf, -d(disp_lr[fr]))
            xld, yld = gather(xrf, yrf, d(disp_rl[fr]))
            xlv, ylv = gather(xlf, ylf, lb[:, :, 0], lb[:, :, 1])
            xrv, yrv = gather(xrf, yrf, rb[:, :, 0], rb[:, :, 1])
            e1, e2 = norm(xrf, yrf, xrd, yrd), norm(xlf, ylf, xld, yld)
            e3, e4 = norm(xl, yl, xlv, ylv), norm(xr, yr, xrv, yrv)
            d12, d3, d4 = norm(xrf, yrf, xlf, ylf), norm(xl, yl, xlf, ylf), norm(xr, yr, xrf, yrf)
            ok = (less(e1, d12, th_ratio) and less(e2, d12, th_ratio) and less(e3, d3, th_ratio) and less(e4, d4, th_ratio)
                  and e1 < th_abs and e2 < th_abs and e3 < th_abs and e4 < th_abs)
            if not ok:
                break
            xl, yl, xr, yr = xlf, ylf, xrf, yrf
            for c, v in enumerate((xl, yl, xr, yr)):
                row[c].append(v)
        if ok:
            rows.append(i)
            out.append(row)
    return np.array(out, np.float64).reshape(len(rows), 4, bsize), np.array(rows, np.int64)
