"""Generates tests/golden/stereotrack_golden.npz by running the REFERENCE's misc_src/run_test_OF_track.py, lines 37-67
(func_get_transf_position) and 167-223 (the stereo track window), on synthetic fields.

Run in the build container only (needs /root/reference): python tests/golden/make_stereotrack_golden.py
The script is Python-2 era and reads a dataset at import, so it cannot be imported: the two line ranges are read at run
time and exec'd under Python 3 with xrange = range, an np.NaN alias and synthetic imgs_d, imgs_fl, imgs_fr, imwidth,
imheight and bsize in their namespace. Nothing of the script is edited or copied; the .npz holds data only: the seeded
input fields and the script's xy_t and its final idxvalid (``rows``).

The fields are float32-valued and mutually consistent up to second order in their gradients (a disparity plane D that the
left flow carries along, the right disparity and the backward flows by fixed-point inversion), so that a clean point passes
every test; sparse noise and rectangular defects in single fields then make single tests fail. The cases differ in the size
of the disparity and of the motion, because a ratio test fails alone only under a small displacement (error < th_abs but
>= th_ratio * displacement) and an absolute test only under a large one.
"""
import os
import sys

import numpy as np

REF = "/root/reference/misc_src/run_test_OF_track.py"
RANGES = ((37, 67), (167, 223))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stereotrack_golden.npz")

# name: H, W, bsize, seed, mean disparity, mean |motion| per frame, noise density, defect amplitude
CASES = {
    "small_disp": dict(h=24, w=40, bsize=4, seed=1, disp=2.2, move=1.2, noise=0.01, defect=0.55),
    "large_disp": dict(h=24, w=40, bsize=4, seed=2, disp=8.0, move=7.0, noise=0.01, defect=1.3),
    "odd_long": dict(h=33, w=47, bsize=6, seed=3, disp=3.0, move=1.5, noise=0.004, defect=0.7),
    "one_frame": dict(h=8, w=8, bsize=1, seed=4, disp=1.5, move=1.0, noise=0.05, defect=0.4),
    "two_frames": dict(h=24, w=40, bsize=2, seed=5, disp=6.5, move=6.0, noise=0.02, defect=1.2),
}


def reference_lines():
    with open(REF) as f:
        lines = f.readlines()
    return "".join("".join(lines[a - 1:b]) for a, b in RANGES)


def run_reference(code, imgs_d, imgs_fl, imgs_fr, w, h, bsize):
    if not hasattr(np, "NaN"):
        np.NaN = np.nan
    ns = dict(np=np, xrange=range, imgs_d=imgs_d, imgs_fl=imgs_fl, imgs_fr=imgs_fr, imwidth=w, imheight=h, bsize=bsize)
    with np.errstate(invalid="ignore", divide="ignore"):
        exec(compile(code, REF, "exec"), ns)
    return ns["xy_t"], ns["idxvalid"]


def invert(f, xx, yy, sign):
    """f at the fixed point q = p + sign * f(q) of every pixel p = (xx, yy), 30 rounds (|grad f| << 1)."""
    qx, qy = xx.copy(), yy.copy()
    for _ in range(30):
        u, v = f(qx, qy)
        qx, qy = xx + sign * u, yy + sign * v
    return f(qx, qy)


def make_fields(h, w, bsize, seed, disp, move, noise, defect):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = rng.uniform(0, 2 * np.pi, 8)
    ang = rng.uniform(0, 2 * np.pi, bsize)
    shift = np.concatenate([[np.zeros(2)], np.cumsum([[move * np.cos(a), 0.5 * move * np.sin(a)] for a in ang], 0)])

    def D(x, y):  # the disparity plane of frame 0, smooth and > 0
        return disp * (1 + 0.12 * np.sin(2 * np.pi * x / (2.0 * w) + ph[0]) * np.cos(2 * np.pi * y / (2.0 * h) + ph[1]))

    def flow(fr):  # left flow fr -> fr + 1: a translation plus a gentle wave
        tx, ty = move * np.cos(ang[fr]), 0.5 * move * np.sin(ang[fr])

        def f(x, y):
            s = 0.15 * np.sin(2 * np.pi * x / (1.5 * w) + ph[2] + fr) * np.cos(2 * np.pi * y / (1.5 * h) + ph[3])
            return tx + s, ty + 0.5 * s
        return f

    imgs_d, imgs_fl, imgs_fr = [], [], []
    for fr in range(bsize):
        sx, sy = shift[fr]

        def d_lr(x, y, sx=sx, sy=sy):
            return D(x - sx, y - sy), np.zeros_like(x)
        lr = d_lr(xx, yy)[0]
        rl = invert(d_lr, xx, yy, +1.0)[0]  # rl(x') = d(x) with x = x' + d(x)
        fl = flow(fr)
        ff = np.stack(fl(xx, yy), 2)
        fb = -np.stack(invert(fl, xx, yy, -1.0), 2)  # b(p) = -f(q) with q = p - f(q)
        # the right flow moves a right pixel as the left flow moves its left match
        gf = np.stack(fl(xx + rl, yy), 2)

        def fr_fun(x, y, fl=fl, d_lr=d_lr):
            return fl(x + invert(d_lr, x, y, +1.0)[0], y)
        gb = -np.stack(invert(fr_fun, xx, yy, -1.0), 2)
        fields = [lr, rl, ff, fb, gf, gb]
        # sparse noise, one field at a time, and one rectangular defect per field
        for k, a in enumerate(fields):
            hit = rng.uniform(size=(h, w)) < noise
            amp = rng.choice([0.3, 0.6, 1.5, 3.0], size=(h, w)) * rng.choice([-1.0, 1.0], size=(h, w))
            y0, x0 = rng.integers(1, max(2, h - 5)), rng.integers(1, max(2, w - 6))
            box = np.zeros((h, w), bool)
            box[y0:y0 + 3, x0:x0 + 4] = True
            add = np.where(hit, amp, 0.0) + np.where(box, defect, 0.0)
            if a.ndim == 3:
                a[:, :, 0] += add
            else:
                a += add
        lr, rl, ff, fb, gf, gb = [a.astype(np.float32) for a in fields]
        imgs_d.append((lr, rl))
        imgs_fl.append((ff, fb))
        imgs_fr.append((gf, gb))
    return imgs_d, imgs_fl, imgs_fr


def main():
    code = reference_lines()
    out = {"cases": np.array(sorted(CASES))}
    for name in sorted(CASES):
        c = CASES[name]
        imgs_d, imgs_fl, imgs_fr = make_fields(**c)
        as64 = lambda seq: [tuple(a.astype(float) for a in t) for t in seq]  # noqa: E731  (the script's .astype(float))
        xy_t, rows = run_reference(code, as64(imgs_d), as64(imgs_fl), as64(imgs_fr), c["w"], c["h"], c["bsize"])
        assert not np.isnan(xy_t).any()
        out[name + "_disp_lr"] = np.stack([d[0] for d in imgs_d])
        out[name + "_disp_rl"] = np.stack([d[1] for d in imgs_d])
        out[name + "_flow_l"] = np.stack([np.stack(f) for f in imgs_fl])  # (bsize, 2 = fwd / bwd, H, W, 2)
        out[name + "_flow_r"] = np.stack([np.stack(f) for f in imgs_fr])
        out[name + "_xy_t"] = xy_t
        out[name + "_rows"] = rows.astype(np.int64)
        print(name, "kept", len(rows), "of", c["w"] * c["h"])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    sys.exit(main())
