"""Runs the small trackings of test_gpu_ref8_staged.py on the device and keeps what came back.

The chunk size of the 8x8 setup kernel is forced with ICTR_CPW, which the library reads when a batch is created and the
test must not put into its own environment, so the test starts this file as a fresh process per chunk size:

    ICTR_CPW=<cpw> python ref8_staged_child.py <cpw> <in.npz> <out.npz>

in.npz: img_a, img_b, fc, cc, wh, p_a, p_2 and the point sets pts_<name> (3, n) f64. Every problem is tracked from p_a
and then, without new points, from p_2 (points that leave the reference view keep their stale patches). For every last level lv_l in 2, 1, 0 (the
buffers then hold what that level's setup left), every form of the setup kernel's static groups and both batches (the
three ragged problems a, b, c in one; the one-point problem alone) out.npz holds, per problem,
    <form>/<lv_l>/<name>/T, Gx, Gy, coef, H (ProbState.H, 6x6), pose.
Forms: staged (the default: reference windows through the LDS tile where the level uses it), direct (ICTR_REF8_DIRECT_TAPS, bit 29),
planes (bit 27: the gradient planes, dynamic loop), image (staged, reference pyramid image-only, getgrad = 2).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

LV_F, PSZ, MAXITER = 2, 8, 3
BATCHES = (("a", "b", "c"), ("one",))


def run(inp):
    import invcompcamtrack_amd as ic
    pa, pb = ic.Pyramid(inp["img_a"], LV_F, PSZ), ic.Pyramid(inp["img_b"], LV_F, PSZ)
    pa_img = ic.Pyramid(inp["img_a"], LV_F, PSZ, getgrad=2)
    forms = (("staged", ic.VARIANT_LAUNCHES, pa), ("direct", ic.VARIANT_LAUNCHES | ic.REF8_DIRECT_TAPS, pa),
             ("planes", ic.VARIANT_LAUNCHES | ic.VARIANT_GRAD_PLANES, pa), ("image", ic.VARIANT_LAUNCHES, pa_img))
    cam = ic.CamClass(LV_F + 1, inp["fc"], inp["cc"], inp["wh"], PSZ)
    out = {}
    for names in BATCHES:
        sets = [np.ascontiguousarray(inp["pts_" + nm]) for nm in names]
        maxpt = max(s.shape[1] for s in sets)
        for lv_l in (2, 1, 0):
            op = ic.optparam(LV_F, lv_l, PSZ, MAXITER, 0.0, 0, 0, maxpt)
            for form, variant, ref in forms:
                e = ic.TrackBatch(cam, op, len(sets))
                e.set_variant(variant)
                for k, s in enumerate(sets):
                    e.Set3Dpoints(k, s.copy())
                for start in (inp["p_a"], inp["p_2"]):
                    for k in range(len(sets)):
                        e.SetPose(k, start, ref, pb)
                    e.track_async()
                    poses = e.poses()
                assert "k_level_resident" not in e.path_name() and "k_track1" not in e.path_name(), e.path_name()
                for k, (nm, s) in enumerate(zip(names, sets)):
                    n, key = s.shape[1], f"{form}/{lv_l}/{nm}/"
                    for w, q in ((0, "T"), (1, "Gx"), (2, "Gy")):
                        out[key + q] = e.read_buffer(k, w, 64 * n)
                    out[key + "coef"] = e.read_buffer(k, 7, 16 * n)
                    out[key + "H"] = e.read_buffer(k, 8, 54)[18:54].copy()
                    out[key + "pose"] = np.asarray(poses[k]).copy()
    return out


def main(argv):
    cpw, src, dst = int(argv[1]), argv[2], argv[3]
    if os.environ.get("ICTR_CPW") != str(cpw):
        raise SystemExit(f"ICTR_CPW must be {cpw}")
    np.savez(dst, **run(dict(np.load(src))))


if __name__ == "__main__":
    main(sys.argv)
