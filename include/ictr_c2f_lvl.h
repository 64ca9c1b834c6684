/* ictr_c2f_lvl.h -- a finest level above 0 for the coarse-to-fine dense flow, and the up-sampling that finishes such a run
 * (ictr_c2fflow.hip; DESIGN.md §4 "A finest level above 0"). Part of ictr.h, which includes it inside its extern "C" block;
 * not to be included alone. It is a file of its own because tests/test_c2fflow_cpu.py pins the list of ictr_c2fflow_*
 * declarations in ictr.h's own text; the ctypes table of these is _lib.SIGNATURES_LVL.
 *
 * The rule (patchflow.upsample_flow_host states it in f64): with s = 2^lv and a field F of level lv's size w_l x h_l, output
 * pixel (x, y) of the w x h frame takes fx = clamp((x + 0.5) / s - 0.5, 0, w_l - 1), x0 = floor(fx), x1 = min(x0 + 1,
 * w_l - 1), rx = fx - x0 (fy, y0, y1, ry alike with h_l) and, per component, top = (1 - rx) F[y0][x0] + rx F[y0][x1],
 * bot = (1 - rx) F[y1][x0] + rx F[y1][x1], val = (1 - ry) top + ry bot; the output is s val. The device takes the six
 * products and three sums in f32 in that order, each rounded. */
#ifndef ICTR_C2F_LVL_H
#define ICTR_C2F_LVL_H
/* ictr_c2fflow_create with a finest level lv_l (0 <= lv_l <= lv_f, refused otherwise): the runs search, densify and refine
 * the levels lv_f .. lv_l alone, and only those get a grid, a densifier, events, status and bias rows and a refiner; their
 * results are, bit for bit, those of the same levels of an object with lv_l = 0. With lv_l > 0 the object owns one
 * w x h x 2 result plane: a run ends with ONE launch of k_flow_upsample from level lv_l's field (the refiner's when the run
 * refined; with x_only set the y component is not read and is written as +0.0), and ictr_c2fflow_result and
 * ictr_c2fflow_device_ptr hand out that plane. The size rules of ictr_c2fflow_create hold for the levels lv_l .. lv_f;
 * ictr_c2fflow_level_dims, _read_level and _read_level_bias refuse a level below lv_l; ictr_c2fflow_get_kernel_ms keeps
 * its 3 (lv_f + 1) values, zeros below lv_l. lv_l = 0 is ictr_c2fflow_create. */
int ictr_c2fflow_create_lvl(ictr_c2fflow **out, int w, int h, int lv_f, int lv_l, int step, int psz);
int ictr_c2fflow_get_lv_l(const ictr_c2fflow *c, int *lv_l);
/* *ms of k_flow_upsample in the last run (waits for it); 0 when timing was off or lv_l = 0 */
int ictr_c2fflow_get_upsample_ms(ictr_c2fflow *c, float *ms);
/* The rule on a caller's field: src [h_l][w_l][2], out [h][w][2], 1 <= lv <= 15, and (w_l, h_l) must be the size of level lv
 * of a w x h pyramid (round-half-even halving), refused otherwise. x_only != 0: the y component of src is not read and the
 * y component of out is +0.0. on_device = 0: both are host arrays, staged by the call, which waits. on_device != 0: both are
 * device pointers and the kernel is enqueued on hip_stream (NULL: the null stream); the call does not wait. */
int ictr_flow_upsample(const float *src, int w_l, int h_l, int lv, float *out, int w, int h, int x_only, int on_device,
                       void *hip_stream);
#endif /* ICTR_C2F_LVL_H */
