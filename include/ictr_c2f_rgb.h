/* ictr_c2f_rgb.h -- colour (three-channel) frames for the coarse-to-fine dense flow (ictr_c2fflow.hip; DESIGN.md §4
 * "Colour"). Part of ictr.h, which includes it inside its extern "C" block; not to be included alone. It is a file of its
 * own because tests/test_c2fflow_cpu.py pins the list of ictr_c2fflow_* declarations in ictr.h's own text; the ctypes table
 * of these is _lib.SIGNATURES_RGB.
 *
 * A colour frame is THREE pyramids, one per channel, built by ictr_pyramid_create as any other and equal in size, levels
 * and padding. The rule (patchflow.c2f_flow_host on triples states it in f64): the nodes, the starts, the view tests, the
 * stop, the rejection, the status values, the fill and the up-sampling are those of one channel; the search sums
 * H = sum_c sum_px G_c G_c^T and b = sum_c sum_px G_c (T_c - I_c) and takes one conditioning decision and one step per
 * node; with patnorm every channel loses its own patch mean and a node has one brightness offset per channel; a
 * densifier's vote weighs the channel mean e = (1/3) sum_c |Bw_c - A_c - beta_c|; the refinement warps and differentiates
 * per channel, takes its two robust weights jointly over the channels on the channel mean,
 * q0 = delta inside / 2 / sqrt((1/3) sum_c n0_c Iz_c^2 + eps^2) and qg likewise, and its coefficients as channel means.
 * Three equal channels give the grey rule in real arithmetic. The number of channels is 1 or 3. */
#ifndef ICTR_C2F_RGB_H
#define ICTR_C2F_RGB_H
/* n = 1 (the object as created) or 3; anything else is refused. To be called before the first run (refused after one): it
 * sizes the node bias block, [ny][nx][n] floats per level; if that allocation fails the object keeps its channel count.
 * (The refinement's two more warp planes are made by the first refined run of a 3-channel object.) */
int ictr_c2fflow_set_channels(ictr_c2fflow *c, int n);
int ictr_c2fflow_get_channels(const ictr_c2fflow *c, int *n);
/* ictr_c2fflow_run of a 3-channel object: pyr_a[ch], pyr_b[ch] are channel ch of frames A and B. Refused with a message:
 * on a 1-channel object (and ictr_c2fflow_run on a 3-channel one), and when the three pyramids of a frame differ in
 * geometry (size, levels' strides or padding). Every other check is ictr_c2fflow_run's, per channel. The result plane, the
 * levels' fields, node displacements and status bytes are read as after ictr_c2fflow_run. */
int ictr_c2fflow_run_rgb(ictr_c2fflow *c, const ictr_pyramid *const pyr_a[3], const ictr_pyramid *const pyr_b[3],
                         void *hip_stream);
/* of the last run, which had patnorm on, of a 3-channel object (waits for it): the node bias [ny][nx][3] of a level;
 * ictr_c2fflow_read_level_bias refuses such an object */
int ictr_c2fflow_read_level_bias_rgb(ictr_c2fflow *c, int level, float *bias);
#endif /* ICTR_C2F_RGB_H */
