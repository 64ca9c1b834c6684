/* ictr_c2f_patnorm.h -- patch-mean normalisation of the coarse-to-fine dense flow (ictr_c2fflow.hip; DESIGN.md §4
 * "Patch-mean normalisation"). Part of ictr.h, which includes it inside its extern "C" block; not to be included alone.
 * It is a file of its own because tests/test_c2fflow_cpu.py pins the list of ictr_c2fflow_* declarations in ictr.h's own
 * text; the ctypes table of these two is _lib.SIGNATURES_PATNORM. */
#ifndef ICTR_C2F_PATNORM_H
#define ICTR_C2F_PATNORM_H
/* on != 0: patch-mean normalisation for the next runs, for frames whose brightness differs by a locally constant offset
 * (the two cameras of a rig, auto-exposure). The search removes the mean of the template and of every frame window;
 * every node that votes from inside the view gets its brightness offset beta = mean(B at its final position) -
 * mean(A at the node), any other node +0.0; a node's vote in the densification weighs |Bw - A - beta|. The refinement is
 * unchanged: its brightness term still sees the offset. Default off: the runs are then, bit for bit and kernel for
 * kernel, those of an object that never had this call. */
int ictr_c2fflow_set_patnorm(ictr_c2fflow *c, int on);
/* of the last run (waits for it), which had patnorm on (refused otherwise): the level's node bias [ny][nx] */
int ictr_c2fflow_read_level_bias(ictr_c2fflow *c, int level, float *bias);
#endif /* ICTR_C2F_PATNORM_H */
