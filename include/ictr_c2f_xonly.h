/* ictr_c2f_xonly.h -- the 1-D (x only) form of the coarse-to-fine dense flow, for rectified stereo pairs
 * (ictr_c2fflow.hip; DESIGN.md §4 "The 1-D form"). Part of ictr.h, which includes it inside its extern "C" block; not to be
 * included alone. It is a file of its own because tests/test_c2fflow_cpu.py pins the list of ictr_c2fflow_* declarations
 * in ictr.h's own text; the ctypes table of these two is _lib.SIGNATURES_XONLY. */
#ifndef ICTR_C2F_XONLY_H
#define ICTR_C2F_XONLY_H
/* on != 0: the next runs search along x only. A node starts from the x component of the coarser field alone, the search is
 * k_patchdisp's rule at the level (hxx and hyy; held by conditioning iff !(tr > 0) or !(hxx > 1e-2 tr); p += bx / hxx),
 * the rejection is (p - init)^2 > psz^2, the refinement (when on) moves u alone, and the y component of every node and of
 * every level's field is +0.0 to the bit. It combines with patch-mean normalisation. Default off: the runs are then, bit
 * for bit, those of an object that never had this call. */
int ictr_c2fflow_set_x_only(ictr_c2fflow *c, int on);
int ictr_c2fflow_get_x_only(const ictr_c2fflow *c, int *on);
#endif /* ICTR_C2F_XONLY_H */
