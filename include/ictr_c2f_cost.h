/* ictr_c2f_cost.h -- the patch cost of the coarse-to-fine dense flow's search (ictr_c2fflow.hip, ictr_c2fflow_robust.hip;
 * DESIGN.md §4 "Robust patch cost"). Part of ictr.h, which includes it inside its extern "C" block; not to be included
 * alone. It is a file of its own because tests/test_c2fflow_cpu.py pins the list of ictr_c2fflow_* declarations in ictr.h's
 * own text; the ctypes table of these is _lib.SIGNATURES_COST. */
#ifndef ICTR_C2F_COST_H
#define ICTR_C2F_COST_H
/* The patch cost of the search, numbered as the cost field of OF_DIS's parameter
 * string is remembered (0 L2, 1 L1, 2 Huber). L2 is the object as created. Huber: every pixel's and channel's residual of
 * every iteration is clipped to [-huber_k, +huber_k] (grey levels on the frames' own scale), after the patch means are
 * removed under patnorm; T, Gx, Gy, H, the conditioning decision, the view tests, the step H^-1 sum G r, the eps stop, the
 * rejection, the status values, the node bias, the densifier and the refinement are unchanged
 * (patchflow.c2f_flow_host(cost="huber") states it). Refused with a message, the object unchanged: cost 1 (L1 is not built:
 * with H fixed its influence sign(r) has no scale; Huber with a small huber_k is its scaled form), any other unknown code,
 * and a huber_k that is NaN, infinite, zero or negative (checked for both costs). It combines with patnorm, x_only, lv_l,
 * channels and the refinement, and may be changed between runs. */
enum { ICTR_C2F_COST_L2 = 0, ICTR_C2F_COST_HUBER = 2 };
int ictr_c2fflow_set_cost(ictr_c2fflow *c, int cost, float huber_k);
int ictr_c2fflow_get_cost(const ictr_c2fflow *c, int *cost, float *huber_k);
#endif /* ICTR_C2F_COST_H */
