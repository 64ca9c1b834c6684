// ictr_c2fflow_robust.hip -- the ROBUST forms of k_c2f_level (ictr_c2fflow_dev.h): the coarse-to-fine flow's search with
// the Huber patch cost (DESIGN.md §4 "Robust patch cost"), every residual clipped to [-huber_k, +huber_k]. They are
// instantiated here, in a module of their own, so that the L2 forms of ictr_c2fflow.hip keep their code to the
// instruction. Restated in NumPy f32 by tests/c2fcost_f32.py; the definition is patchflow.c2f_flow_host(cost="huber").
#include "ictr_c2fflow_dev.h"

namespace ictr {

template <bool MEAN, int NCH>
static void launch_robust(const C2fArgsRobust<MEAN, NCH> &a, int x_only, hipStream_t s) {
  if (x_only)
    launch_c2f_level<MEAN, true, NCH, true>(a, s);
  else
    launch_c2f_level<MEAN, false, NCH, true>(a, s);
}
void launch_c2f_level_robust(const C2fArgsRobust<false, 1> &a, int x_only, hipStream_t s) { launch_robust(a, x_only, s); }
void launch_c2f_level_robust(const C2fArgsRobust<false, 3> &a, int x_only, hipStream_t s) { launch_robust(a, x_only, s); }
void launch_c2f_level_robust(const C2fArgsRobust<true, 1> &a, int x_only, hipStream_t s) { launch_robust(a, x_only, s); }
void launch_c2f_level_robust(const C2fArgsRobust<true, 3> &a, int x_only, hipStream_t s) { launch_robust(a, x_only, s); }

}  // namespace ictr
