// ictr_c2fflow_robust.hip -- the ROBUST forms of k_c2f_level (ictr_c2fflow_dev.h): the coarse-to-fine flow's search with
// the Huber patch cost (DESIGN.md §4 "Robust patch cost"), every residual clipped to [-huber_k, +huber_k]. They are
// instantiated here, in a module of their own, so that the L2 forms of ictr_c2fflow.hip keep their code to the
// instruction. Restated in NumPy f32 by tests/c2fcost_f32.py; the definition is patchflow.c2f_flow_host(cost="huber").
#include "ictr_c2fflow_dev.h"

namespace ictr {

template void launch_c2f_level<false, 1, true>(const SetArgs<C2fArgsRobust<false, 1>> &, int, int, hipStream_t);
template void launch_c2f_level<false, 3, true>(const SetArgs<C2fArgsRobust<false, 3>> &, int, int, hipStream_t);
template void launch_c2f_level<true, 1, true>(const SetArgs<C2fArgsRobust<true, 1>> &, int, int, hipStream_t);
template void launch_c2f_level<true, 3, true>(const SetArgs<C2fArgsRobust<true, 3>> &, int, int, hipStream_t);

}  // namespace ictr
