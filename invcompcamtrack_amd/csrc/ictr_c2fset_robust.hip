// ictr_c2fset_robust.hip -- the ROBUST forms of k_c2f_level_set (ictr_c2fflow_dev.h): the lockstep twins of the kernels of
// ictr_c2fflow_robust.hip (DESIGN.md §4 "Lockstep sets"), in a module of their own as those are.
#include "ictr_c2fflow_dev.h"

namespace ictr {

template <bool MEAN, int NCH>
static void launch_set_robust(const SetArgs<C2fArgsRobust<MEAN, NCH>> &a, int n, int x_only, hipStream_t s) {
  if (x_only)
    launch_c2f_level_set<MEAN, true, NCH, true>(a, n, s);
  else
    launch_c2f_level_set<MEAN, false, NCH, true>(a, n, s);
}
void launch_c2f_level_set(const SetArgs<C2fArgsRobust<false, 1>> &a, int n, int x_only, hipStream_t s) {
  launch_set_robust(a, n, x_only, s);
}
void launch_c2f_level_set(const SetArgs<C2fArgsRobust<false, 3>> &a, int n, int x_only, hipStream_t s) {
  launch_set_robust(a, n, x_only, s);
}
void launch_c2f_level_set(const SetArgs<C2fArgsRobust<true, 1>> &a, int n, int x_only, hipStream_t s) {
  launch_set_robust(a, n, x_only, s);
}
void launch_c2f_level_set(const SetArgs<C2fArgsRobust<true, 3>> &a, int n, int x_only, hipStream_t s) {
  launch_set_robust(a, n, x_only, s);
}

}  // namespace ictr
