// ictr_c2fset.hip -- the lockstep twins of the coarse-to-fine flow's own kernels (DESIGN.md §4 "Lockstep sets"): the L2 forms
// of k_c2f_level_set (ictr_c2fflow_dev.h) and k_flow_upsample_set. A twin runs its kernel's body (c2f_level_body,
// flow_upsample_body) on item m of a per-member argument block, m the block index along the grid dimension the kernel does
// not use: a member's workgroups are the workgroups of its own launch, and no workgroup reads another member's buffers.
// They are instantiated here, in a module of their own, so that the kernels of ictr_c2fflow.hip keep their code to the
// instruction. The set object and its run are in ictr_c2fflow.hip, next to the object they drive.
#include "ictr_c2fflow_dev.h"

namespace ictr {

template <bool XONLY>
__global__ __launch_bounds__(kBlock) void k_flow_upsample_set(UpSetArgs a, int wl, int hl, float inv_s, float s, int w, int h) {
  flow_upsample_body<XONLY>(a.src[blockIdx.z], wl, hl, inv_s, s, a.out[blockIdx.z], w, h);
}

void launch_flow_upsample_set(const UpSetArgs &a, int n, int wl, int hl, int lv, int w, int h, int x_only, hipStream_t s) {
  const float sc = (float)(1 << lv), inv = 1.0f / sc;
  dim3 g = pixel_rows_grid(w, h);
  g.z = n;
  if (x_only)
    hipLaunchKernelGGL((k_flow_upsample_set<true>), g, dim3(kBlock), 0, s, a, wl, hl, inv, sc, w, h);
  else
    hipLaunchKernelGGL((k_flow_upsample_set<false>), g, dim3(kBlock), 0, s, a, wl, hl, inv, sc, w, h);
}

template <bool MEAN, int NCH>
static void launch_set(const SetArgs<C2fArgs<MEAN, NCH>> &a, int n, int x_only, hipStream_t s) {
  if (x_only)
    launch_c2f_level_set<MEAN, true, NCH, false>(a, n, s);
  else
    launch_c2f_level_set<MEAN, false, NCH, false>(a, n, s);
}
void launch_c2f_level_set(const SetArgs<C2fArgs<false, 1>> &a, int n, int x_only, hipStream_t s) { launch_set(a, n, x_only, s); }
void launch_c2f_level_set(const SetArgs<C2fArgs<false, 3>> &a, int n, int x_only, hipStream_t s) { launch_set(a, n, x_only, s); }
void launch_c2f_level_set(const SetArgs<C2fArgs<true, 1>> &a, int n, int x_only, hipStream_t s) { launch_set(a, n, x_only, s); }
void launch_c2f_level_set(const SetArgs<C2fArgs<true, 3>> &a, int n, int x_only, hipStream_t s) { launch_set(a, n, x_only, s); }

}  // namespace ictr
