// ictr_c2fflow_dev.h -- k_c2f_level, the per-level search kernel of the coarse-to-fine dense flow, with its arguments and
// its launcher, for the two files that instantiate it: ictr_c2fflow.hip the L2 forms, ictr_c2fflow_robust.hip the ROBUST
// forms (the Huber patch cost, DESIGN.md "Robust patch cost"), in a module of their own because more kernels in one module
// move the compiler's schedule of some of the two-wave forms by an instruction or two. The forms are described at the head
// of ictr_c2fflow.hip.
// The kernel runs on 1 .. kSetMax coarse-to-fine flows of one shape at once (DESIGN.md "Lockstep sets"): its argument is
// a SetArgs block, the arguments of one flow per member, and a workgroup runs c2f_level_body on member blockIdx.y's. A
// single object's run is a set of one.
#pragma once

#include <type_traits>

#include "ictr_dev.h"
#include "ictr_launch.h"
#include "ictr_devfn.h"
#include "ictr_patchflow_dev.h"

namespace ictr {

// The plain forms' arguments ...
template <bool MEAN, int NCH>
struct C2fArgs {
  const float *a[NCH], *ax[NCH], *ay[NCH], *b[NCH];  // this level, per channel: frame A image + gradients, frame B image
                                                     // (padded planes of one geometry)
  int sw, shift;                 // row stride; (pad - P) * (sw + 1), as PFLevel
  float swo, sho;                // the level's unpadded size
  int nx, K, step;               // nodes per row, nodes, node spacing
  const float2 *coarse;          // the coarser level's dense field [ch][cw], NULL at the coarsest level
  int cw, ch;
  int P, maxiter;
  float eps2, min_det, far2;     // stop when |dp|^2 < eps2; conditioning (XONLY: min_hx); (float)(P * P)
  float *d;                      // [K][2] raw node displacements (the fill's input)
  unsigned char *lost, *status;  // [K], [K]
};
// ... and behind them bias for the MEAN forms alone (the plain forms keep their arguments, and with them their code, to
// the instruction)
template <int NCH>
struct C2fArgs<true, NCH> : C2fArgs<false, NCH> {
  float *bias;  // [K][NCH] node brightness offsets per channel
};

// ... and behind all of them huber_k for the ROBUST forms alone (DESIGN.md "Robust patch cost"), in the same way
template <bool MEAN, int NCH>
struct C2fArgsRobust : C2fArgs<MEAN, NCH> {
  float huber_k;  // the clip of a residual, in grey levels
};
template <bool MEAN, int NCH, bool ROBUST>
using C2fArgsOf = std::conditional_t<ROBUST, C2fArgsRobust<MEAN, NCH>, C2fArgs<MEAN, NCH>>;

// channel c's planes of a level
template <bool MEAN, int NCH>
__device__ __forceinline__ PFPlanes c2f_planes(const C2fArgs<MEAN, NCH> &a, int c) {
  return PFPlanes{(gconst_f32)a.a[c], (gconst_f32)a.ax[c], (gconst_f32)a.ay[c], (gconst_f32)a.b[c],
                  a.sw,               a.shift,             a.swo,               a.sho};
}

// NCH = 3 is the colour form (DESIGN.md "Colour"): pf_level_search_ch over three channel planes, one decision and one
// step per node, and with MEAN three betas per node, bias[k][c]. A reduction's row of sSum is then 8 floats wide: the
// widest (H with three sums of T) carries six values in one trip. Restated by tests/c2frgb_f32.py.
// ROBUST is the Huber patch cost: pf_level_search_ch's ROBUST forms with a.huber_k; the start, the hold rules, the MEAN
// tail and what is written are unchanged. Restated by tests/c2fcost_f32.py.
// The body of k_c2f_level (below) for one member, whose arguments it takes by value.
template <int NPL, int WPP, bool MEAN, bool XONLY, int NCH, bool ROBUST>
__device__ __forceinline__ void c2f_level_body(C2fArgsOf<MEAN, NCH, ROBUST> a) {
  static_assert(NCH == 1 || NCH == 3, "one channel or three");
  constexpr int PPB = kWaves / WPP;  // nodes per workgroup
  constexpr int SW = NCH == 1 ? 4 : 8;
  __shared__ float sSum[WPP > 1 ? kWaves : 1][SW];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int k = blockIdx.x * PPB + wave / WPP;
  const bool valid = k < a.K;
  if (WPP == 1 && !valid) return;
  const int kk = valid ? k : 0;
  const int nj = kk / a.nx, ni = kk - nj * a.nx;
  const int X = a.step / 2 + ni * a.step, Y = a.step / 2 + nj * a.step;  // inside the level: the template needs no test
  const float xl = (float)X, yl = (float)Y;
  float ix = 0.0f, iy = 0.0f;
  if (a.coarse) {
    if constexpr (XONLY) {  // y is not read and stays +0.0
      ix = 2.0f * a.coarse[(size_t)min(Y >> 1, a.ch - 1) * a.cw + min(X >> 1, a.cw - 1)].x;
    } else {
      const float2 c = a.coarse[(size_t)min(Y >> 1, a.ch - 1) * a.cw + min(X >> 1, a.cw - 1)];
      ix = 2.0f * c.x;
      iy = 2.0f * c.y;
    }
  }
  const bool finite = (fabsf(ix) <= 3.402823466e+38f) & (fabsf(iy) <= 3.402823466e+38f);  // false for NaN
  int st = (valid && finite && pf_in_view(xl + ix, yl + iy, a.swo, a.sho)) ? ICTR_C2F_TRACKED : ICTR_C2F_LOST;
  float px = ix, py = iy;
  float mean_t[NCH] = {};
  // (formed once, ahead of both uses: the grey forms then report the registers they had with one set of planes per use)
  PFPlanes L[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) L[c] = c2f_planes<MEAN, NCH>(a, c);
  // One wave per node with a start out of view is done; two waves per node share the search's barriers.
  if (WPP > 1 || st == ICTR_C2F_TRACKED) {
    int nit = 0;
    int why;
    if constexpr (ROBUST)
      why = pf_level_search_ch<NPL, WPP, XONLY, MEAN, NCH, SW, true>(L, a.P, xl, yl, st == ICTR_C2F_TRACKED, px, py, nit,
                                                                     a.maxiter, a.eps2, a.min_det, sSum, mean_t, a.huber_k);
    else
      why = pf_level_search_ch<NPL, WPP, XONLY, MEAN, NCH, SW>(L, a.P, xl, yl, st == ICTR_C2F_TRACKED, px, py, nit,
                                                               a.maxiter, a.eps2, a.min_det, sSum, mean_t);
    if (why) st = why == PF_STOP_COND ? ICTR_C2F_HELD_COND : ICTR_C2F_HELD_VIEW;
    if (st == ICTR_C2F_TRACKED) {  // a runaway patch: further than P from its start, or not finite (a positive test)
      const float dx = px - ix, dy = py - iy;
      if constexpr (XONLY) {
        if (!(dx * dx <= a.far2)) st = ICTR_C2F_HELD_FAR;
      } else {
        if (!(dx * dx + dy * dy <= a.far2)) st = ICTR_C2F_HELD_FAR;
      }
    }
  }
  float beta[NCH] = {};
  if constexpr (MEAN) {
    // the node's final position: where it votes from. Two waves per node: every node of the workgroup makes the pass.
    const bool held = st >= ICTR_C2F_HELD_COND;
    const float fx = xl + (held ? ix : px), fy = yl + (held ? iy : py);
    const bool votes = valid && st != ICTR_C2F_LOST && pf_in_view(fx, fy, a.swo, a.sho);
    if (WPP > 1 || votes) {
      float sb[NCH];
      pf_window_sum_ch<NPL, WPP, NCH, SW>(L, a.P, votes ? fx : 1.0f, votes ? fy : 1.0f, sSum, sb);
      if (votes) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) beta[c] = sb[c] / (float)(a.P * a.P) - mean_t[c];
      }
    }
  }
  if (lane == 0 && wave % WPP == 0 && valid) {
    const float nanv = __int_as_float(0x7fc00000);
    const bool held = st >= ICTR_C2F_HELD_COND;
    a.d[2 * k] = st == ICTR_C2F_LOST ? nanv : held ? ix : px;  // a held node: its start's bits
    a.d[2 * k + 1] = st == ICTR_C2F_LOST ? nanv : held ? iy : py;
    a.lost[k] = st == ICTR_C2F_LOST ? 1 : 0;
    a.status[k] = (unsigned char)st;
    if constexpr (MEAN) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) a.bias[NCH * k + c] = beta[c];
    }
  }
}

// a member's workgroups along x, the members along y
template <int NPL, int WPP, bool MEAN, bool XONLY, int NCH = 1, bool ROBUST = false>
__global__ __launch_bounds__(kBlock) void k_c2f_level(SetArgs<C2fArgsOf<MEAN, NCH, ROBUST>> s) {
  static_assert(sizeof(s) <= kKernargLimit, "the argument block of a set exceeds the kernel-argument limit");
  c2f_level_body<NPL, WPP, MEAN, XONLY, NCH, ROBUST>(s.m[blockIdx.y]);
}

// The search of n members (1 .. kSetMax, of one shape: member 0's stands for all). The form follows from the patch size
// alone, as launch_patchdisp's: up to 4 pixels per lane one wave per node, above two; x_only selects the XONLY forms.
template <bool MEAN, bool XONLY, int NCH, bool ROBUST>
inline void launch_c2f_level_form(const SetArgs<C2fArgsOf<MEAN, NCH, ROBUST>> &a, int n, hipStream_t s) {
  const int npl = (a.m[0].P * a.m[0].P + 63) / 64, K = a.m[0].K;
  const dim3 blk(kBlock);
  if (npl > 4) {
    hipLaunchKernelGGL((k_c2f_level<8, 2, MEAN, XONLY, NCH, ROBUST>), dim3((K + kWaves / 2 - 1) / (kWaves / 2), n), blk, 0, s,
                       a);
    return;
  }
  const dim3 g((K + kWaves - 1) / kWaves, n);
  if (npl <= 1)
    hipLaunchKernelGGL((k_c2f_level<1, 1, MEAN, XONLY, NCH, ROBUST>), g, blk, 0, s, a);
  else
    hipLaunchKernelGGL((k_c2f_level<4, 1, MEAN, XONLY, NCH, ROBUST>), g, blk, 0, s, a);
}
template <bool MEAN, int NCH, bool ROBUST>
void launch_c2f_level(const SetArgs<C2fArgsOf<MEAN, NCH, ROBUST>> &a, int n, int x_only, hipStream_t s) {
  if (x_only)
    launch_c2f_level_form<MEAN, true, NCH, ROBUST>(a, n, s);
  else
    launch_c2f_level_form<MEAN, false, NCH, ROBUST>(a, n, s);
}
// the ROBUST forms are instantiated in ictr_c2fflow_robust.hip alone
extern template void launch_c2f_level<false, 1, true>(const SetArgs<C2fArgsRobust<false, 1>> &, int, int, hipStream_t);
extern template void launch_c2f_level<false, 3, true>(const SetArgs<C2fArgsRobust<false, 3>> &, int, int, hipStream_t);
extern template void launch_c2f_level<true, 1, true>(const SetArgs<C2fArgsRobust<true, 1>> &, int, int, hipStream_t);
extern template void launch_c2f_level<true, 3, true>(const SetArgs<C2fArgsRobust<true, 3>> &, int, int, hipStream_t);

}  // namespace ictr
