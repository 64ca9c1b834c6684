// ictr_c2fflow_dev.h -- k_c2f_level, the per-level search kernel of the coarse-to-fine dense flow, with its arguments and
// its launcher, for the two files that instantiate it: ictr_c2fflow.hip the L2 forms (which keeps that file's device code
// what it was before the ROBUST forms existed, to the instruction: more kernels in one module move the compiler's
// schedule of three of the two-wave forms by an instruction or two), ictr_c2fflow_robust.hip the ROBUST forms (the Huber
// patch cost, DESIGN.md "Robust patch cost"). The forms are described at the head of ictr_c2fflow.hip.
// The kernel's body is c2f_level_body, which the lockstep twin k_c2f_level_set runs per member of a set of coarse-to-fine
// flows (DESIGN.md "Lockstep sets"); its forms are instantiated in ictr_c2fset.hip (L2) and ictr_c2fset_robust.hip
// (ROBUST). k_flow_upsample's body is here for the same reason.
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
// The body is stated once, for k_c2f_level and for its lockstep twin k_c2f_level_set (below).
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

template <int NPL, int WPP, bool MEAN, bool XONLY, int NCH = 1, bool ROBUST = false>
__global__ __launch_bounds__(kBlock) void k_c2f_level(C2fArgsOf<MEAN, NCH, ROBUST> a) {
  c2f_level_body<NPL, WPP, MEAN, XONLY, NCH, ROBUST>(a);
}
// The lockstep twin (DESIGN.md "Lockstep sets"): the same workgroups along x, once per member along y.
template <int NPL, int WPP, bool MEAN, bool XONLY, int NCH = 1, bool ROBUST = false>
__global__ __launch_bounds__(kBlock) void k_c2f_level_set(SetArgs<C2fArgsOf<MEAN, NCH, ROBUST>> s) {
  static_assert(sizeof(s) <= kKernargLimit, "the argument block of a set exceeds the kernel-argument limit");
  c2f_level_body<NPL, WPP, MEAN, XONLY, NCH, ROBUST>(s.m[blockIdx.y]);
}

// the form follows from the patch size alone, as launch_patchdisp's: up to 4 pixels per lane one wave per node, above two
template <bool MEAN, bool XONLY, int NCH, bool ROBUST>
inline void launch_c2f_level(const C2fArgsOf<MEAN, NCH, ROBUST> &a, hipStream_t s) {
  const int npl = (a.P * a.P + 63) / 64;
  const dim3 blk(kBlock);
  if (npl > 4) {
    hipLaunchKernelGGL((k_c2f_level<8, 2, MEAN, XONLY, NCH, ROBUST>), dim3((a.K + kWaves / 2 - 1) / (kWaves / 2)), blk, 0, s,
                       a);
    return;
  }
  const dim3 g((a.K + kWaves - 1) / kWaves);
  if (npl <= 1)
    hipLaunchKernelGGL((k_c2f_level<1, 1, MEAN, XONLY, NCH, ROBUST>), g, blk, 0, s, a);
  else
    hipLaunchKernelGGL((k_c2f_level<4, 1, MEAN, XONLY, NCH, ROBUST>), g, blk, 0, s, a);
}

// k_flow_upsample's body (the kernel is described at the head of ictr_c2fflow.hip), for it and for its lockstep twin.
// s = 2^lv, inv_s = 2^-lv. Everything before the taps is exact in f32 (x + 0.5, the product with 2^-lv, - 0.5, rx,
// 1 - rx); the six products and three sums are taken in the order written, each rounded (no contraction), then s * val.
template <bool XONLY>
__device__ __forceinline__ void flow_upsample_body(const float2 *__restrict__ src, int wl, int hl, float inv_s, float s,
                                                   float2 *__restrict__ out, int w, int h) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * kWaves + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  const float fx = fminf(fmaxf(((float)x + 0.5f) * inv_s - 0.5f, 0.0f), (float)(wl - 1));
  const float fy = fminf(fmaxf(((float)y + 0.5f) * inv_s - 0.5f, 0.0f), (float)(hl - 1));
  const int x0 = (int)fx, y0 = (int)fy;  // fx, fy >= 0: the cast is the floor
  const int x1 = min(x0 + 1, wl - 1), y1 = min(y0 + 1, hl - 1);
  const float rx = fx - (float)x0, ry = fy - (float)y0;
  const float qx = 1.0f - rx, qy = 1.0f - ry;
  const size_t r0 = (size_t)y0 * wl, r1 = (size_t)y1 * wl;
  float2 o;
  if constexpr (XONLY) {  // y is not read and is +0.0
    const float *f = reinterpret_cast<const float *>(src);
    const float top = qx * f[2 * (r0 + x0)] + rx * f[2 * (r0 + x1)];
    const float bot = qx * f[2 * (r1 + x0)] + rx * f[2 * (r1 + x1)];
    o.x = s * (qy * top + ry * bot);
    o.y = 0.0f;
  } else {
    const float2 a = src[r0 + x0], b = src[r0 + x1], c = src[r1 + x0], d = src[r1 + x1];
    const float tx = qx * a.x + rx * b.x, bx = qx * c.x + rx * d.x;
    const float ty = qx * a.y + rx * b.y, by = qx * c.y + rx * d.y;
    o.x = s * (qy * tx + ry * bx);
    o.y = s * (qy * ty + ry * by);
  }
  out[(size_t)y * w + x] = o;
}

// the fields a lockstep k_flow_upsample reads and writes, per member
struct UpSetArgs {
  const float2 *src[kSetMax];
  float2 *out[kSetMax];
};
void launch_flow_upsample_set(const UpSetArgs &a, int n, int wl, int hl, int lv, int w, int h, int x_only, hipStream_t s);

// the lockstep twin's launch: k_c2f_level's grid along x, the n members along y
template <bool MEAN, bool XONLY, int NCH, bool ROBUST>
inline void launch_c2f_level_set(const SetArgs<C2fArgsOf<MEAN, NCH, ROBUST>> &a, int n, hipStream_t s) {
  const int npl = (a.m[0].P * a.m[0].P + 63) / 64, K = a.m[0].K;
  const dim3 blk(kBlock);
  if (npl > 4) {
    hipLaunchKernelGGL((k_c2f_level_set<8, 2, MEAN, XONLY, NCH, ROBUST>), dim3((K + kWaves / 2 - 1) / (kWaves / 2), n), blk, 0,
                       s, a);
    return;
  }
  const dim3 g((K + kWaves - 1) / kWaves, n);
  if (npl <= 1)
    hipLaunchKernelGGL((k_c2f_level_set<1, 1, MEAN, XONLY, NCH, ROBUST>), g, blk, 0, s, a);
  else
    hipLaunchKernelGGL((k_c2f_level_set<4, 1, MEAN, XONLY, NCH, ROBUST>), g, blk, 0, s, a);
}
// the lockstep forms' launchers, by [patnorm][channels]; x_only selects the XONLY form: the L2 forms (ictr_c2fset.hip)
// and the ROBUST ones (ictr_c2fset_robust.hip), in modules of their own like the ROBUST twins
void launch_c2f_level_set(const SetArgs<C2fArgs<false, 1>> &a, int n, int x_only, hipStream_t s);
void launch_c2f_level_set(const SetArgs<C2fArgs<false, 3>> &a, int n, int x_only, hipStream_t s);
void launch_c2f_level_set(const SetArgs<C2fArgs<true, 1>> &a, int n, int x_only, hipStream_t s);
void launch_c2f_level_set(const SetArgs<C2fArgs<true, 3>> &a, int n, int x_only, hipStream_t s);
void launch_c2f_level_set(const SetArgs<C2fArgsRobust<false, 1>> &a, int n, int x_only, hipStream_t s);
void launch_c2f_level_set(const SetArgs<C2fArgsRobust<false, 3>> &a, int n, int x_only, hipStream_t s);
void launch_c2f_level_set(const SetArgs<C2fArgsRobust<true, 1>> &a, int n, int x_only, hipStream_t s);
void launch_c2f_level_set(const SetArgs<C2fArgsRobust<true, 3>> &a, int n, int x_only, hipStream_t s);

// the ROBUST forms' launchers (ictr_c2fflow_robust.hip), by [patnorm][channels]; x_only selects the XONLY form
void launch_c2f_level_robust(const C2fArgsRobust<false, 1> &a, int x_only, hipStream_t s);
void launch_c2f_level_robust(const C2fArgsRobust<false, 3> &a, int x_only, hipStream_t s);
void launch_c2f_level_robust(const C2fArgsRobust<true, 1> &a, int x_only, hipStream_t s);
void launch_c2f_level_robust(const C2fArgsRobust<true, 3> &a, int x_only, hipStream_t s);

}  // namespace ictr
