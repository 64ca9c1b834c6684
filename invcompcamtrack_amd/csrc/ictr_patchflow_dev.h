// ictr_patchflow_dev.h -- the patch search at one pyramid level, stated once for the kernels of ictr_patchflow.hip
// (k_patchflow, k_patchdisp) and of ictr_c2fflow.hip (k_c2f_level): the four tap weights and the first pixel of a patch
// (pf_taps), a pixel's two 8-byte loads (pf_load), their blend (pf_blend), the view test (pf_in_view), the sum over a
// patch's waves (pf_patch_sum) and the search itself, from the template to the last iteration (pf_level_search, 2-D or
// along x only; with MEAN, k_c2f_level's patch-mean normalisation) and one more window pass of frame B (pf_window_sum).
// tests/patchflow_f32.py restates these expressions in NumPy f32 (level_search there), tests/patnorm_f32.py the MEAN form.
#pragma once

#include "ictr_dev.h"
#include "ictr_devfn.h"

namespace ictr {

__device__ __forceinline__ float pf_wave_sum(float v) { return wave_sum_dpp(v); }

struct PFTaps {
  float w0, w1, w2, w3;
  int base;
};
// shift = (pad - P) * (sw + 1): (p + P/2) is the patch's first pixel only in a plane padded by exactly P
__device__ __forceinline__ PFTaps pf_taps(float mx, float my, int P, int sw, int shift) {
  PFTaps t;
  const float f0 = floorf(mx), f1 = floorf(my);
  const int p0 = (int)f0 + 1, p1 = (int)f1 + 1;  // taps (floor, floor + 1): the pair the weights are taken for
  const float r0 = mx - f0, r1 = my - f1;
  t.w0 = r0 * r1;
  t.w1 = (1 - r0) * r1;
  t.w2 = r0 * (1 - r1);
  t.w3 = (1 - r0) * (1 - r1);
  t.base = (p1 + P / 2) * sw + p0 + P / 2 + shift;
  return t;
}
struct PFWin {
  f32x2_a4 ab, cd;  // (x-1,y),(x,y) and (x-1,y-1),(x,y-1)
};
__device__ __forceinline__ PFWin pf_load(gconst_f32 img, int idx, int sw) {
  PFWin w;
  w.ab = *reinterpret_cast<gconst_f32x2>(img + (idx - 1));
  w.cd = *reinterpret_cast<gconst_f32x2>(img + (idx - sw - 1));
  return w;
}
__device__ __forceinline__ float pf_blend(const PFWin &w, const PFTaps &t) {
  return t.w0 * w.ab.y + t.w1 * w.ab.x + t.w2 * w.cd.y + t.w3 * w.cd.x;
}
__device__ __forceinline__ float pf_fetch(gconst_f32 img, int idx, int sw, const PFTaps &t) {
  return pf_blend(pf_load(img, idx, sw), t);
}
__device__ __forceinline__ bool pf_in_view(float x, float y, float swo, float sho) {
  return (x >= 0.0f) & (y >= 0.0f) & (x <= swo) & (y <= sho);
}

// WPP waves share a patch (pixels per lane NPL = ceil(P*P / (64 WPP))). One wave per patch needs no synchronisation at
// all; for large patches (more than 4 pixels per lane) TWO waves per patch halve each wave's chain of pixels and double
// the waves that hide each other's loads: the wave sums then meet in LDS, one workgroup barrier per reduction.
// pf_patch_sum: N per-wave totals summed over the patch's WPP waves, the partials added in wave order from 0 by every
// wave (all waves of the patch get the same bits). sSum: the workgroup's [kWaves][4] floats (unused with one wave).
template <int WPP, int N>
__device__ __forceinline__ void pf_patch_sum(float (&v)[N], float (*sSum)[4]) {
  static_assert(N <= 4, "a wave's row of sSum holds four partials");
#pragma unroll
  for (int j = 0; j < N; ++j) v[j] = pf_wave_sum(v[j]);
  if constexpr (WPP > 1) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();  // (the previous reduction's partials have been read)
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < N; ++j) sSum[wave][j] = v[j];
    }
    __syncthreads();
    const int w0 = wave - wave % WPP;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      v[j] = 0.0f;
#pragma unroll
      for (int q = 0; q < WPP; ++q) v[j] += sSum[w0 + q][j];
    }
  }
}

// one level's planes and geometry, as PFLevel and C2fArgs carry them
struct PFPlanes {
  gconst_f32 a, ax, ay, b;  // frame A image + gradients, frame B image (padded planes)
  int sw, shift;            // row stride; (pad - P) * (sw + 1)
  float swo, sho;           // the level's unpadded size
};
enum { PF_STOP_NONE = 0, PF_STOP_COND = 1, PF_STOP_VIEW = 2 };  // why a patch stopped being tracked at a level

// The search of one P x P patch at (xl, yl) of one level, from the displacement (px, py): the template T/Gx/Gy in
// registers, H summed once, then up to maxiter Gauss-Newton steps p += H^-1 b, b = sum [Gx Gy]^T (T - I(x + p)), until
// |dp|^2 < eps2. XONLY is the 1-D rule: hxx and hyy alone (Gy lives only until hyy is summed), the patch is refused iff
// !(tr > 0) or !(hxx > min_cond * tr) (horizontal edges alone carry no disparity; vertical edges alone, which the 2x2
// system refuses, are kept), p += bx * (1 / hxx) and y never moves. Returns why the patch is no longer tracked, if so.
// An iteration is a latency chain per wave: the four taps of a pixel are TWO 8-byte loads, every lane's loads of an
// iteration are issued before the first is consumed (pixels beyond the patch read the patch's first pixel and carry
// zero templates: no branch in the loop), and the wave sums use DPP.
// One wave per patch leaves at the first decision against it (and is not to be called with !ok). Two waves per patch
// share barriers, which need a uniform loop structure: every patch of the workgroup runs every iteration slot, and one
// that is not ok, stopped or converged only stops updating (its windows are the harmless in-plane one at (1,1)).
// MEAN is patch-mean normalisation: T' = T - mean(T) once and r = T' - (I - mean(I)) in every iteration. The sum of T
// joins the sums of H in their one reduction (of four; XONLY of three), the sums of Gx and Gy (XONLY: of Gx alone) are
// taken once in a second, and an iteration keeps its single reduction, now of three (XONLY of two): with
// s = sum G (T' - I), b = s + (sum I / n) sum G. The direct form would need the frame mean before the residual, two
// reductions on the chain and in the two-wave form four barriers.
// mean_t receives mean(T) = sum T / n (also when the patch is refused by the conditioning test).
template <int NPL, int WPP, bool XONLY, bool MEAN>
__device__ __forceinline__ int pf_level_search(const PFPlanes &L, int P, float xl, float yl, bool ok, float &px, float &py,
                                               int &nit, int maxiter, float eps2, float min_cond, float (*sSum)[4],
                                               float &mean_t) {
  const int n = P * P;
  const int slot0 = (WPP > 1 ? ((threadIdx.x >> 6) % WPP) * 64 : 0) + (threadIdx.x & 63);
  const PFTaps ta = pf_taps(ok ? xl : 1.0f, ok ? yl : 1.0f, P, L.sw, L.shift);
  int off[NPL];
  float T[NPL], Gx[NPL], Gy[XONLY ? 1 : NPL];
  constexpr int NH = XONLY ? 2 : 3, NB = XONLY ? 1 : 2;  // the sums of H and of b; MEAN: sum T, sum I behind them
  float h[MEAN ? NH + 1 : NH] = {};  // hxx, (hxy,) hyy(, sum T)
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    const int q = slot0 + 64 * WPP * i;
    const bool in = q < n;
    off[i] = in ? (q / P) * L.sw + (q % P) : 0;  // beyond the patch: its first pixel, with zero templates
    const int idx = ta.base + off[i];
    const float t = pf_fetch(L.a, idx, L.sw, ta), gx = pf_fetch(L.ax, idx, L.sw, ta), gy = pf_fetch(L.ay, idx, L.sw, ta);
    T[i] = in ? t : 0.0f;
    Gx[i] = in ? gx : 0.0f;
    const float gyi = in ? gy : 0.0f;
    h[0] += Gx[i] * Gx[i];
    if constexpr (XONLY) {
      h[1] += gyi * gyi;
    } else {
      Gy[i] = gyi;
      h[1] += Gx[i] * gyi;
      h[2] += gyi * gyi;
    }
    if constexpr (MEAN) h[NH] += T[i];
  }
  pf_patch_sum<WPP>(h, sSum);
  float sg[NB] = {};  // MEAN: sum Gx(, sum Gy)
  if constexpr (MEAN) {
    mean_t = h[NH] / (float)n;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      T[i] = (slot0 + 64 * WPP * i < n) ? T[i] - mean_t : 0.0f;
      sg[0] += Gx[i];
      if constexpr (!XONLY) sg[1] += Gy[i];
    }
  }
  const float hxx = h[0], hxy = XONLY ? 0.0f : h[1], hyy = h[XONLY ? 1 : 2];
  const float tr = hxx + hyy;
  float inv;  // of what the solve divides by
  bool cond;
  if constexpr (XONLY) {
    cond = (tr > 0.0f) && (hxx > min_cond * tr);
    inv = 1.0f / hxx;
  } else {
    const float det = hxx * hyy - hxy * hxy;
    cond = (det > min_cond * tr * tr) && (tr > 0.0f);  // else textureless or 1-D structure
    inv = 1.0f / det;
  }
  int why = PF_STOP_NONE;
  if (ok && !cond) why = PF_STOP_COND;
  if (WPP == 1 && why) return why;
  if constexpr (MEAN) pf_patch_sum<WPP>(sg, sSum);
  bool run = ok && !why;  // this patch still iterates at this level
  for (int it = 0; it < maxiter; ++it) {
    if (WPP == 1 && !run) break;
    const float cx = xl + px, cy = XONLY ? yl : yl + py;
    if (run && !pf_in_view(cx, cy, L.swo, L.sho)) {
      why = PF_STOP_VIEW;
      run = false;
      if (WPP == 1) break;
    }
    const PFTaps tb = pf_taps(run ? cx : 1.0f, run ? cy : 1.0f, P, L.sw, L.shift);
    float b[MEAN ? NB + 1 : NB] = {};  // bx, (by)(, sum I)
    PFWin w[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) w[i] = pf_load(L.b, tb.base + off[i], L.sw);  // all in flight before the first use
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      const bool in = slot0 + 64 * WPP * i < n;
      const float iv = pf_blend(w[i], tb);
      float r = T[i] - iv;
      r = in ? r : 0.0f;  // (T = 0 there, but the frame value is not)
      b[0] += Gx[i] * r;
      if constexpr (!XONLY) b[1] += Gy[i] * r;
      if constexpr (MEAN) b[NB] += in ? iv : 0.0f;
    }
    pf_patch_sum<WPP>(b, sSum);
    if constexpr (MEAN) {
      const float mi = b[NB] / (float)n;
      b[0] = b[0] + mi * sg[0];
      if constexpr (!XONLY) b[1] = b[1] + mi * sg[1];
    }
    if (run) {
      float dx, dy = 0.0f;
      if constexpr (XONLY) {
        dx = b[0] * inv;
      } else {
        dx = (hyy * b[0] - hxy * b[1]) * inv;
        dy = (hxx * b[1] - hxy * b[0]) * inv;
        py += dy;
      }
      px += dx;
      ++nit;
      if ((XONLY ? dx * dx : dx * dx + dy * dy) < eps2) run = false;
    }
  }
  return why;
}

// The sum of frame B over the P x P patch at (x, y), in the search's sampling, lane order and sum shape: one more window
// pass, as an iteration makes it. Two waves per patch: every patch of the workgroup calls it (the barriers), one without a
// use for the sum at the harmless window (1, 1).
template <int NPL, int WPP>
__device__ __forceinline__ float pf_window_sum(const PFPlanes &L, int P, float x, float y, float (*sSum)[4]) {
  const int n = P * P;
  const int slot0 = (WPP > 1 ? ((threadIdx.x >> 6) % WPP) * 64 : 0) + (threadIdx.x & 63);
  const PFTaps tb = pf_taps(x, y, P, L.sw, L.shift);
  PFWin w[NPL];
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    const int q = slot0 + 64 * WPP * i;
    w[i] = pf_load(L.b, tb.base + (q < n ? (q / P) * L.sw + (q % P) : 0), L.sw);
  }
  float s[1] = {};
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    const float iv = pf_blend(w[i], tb);
    s[0] += (slot0 + 64 * WPP * i < n) ? iv : 0.0f;
  }
  pf_patch_sum<WPP>(s, sSum);
  return s[0];
}

}  // namespace ictr
