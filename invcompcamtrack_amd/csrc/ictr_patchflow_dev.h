// ictr_patchflow_dev.h -- the patch search at one pyramid level, stated once for the kernels of ictr_patchflow.hip
// (k_patchflow, k_patchdisp) and of ictr_c2fflow.hip (k_c2f_level): the four tap weights and the first pixel of a patch
// (pf_taps), a pixel's two 8-byte loads (pf_load), their blend (pf_blend), the view test (pf_in_view), the sum over a
// patch's waves (pf_patch_sum) and the search itself, from the template to the last iteration (pf_level_search, 2-D or
// along x only; with MEAN, k_c2f_level's patch-mean normalisation) and one more window pass of frame B (pf_window_sum).
// tests/patchflow_f32.py restates these expressions in NumPy f32 (level_search there), tests/patnorm_f32.py the MEAN form.
// pf_level_search_ch and pf_window_sum_ch are the same two for NCH channels (1: the grey code; 3: colour frames, DESIGN.md
// "Colour"), restated for three channels by tests/c2frgb_f32.py.
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
// wave (all waves of the patch get the same bits). sSum: the workgroup's [kWaves][SW] floats (unused with one wave); SW
// is 4 for one channel and 8 for three, whose widest reduction carries six values in one trip.
template <int WPP, int N, int SW>
__device__ __forceinline__ void pf_patch_sum(float (&v)[N], float (*sSum)[SW]) {
  static_assert(N <= SW, "a wave's row of sSum holds SW partials");
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
// NCH channels (pf_level_search_ch; 1 is the grey search, to the operation): a frame is NCH planes of one geometry
// (L[0]'s). T, Gx, Gy of every channel stay in registers; H = sum_c sum_px G_c G_c^T and b = sum_c sum_px G_c r_c with
// r_c = T_c - I_c, ONE conditioning decision and ONE step per patch. The summation order is fixed: a lane adds channel 0,
// then 1, then 2 into the same accumulators, the pixels of a channel in the grey order, and the wave and patch sums follow
// once, so that an iteration keeps its single reduction. A channel's window loads of an iteration are all issued before
// their first use. MEAN: every channel loses its own mean; the reduction of H carries the NCH sums of T behind it (six
// values in 2-D), the second the NCH sums of Gx(, Gy), an iteration's the NCH sums of I behind b (five in 2-D), and
// b = s + sum_c (sum I_c / n) sum G_c, the channels added in order. mean_t[c] = mean(T_c).
// ROBUST is the Huber patch cost (DESIGN.md "Robust patch cost"): every pixel's and channel's residual is clipped,
// r <- fminf(fmaxf(r, -k), k), between T - iv and the two products; T, Gx, Gy, H, the conditioning decision, the view
// tests, the solve and the stop are the L2 forms', and without MEAN an iteration keeps its single reduction. k = huber_k
// travels behind the existing arguments and is read by the ROBUST forms alone: the others are today's code.
// ROBUST with MEAN cannot use b = s + mean(I) sum G, which rests on a linear residual; its iteration is the direct form in
// two passes. Pass 1: per channel all window loads issued, iv blended and KEPT in registers (NPL NCH values), sum I_c; one
// reduction of NCH values. Pass 2: r = T' - (iv - sum I_c / n), clipped, into b; one reduction of NB values. A window is
// still loaded once per iteration; the second reduction is on the chain (two waves per patch: two more barriers, every
// patch of the workgroup running every slot as before). The operation order is fixed: channels 0, 1, 2 into the same
// accumulators, the pixels of a channel in the grey order; (iv - mean) is formed first, then T' minus it. The sums of Gx
// and Gy of the L2 MEAN forms are not taken. tests/c2fcost_f32.py restates the ROBUST forms.
template <int NPL, int WPP, bool XONLY, bool MEAN, int NCH, int SW, bool ROBUST = false>
__device__ __forceinline__ int pf_level_search_ch(const PFPlanes (&Lc)[NCH], int P, float xl, float yl, bool ok, float &px,
                                                  float &py, int &nit, int maxiter, float eps2, float min_cond,
                                                  float (*sSum)[SW], float (&mean_t)[NCH], float huber_k = 0.0f) {
  const PFPlanes &L = Lc[0];  // the geometry of every channel
  const int n = P * P;
  const int slot0 = (WPP > 1 ? ((threadIdx.x >> 6) % WPP) * 64 : 0) + (threadIdx.x & 63);
  const PFTaps ta = pf_taps(ok ? xl : 1.0f, ok ? yl : 1.0f, P, L.sw, L.shift);
  int off[NPL];
  float T[NCH][NPL], Gx[NCH][NPL], Gy[NCH][XONLY ? 1 : NPL];
  constexpr int NH = XONLY ? 2 : 3, NB = XONLY ? 1 : 2;  // the sums of H and of b; MEAN: sum T_c, sum I_c behind them
  float h[MEAN ? NH + NCH : NH] = {};  // hxx, (hxy,) hyy(, sum T_c)
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      const int q = slot0 + 64 * WPP * i;
      const bool in = q < n;
      if (c == 0) off[i] = in ? (q / P) * L.sw + (q % P) : 0;  // beyond the patch: its first pixel, with zero templates
      const int idx = ta.base + off[i];
      const float t = pf_fetch(Lc[c].a, idx, L.sw, ta), gx = pf_fetch(Lc[c].ax, idx, L.sw, ta),
                  gy = pf_fetch(Lc[c].ay, idx, L.sw, ta);
      T[c][i] = in ? t : 0.0f;
      Gx[c][i] = in ? gx : 0.0f;
      const float gyi = in ? gy : 0.0f;
      h[0] += Gx[c][i] * Gx[c][i];
      if constexpr (XONLY) {
        h[1] += gyi * gyi;
      } else {
        Gy[c][i] = gyi;
        h[1] += Gx[c][i] * gyi;
        h[2] += gyi * gyi;
      }
      if constexpr (MEAN) h[NH + c] += T[c][i];
    }
  }
  pf_patch_sum<WPP>(h, sSum);
  float sg[NB * NCH] = {};  // MEAN (L2): per channel sum Gx(, sum Gy)
  if constexpr (MEAN) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      mean_t[c] = h[NH + c] / (float)n;
#pragma unroll
      for (int i = 0; i < NPL; ++i) {
        T[c][i] = (slot0 + 64 * WPP * i < n) ? T[c][i] - mean_t[c] : 0.0f;
        if constexpr (!ROBUST) {
          sg[NB * c] += Gx[c][i];
          if constexpr (!XONLY) sg[NB * c + 1] += Gy[c][i];
        }
      }
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
  if constexpr (MEAN && !ROBUST) pf_patch_sum<WPP>(sg, sSum);
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
    float b[(MEAN && !ROBUST) ? NB + NCH : NB] = {};  // bx, (by)(, sum I_c)
    if constexpr (ROBUST && MEAN) {
      float iv[NCH][NPL], si[NCH] = {};
#pragma unroll
      for (int c = 0; c < NCH; ++c) {  // pass 1: the windows, once
        PFWin w[NPL];
#pragma unroll
        for (int i = 0; i < NPL; ++i) w[i] = pf_load(Lc[c].b, tb.base + off[i], L.sw);  // all in flight before the first use
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
          iv[c][i] = pf_blend(w[i], tb);
          si[c] += (slot0 + 64 * WPP * i < n) ? iv[c][i] : 0.0f;
        }
      }
      pf_patch_sum<WPP>(si, sSum);
#pragma unroll
      for (int c = 0; c < NCH; ++c) {  // pass 2: the clipped residual of the mean-free window
        const float mi = si[c] / (float)n;
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
          float r = T[c][i] - (iv[c][i] - mi);
          r = (slot0 + 64 * WPP * i < n) ? r : 0.0f;
          r = fminf(fmaxf(r, -huber_k), huber_k);
          b[0] += Gx[c][i] * r;
          if constexpr (!XONLY) b[1] += Gy[c][i] * r;
        }
      }
      pf_patch_sum<WPP>(b, sSum);
    } else {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        PFWin w[NPL];
#pragma unroll
        for (int i = 0; i < NPL; ++i) w[i] = pf_load(Lc[c].b, tb.base + off[i], L.sw);  // all in flight before the first use
#pragma unroll
        for (int i = 0; i < NPL; ++i) {
          const bool in = slot0 + 64 * WPP * i < n;
          const float iv = pf_blend(w[i], tb);
          float r = T[c][i] - iv;
          r = in ? r : 0.0f;  // (T = 0 there, but the frame value is not)
          if constexpr (ROBUST) r = fminf(fmaxf(r, -huber_k), huber_k);
          b[0] += Gx[c][i] * r;
          if constexpr (!XONLY) b[1] += Gy[c][i] * r;
          if constexpr (MEAN) b[NB + c] += in ? iv : 0.0f;
        }
      }
      pf_patch_sum<WPP>(b, sSum);
      if constexpr (MEAN) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const float mi = b[NB + c] / (float)n;
          b[0] = b[0] + mi * sg[NB * c];
          if constexpr (!XONLY) b[1] = b[1] + mi * sg[NB * c + 1];
        }
      }
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
// one channel: the search as k_patchflow, k_patchdisp and the grey k_c2f_level call it
template <int NPL, int WPP, bool XONLY, bool MEAN>
__device__ __forceinline__ int pf_level_search(const PFPlanes &L, int P, float xl, float yl, bool ok, float &px, float &py,
                                               int &nit, int maxiter, float eps2, float min_cond, float (*sSum)[4],
                                               float &mean_t) {
  const PFPlanes Lc[1] = {L};
  float m[1] = {mean_t};
  const int why = pf_level_search_ch<NPL, WPP, XONLY, MEAN, 1, 4>(Lc, P, xl, yl, ok, px, py, nit, maxiter, eps2, min_cond,
                                                                  sSum, m);
  mean_t = m[0];
  return why;
}

// The sum of frame B over the P x P patch at (x, y), in the search's sampling, lane order and sum shape: one more window
// pass, as an iteration makes it. Two waves per patch: every patch of the workgroup calls it (the barriers), one without a
// use for the sum at the harmless window (1, 1). NCH channels: s[c] per channel, one reduction of NCH values.
template <int NPL, int WPP, int NCH, int SW>
__device__ __forceinline__ void pf_window_sum_ch(const PFPlanes (&Lc)[NCH], int P, float x, float y, float (*sSum)[SW],
                                                 float (&s)[NCH]) {
  const PFPlanes &L = Lc[0];
  const int n = P * P;
  const int slot0 = (WPP > 1 ? ((threadIdx.x >> 6) % WPP) * 64 : 0) + (threadIdx.x & 63);
  const PFTaps tb = pf_taps(x, y, P, L.sw, L.shift);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    PFWin w[NPL];
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      const int q = slot0 + 64 * WPP * i;
      w[i] = pf_load(Lc[c].b, tb.base + (q < n ? (q / P) * L.sw + (q % P) : 0), L.sw);
    }
    s[c] = 0.0f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      const float iv = pf_blend(w[i], tb);
      s[c] += (slot0 + 64 * WPP * i < n) ? iv : 0.0f;
    }
  }
  pf_patch_sum<WPP>(s, sSum);
}
template <int NPL, int WPP>
__device__ __forceinline__ float pf_window_sum(const PFPlanes &L, int P, float x, float y, float (*sSum)[4]) {
  const PFPlanes Lc[1] = {L};
  float s[1];
  pf_window_sum_ch<NPL, WPP, 1, 4>(Lc, P, x, y, sSum, s);
  return s[0];
}

}  // namespace ictr
