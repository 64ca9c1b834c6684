// ictr_patchflow_dev.h -- the patch sampling of the patch searches, stated once for the kernels of ictr_patchflow.hip
// (k_patchflow, k_patchdisp) and of ictr_c2fflow.hip (k_c2f_level): the four tap weights and the first pixel of a patch
// (pf_taps), a pixel's two 8-byte loads (pf_load), their blend (pf_blend), the view test (pf_in_view) and the wave sum
// (pf_wave_sum). tests/patchflow_f32.py restates these expressions in NumPy f32.
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

}  // namespace ictr
