// ictr_warp_dev.h -- the level-0 warp rule of patchflow.refine_flow_host, step 1, stated once for k_fr_warp
// (ictr_flowrefine.hip) and k_densify (ictr_densify.hip): the inside test of a position, and the bilinear value of a plane
// at a position clamped to the frame BEFORE any index is formed, so that no index depends on a non-finite value and every
// tap lies in the frame (w, h >= 2). One fixed operation order; compiled without contraction.
#pragma once

#include <hip/hip_runtime.h>

namespace ictr {

__device__ __forceinline__ bool fr_inside(float px, float py, int w, int h) {
  return (px >= 0.0f) & (px <= (float)(w - 1)) & (py >= 0.0f) & (py <= (float)(h - 1));  // NaN: outside
}

// B: the plane at pixel (0, 0), stride sb
__device__ __forceinline__ float fr_bilinear(const float *__restrict__ B, int sb, int w, int h, float px, float py) {
  px = fminf(fmaxf(px, 0.0f), (float)(w - 1));  // fmaxf(NaN, 0) = 0
  py = fminf(fmaxf(py, 0.0f), (float)(h - 1));
  const int x0 = min((int)floorf(px), w - 2), y0 = min((int)floorf(py), h - 2);
  const float fx = px - (float)x0, fy = py - (float)y0;
  const float *b = B + (size_t)y0 * sb + x0;
  const float b00 = b[0], b01 = b[1], b10 = b[sb], b11 = b[sb + 1];
  const float w00 = (1.0f - fx) * (1.0f - fy), w01 = fx * (1.0f - fy), w10 = (1.0f - fx) * fy, w11 = fx * fy;
  return ((w00 * b00 + w01 * b01) + w10 * b10) + w11 * b11;
}

}  // namespace ictr
