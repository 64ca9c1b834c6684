// ictr_flowrefine.hip -- variational refinement of a dense flow field at level 0 (DESIGN.md §4 "Variational refinement of
// a dense field"). The rule is build-defined; its statement of record is patchflow.refine_flow_host (NumPy, f64). This
// file is the same rule in f32 with one fixed operation order, restated in NumPy f32 by tests/flowrefine_f32.py.
//
// One outer iteration is   k_fr_warp<1> -> k_fr_coef -> n_sor x (k_fr_sor<0>, k_fr_sor<1>)   on planes of the frame's size:
//   k_fr_warp   (u, v) += (du, dv) of the previous outer iteration (step 6 folded in), then Bw = bilinear(B, x + u, y + v).
//               The position is clamped with fmaxf / fminf BEFORE any index is formed: no index depends on a non-finite
//               value, every tap lies in the frame.
//   k_fr_coef   one 16 x 16 tile per workgroup with a 2-pixel halo of Bw, A, u, v in LDS (the stencil reaches +-2: a
//               derivative of a derivative, and the edge weight of s). Writes a11, a12, a22, b1, b2, the right and down
//               edge weights, and du = dv = 0.
//   k_fr_sor<c> one half-sweep: a lane per pixel of colour (x + y) & 1 == c. All four neighbours have the other colour,
//               which this launch does not write: no order inside a half-sweep, the result is deterministic. The five
//               coefficient planes are stored compacted by colour (fr_ci).
// k_fr_warp<3> and k_fr_coef_rgb are the two stages on colour frames (three planes per frame; the coarse-to-fine flow's
// colour runs alone): per-channel derivatives, robust weights joint over the channels, coefficients as channel means.
// k_fr_final adds the last (du, dv) into the interleaved result. Memory bound throughout: plain vector loads and stores,
// no atomics. Everything is enqueued on the caller's stream; run waits for nothing but the copy of a field that lives in
// host memory.
// Every kernel takes the arguments of 1 .. kSetMax refiners of one size and one set of parameters (DESIGN.md §4 "Lockstep
// sets") and runs its body on member m's, m the block index along the grid dimension the stage does not use: y for the
// two linear kernels, z for the others. A refiner's own run is a set of one.
#include <math.h>
#include <string.h>

#include <memory>
#include <vector>

#include "ictr_dev.h"
#include "ictr_launch.h"
#include "ictr_flowgrid_dev.h"
#include "ictr_warp_dev.h"

namespace ictr {

constexpr int kFrTile = 16;                   // kFrTile^2 = kBlock: one pixel per lane
constexpr int kFrHalo = 2;
constexpr int kFrSide = kFrTile + 2 * kFrHalo;  // 20
constexpr float kFrEps2 = 1e-3f * 1e-3f;
constexpr float kFrZeta2 = 0.1f * 0.1f;
static_assert(kFrTile * kFrTile == kBlock, "k_fr_coef maps one lane to one pixel of its tile");

// NCH planes per frame: 1 for grey frames, 3 for colour
template <int NCH>
struct FrArgsT {
  const float *A[NCH], *B[NCH];  // per channel, level planes at pixel (0, 0), strides sa, sb
  int sa, sb, w, h;
  float *u, *v, *du, *dv;        // planes [h][w], and so are those below
  float *bw[NCH];                // per channel
  float *a11, *a12, *a22, *b1, *b2, *wr, *wd;
  float alpha, gamma, delta, omega;
  int x_only;
};
// The half-sweeps and k_fr_final read neither the frames nor Bw: they take the one-channel arguments whatever the frames
// are (fr_args<1>).
using FrArgs = FrArgsT<1>;

// The bodies, each for one member, whose arguments it takes by value; the kernels are below them.
// interleaved (u, v) -> the two working planes
__device__ __forceinline__ void fr_init_body(const float2 *__restrict__ f0, float *__restrict__ u, float *__restrict__ v, int n) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float2 f = f0[i];
  u[i] = f.x;
  v[i] = f.y;
}
// (a flow grid's dense field is formed by launch_fg_dense: ictr_flowgrid_dev.h)

// Where a coefficient (a11, a12, a22, b1, b2) of pixel (X, Y) lives in its plane: the plane is compacted by colour, first
// all pixels of colour 0 row by row, then those of colour 1, rows of ceil(w / 2). A half-sweep, which reads the
// coefficients of one colour only, then reads whole lines (measured against the pixel order: DESIGN.md).
__host__ __device__ __forceinline__ int fr_ci(int X, int Y, int w, int h) {
  const int wc = (w + 1) >> 1;
  return ((X + Y) & 1) * wc * h + Y * wc + (X >> 1);
}

// fr_inside, fr_bilinear: ictr_warp_dev.h

// (the channels of B are warped at ONE position)
template <int NCH>
__device__ __forceinline__ void fr_warp_body(FrArgsT<NCH> a, int fold) {
  const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * kWaves + (threadIdx.x >> 6);
  if (X >= a.w || Y >= a.h) return;
  const int i = Y * a.w + X;
  float u = a.u[i], v = a.v[i];
  if (fold) {
    u += a.du[i];
    a.u[i] = u;
    if (!a.x_only) {
      v += a.dv[i];
      a.v[i] = v;
    }
  }
  // (no loop statement in the grey form, not even one of one trip: with one the compiler moves the argument loads of the
  // fold into its branch, three scalar loads and a branch more: DESIGN.md "Colour")
  if constexpr (NCH == 1) {
    a.bw[0][i] = fr_bilinear(a.B[0], a.sb, a.w, a.h, (float)X + u, (float)Y + v);
  } else {
#pragma unroll
    for (int c = 0; c < NCH; ++c) a.bw[c][i] = fr_bilinear(a.B[c], a.sb, a.w, a.h, (float)X + u, (float)Y + v);
  }
}

// a tile with its halo; (cx, cy) are tile coordinates, the frame coordinate is (gx0 + cx, gy0 + cy)
struct FrTile {
  const float (*p)[kFrSide];
  int gx0, gy0, w, h;
  __device__ __forceinline__ float at(int cx, int cy) const { return p[cy][cx]; }
  // dx(a) = (a[x+1] - a[x-1]) / 2, and 0 in the first and last column; dy likewise
  __device__ __forceinline__ float dx(int cx, int cy) const {
    const int X = gx0 + cx;
    return (X <= 0 || X >= w - 1) ? 0.0f : 0.5f * (p[cy][cx + 1] - p[cy][cx - 1]);
  }
  __device__ __forceinline__ float dy(int cx, int cy) const {
    const int Y = gy0 + cy;
    return (Y <= 0 || Y >= h - 1) ? 0.0f : 0.5f * (p[cy + 1][cx] - p[cy - 1][cx]);
  }
  __device__ __forceinline__ float dxx(int cx, int cy) const {
    const int X = gx0 + cx;
    return (X <= 0 || X >= w - 1) ? 0.0f : 0.5f * (dx(cx + 1, cy) - dx(cx - 1, cy));
  }
  __device__ __forceinline__ float dxy(int cx, int cy) const {  // dy(dx(a))
    const int Y = gy0 + cy;
    return (Y <= 0 || Y >= h - 1) ? 0.0f : 0.5f * (dx(cx, cy + 1) - dx(cx, cy - 1));
  }
  __device__ __forceinline__ float dyy(int cx, int cy) const {
    const int Y = gy0 + cy;
    return (Y <= 0 || Y >= h - 1) ? 0.0f : 0.5f * (dy(cx, cy + 1) - dy(cx, cy - 1));
  }
};
// s = alpha / 2 / sqrt(|grad u|^2 + |grad v|^2 + eps^2)
__device__ __forceinline__ float fr_smooth(const FrTile &tu, const FrTile &tv, int cx, int cy, float half_alpha) {
  const float ux = tu.dx(cx, cy), uy = tu.dy(cx, cy), vx = tv.dx(cx, cy), vy = tv.dy(cx, cy);
  float t = ux * ux + uy * uy;
  t = t + vx * vx;
  t = t + vy * vy;
  t = t + kFrEps2;
  return half_alpha / sqrtf(t);
}

// k_fr_coef and k_fr_coef_rgb (below) are two kernels and not one template over the channel count: this one forms
// w0 = ((delta n0) / 2) / sqrt(n0 Iz^2 + eps^2) per pixel, the colour one q0 on the channel mean, then q0 n0[c], and divides
// the coefficients by 3. These are different roundings, so a template would be these two bodies under `if constexpr`.
__device__ __forceinline__ void fr_coef_body(FrArgsT<1> a) {
  __shared__ float sB[kFrSide][kFrSide], sA[kFrSide][kFrSide], sU[kFrSide][kFrSide], sV[kFrSide][kFrSide];
  const int gx0 = blockIdx.x * kFrTile - kFrHalo, gy0 = blockIdx.y * kFrTile - kFrHalo;
  // the halo is read at the nearest pixel of the frame; what lies outside is never used (the border rules above)
  for (int q = threadIdx.x; q < kFrSide * kFrSide; q += kBlock) {
    const int cy = q / kFrSide, cx = q - cy * kFrSide;
    const int X = min(max(gx0 + cx, 0), a.w - 1), Y = min(max(gy0 + cy, 0), a.h - 1);
    const int i = Y * a.w + X;
    sB[cy][cx] = a.bw[0][i];
    sU[cy][cx] = a.u[i];
    sV[cy][cx] = a.v[i];
    sA[cy][cx] = a.A[0][(size_t)Y * a.sa + X];
  }
  __syncthreads();
  const int cx = (threadIdx.x & (kFrTile - 1)) + kFrHalo, cy = threadIdx.x / kFrTile + kFrHalo;
  const int X = gx0 + cx, Y = gy0 + cy;
  if (X >= a.w || Y >= a.h) return;
  const int i = Y * a.w + X;
  const FrTile tb{sB, gx0, gy0, a.w, a.h}, ta{sA, gx0, gy0, a.w, a.h}, tu{sU, gx0, gy0, a.w, a.h},
      tv{sV, gx0, gy0, a.w, a.h};
  // step 2
  const float Ix = tb.dx(cx, cy), Iy = tb.dy(cx, cy), Iz = tb.at(cx, cy) - ta.at(cx, cy);
  const float Ixx = tb.dxx(cx, cy), Ixy = tb.dxy(cx, cy), Iyy = tb.dyy(cx, cy);
  const float Ixz = Ix - ta.dx(cx, cy), Iyz = Iy - ta.dy(cx, cy);
  // step 3
  const bool in = fr_inside((float)X + tu.at(cx, cy), (float)Y + tv.at(cx, cy), a.w, a.h);
  const float n0 = 1.0f / ((Ix * Ix + Iy * Iy) + kFrZeta2);
  const float n1 = 1.0f / ((Ixx * Ixx + Ixy * Ixy) + kFrZeta2);
  const float n2 = 1.0f / ((Ixy * Ixy + Iyy * Iyy) + kFrZeta2);
  const float w0 = in ? ((a.delta * n0) * 0.5f) / sqrtf((n0 * Iz) * Iz + kFrEps2) : 0.0f;
  const float wg = in ? (a.gamma * 0.5f) / sqrtf(((n1 * Ixz) * Ixz + (n2 * Iyz) * Iyz) + kFrEps2) : 0.0f;
  const int c = fr_ci(X, Y, a.w, a.h);
  a.a11[c] = w0 * (Ix * Ix) + wg * (n1 * (Ixx * Ixx) + n2 * (Ixy * Ixy));
  a.a12[c] = w0 * (Ix * Iy) + wg * (n1 * (Ixx * Ixy) + n2 * (Ixy * Iyy));
  a.a22[c] = w0 * (Iy * Iy) + wg * (n1 * (Ixy * Ixy) + n2 * (Iyy * Iyy));
  a.b1[c] = -(w0 * (Ix * Iz) + wg * (n1 * (Ixx * Ixz) + n2 * (Ixy * Iyz)));
  a.b2[c] = -(w0 * (Iy * Iz) + wg * (n1 * (Ixy * Ixz) + n2 * (Iyy * Iyz)));
  // step 4: the edge to the right and the edge down carry the mean of their two pixels' s; no edge leaves the frame
  const float ha = a.alpha * 0.5f;
  const float s0 = fr_smooth(tu, tv, cx, cy, ha);
  a.wr[i] = X < a.w - 1 ? 0.5f * (s0 + fr_smooth(tu, tv, cx + 1, cy, ha)) : 0.0f;
  a.wd[i] = Y < a.h - 1 ? 0.5f * (s0 + fr_smooth(tu, tv, cx, cy + 1, ha)) : 0.0f;
  // step 5 starts from du = dv = 0
  a.du[i] = 0.0f;
  a.dv[i] = 0.0f;
}

// The colour form of the coefficient stage (DESIGN.md §4 "Colour"): three planes per frame and three Bw planes. Steps 1
// and 2 run per channel, n0, n1, n2 are per channel; the two robust weights are joint over the channels, taken on the
// channel mean, and the coefficients are channel means. Every sum over the channels starts from 0.0f and adds channel 0,
// 1, 2 in order; the mean is the quotient by 3.0f. Restated by tests/c2frgb_f32.py.
// U and V are staged once, and with them the three channels' tiles of Bw and A: 8 tiles x 1600 B = 12.8 KB of LDS. A
// lane keeps the eleven per-channel values of all three channels (the joint weights need every channel's Iz, Ixz, Iyz
// before any coefficient is final); the register report shows no scratch.
__device__ __forceinline__ void fr_coef_rgb_body(FrArgsT<3> a) {
  __shared__ float sB[3][kFrSide][kFrSide], sA[3][kFrSide][kFrSide], sU[kFrSide][kFrSide], sV[kFrSide][kFrSide];
  const int gx0 = blockIdx.x * kFrTile - kFrHalo, gy0 = blockIdx.y * kFrTile - kFrHalo;
  for (int q = threadIdx.x; q < kFrSide * kFrSide; q += kBlock) {
    const int cy = q / kFrSide, cx = q - cy * kFrSide;
    const int X = min(max(gx0 + cx, 0), a.w - 1), Y = min(max(gy0 + cy, 0), a.h - 1);
    const int i = Y * a.w + X;
    sU[cy][cx] = a.u[i];
    sV[cy][cx] = a.v[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      sB[c][cy][cx] = a.bw[c][i];
      sA[c][cy][cx] = a.A[c][(size_t)Y * a.sa + X];
    }
  }
  __syncthreads();
  const int cx = (threadIdx.x & (kFrTile - 1)) + kFrHalo, cy = threadIdx.x / kFrTile + kFrHalo;
  const int X = gx0 + cx, Y = gy0 + cy;
  if (X >= a.w || Y >= a.h) return;
  const int i = Y * a.w + X;
  const FrTile tu{sU, gx0, gy0, a.w, a.h}, tv{sV, gx0, gy0, a.w, a.h};
  const bool in = fr_inside((float)X + tu.at(cx, cy), (float)Y + tv.at(cx, cy), a.w, a.h);
  float Ix[3], Iy[3], Iz[3], Ixx[3], Ixy[3], Iyy[3], Ixz[3], Iyz[3], n0[3], n1[3], n2[3];
  float s0 = 0.0f, sg = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const FrTile tb{sB[c], gx0, gy0, a.w, a.h}, ta{sA[c], gx0, gy0, a.w, a.h};
    Ix[c] = tb.dx(cx, cy), Iy[c] = tb.dy(cx, cy), Iz[c] = tb.at(cx, cy) - ta.at(cx, cy);
    Ixx[c] = tb.dxx(cx, cy), Ixy[c] = tb.dxy(cx, cy), Iyy[c] = tb.dyy(cx, cy);
    Ixz[c] = Ix[c] - ta.dx(cx, cy), Iyz[c] = Iy[c] - ta.dy(cx, cy);
    n0[c] = 1.0f / ((Ix[c] * Ix[c] + Iy[c] * Iy[c]) + kFrZeta2);
    n1[c] = 1.0f / ((Ixx[c] * Ixx[c] + Ixy[c] * Ixy[c]) + kFrZeta2);
    n2[c] = 1.0f / ((Ixy[c] * Ixy[c] + Iyy[c] * Iyy[c]) + kFrZeta2);
    s0 = s0 + (n0[c] * Iz[c]) * Iz[c];
    sg = sg + ((n1[c] * Ixz[c]) * Ixz[c] + (n2[c] * Iyz[c]) * Iyz[c]);
  }
  const float q0 = in ? (a.delta * 0.5f) / sqrtf(s0 / 3.0f + kFrEps2) : 0.0f;
  const float qg = in ? (a.gamma * 0.5f) / sqrtf(sg / 3.0f + kFrEps2) : 0.0f;
  float a11 = 0.0f, a12 = 0.0f, a22 = 0.0f, b1 = 0.0f, b2 = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float w0 = q0 * n0[c];
    a11 = a11 + (w0 * (Ix[c] * Ix[c]) + qg * (n1[c] * (Ixx[c] * Ixx[c]) + n2[c] * (Ixy[c] * Ixy[c])));
    a12 = a12 + (w0 * (Ix[c] * Iy[c]) + qg * (n1[c] * (Ixx[c] * Ixy[c]) + n2[c] * (Ixy[c] * Iyy[c])));
    a22 = a22 + (w0 * (Iy[c] * Iy[c]) + qg * (n1[c] * (Ixy[c] * Ixy[c]) + n2[c] * (Iyy[c] * Iyy[c])));
    b1 = b1 + (w0 * (Ix[c] * Iz[c]) + qg * (n1[c] * (Ixx[c] * Ixz[c]) + n2[c] * (Ixy[c] * Iyz[c])));
    b2 = b2 + (w0 * (Iy[c] * Iz[c]) + qg * (n1[c] * (Ixy[c] * Ixz[c]) + n2[c] * (Iyy[c] * Iyz[c])));
  }
  const int ci = fr_ci(X, Y, a.w, a.h);
  a.a11[ci] = a11 / 3.0f;
  a.a12[ci] = a12 / 3.0f;
  a.a22[ci] = a22 / 3.0f;
  a.b1[ci] = -(b1 / 3.0f);
  a.b2[ci] = -(b2 / 3.0f);
  const float ha = a.alpha * 0.5f;
  const float sm = fr_smooth(tu, tv, cx, cy, ha);
  a.wr[i] = X < a.w - 1 ? 0.5f * (sm + fr_smooth(tu, tv, cx + 1, cy, ha)) : 0.0f;
  a.wd[i] = Y < a.h - 1 ? 0.5f * (sm + fr_smooth(tu, tv, cx, cy + 1, ha)) : 0.0f;
  a.du[i] = 0.0f;
  a.dv[i] = 0.0f;
}

// One half-sweep. A lane owns one pixel of the active colour: x = 2 p + ((y + COLOUR) & 1). The reads of du / dv / u / v
// of a wave cover whole lines (the pixel and its two row neighbours alternate), and so do those of the coefficient
// planes, which are compacted by colour; only wd is read at stride 2.
template <int COLOUR>
__device__ __forceinline__ void fr_sor_body(FrArgs a) {
  const int Y = blockIdx.y * kWaves + (threadIdx.x >> 6);
  if (Y >= a.h) return;
  const int X = 2 * (blockIdx.x * 64 + (threadIdx.x & 63)) + ((Y + COLOUR) & 1);
  if (X >= a.w) return;
  const int i = Y * a.w + X;
  const bool hl = X > 0, hr = X < a.w - 1, hu = Y > 0, hd = Y < a.h - 1;
  const int il = hl ? i - 1 : i, ir = hr ? i + 1 : i, iu = hu ? i - a.w : i, id = hd ? i + a.w : i;
  const float wl = hl ? a.wr[il] : 0.0f, wr = hr ? a.wr[i] : 0.0f;
  const float wu = hu ? a.wd[iu] : 0.0f, wd = hd ? a.wd[i] : 0.0f;
  const float sw = ((wl + wr) + wu) + wd;
  const int c = fr_ci(X, Y, a.w, a.h);
  const float u = a.u[i], du = a.du[i], dv = a.dv[i], a12 = a.a12[c];
  const float tl = hl ? wl * (a.u[il] + a.du[il]) : 0.0f, tr = hr ? wr * (a.u[ir] + a.du[ir]) : 0.0f;
  const float tu = hu ? wu * (a.u[iu] + a.du[iu]) : 0.0f, td = hd ? wd * (a.u[id] + a.du[id]) : 0.0f;
  const float su = ((tl + tr) + tu) + td;
  const float om = a.omega;
  const float dun = (1.0f - om) * du + om * ((((a.b1[c] - a12 * dv) + su) - sw * u) / (a.a11[c] + sw));
  a.du[i] = dun;
  if (a.x_only) return;
  const float v = a.v[i];
  const float sl = hl ? wl * (a.v[il] + a.dv[il]) : 0.0f, sr = hr ? wr * (a.v[ir] + a.dv[ir]) : 0.0f;
  const float st = hu ? wu * (a.v[iu] + a.dv[iu]) : 0.0f, sd = hd ? wd * (a.v[id] + a.dv[id]) : 0.0f;
  const float sv = ((sl + sr) + st) + sd;
  a.dv[i] = (1.0f - om) * dv + om * ((((a.b2[c] - a12 * dun) + sv) - sw * v) / (a.a22[c] + sw));
}

// step 6 of the last outer iteration, into the interleaved result; u and v keep the last outer iteration's field
__device__ __forceinline__ void fr_final_body(FrArgs a, float2 *__restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.w * a.h) return;
  const float v = a.v[i];
  out[i] = make_float2(a.u[i] + a.du[i], a.x_only ? v : v + a.dv[i]);
}

// The kernels: each body on member m's arguments.
struct FrIo {
  const float2 *f0[kSetMax];  // per member the field a run starts from ...
  float2 *out[kSetMax];       // ... and its result
};
using FrSet = SetArgs<FrArgs>;
static_assert(sizeof(SetArgs<FrArgsT<3>>) <= kKernargLimit && sizeof(FrSet) + sizeof(FrIo) <= kKernargLimit,
              "the argument block of a set exceeds the kernel-argument limit");
__global__ __launch_bounds__(kBlock) void k_fr_init(FrSet s, FrIo io, int n) {
  const int m = blockIdx.y;
  fr_init_body(io.f0[m], s.m[m].u, s.m[m].v, n);
}
template <int NCH>
__global__ __launch_bounds__(kBlock) void k_fr_warp(SetArgs<FrArgsT<NCH>> s, int fold) {
  fr_warp_body<NCH>(s.m[blockIdx.z], fold);
}
__global__ __launch_bounds__(kBlock) void k_fr_coef(SetArgs<FrArgsT<1>> s) { fr_coef_body(s.m[blockIdx.z]); }
__global__ __launch_bounds__(kBlock) void k_fr_coef_rgb(SetArgs<FrArgsT<3>> s) { fr_coef_rgb_body(s.m[blockIdx.z]); }
template <int COLOUR>
__global__ __launch_bounds__(kBlock) void k_fr_sor(FrSet s) {
  fr_sor_body<COLOUR>(s.m[blockIdx.z]);
}
__global__ __launch_bounds__(kBlock) void k_fr_final(FrSet s, FrIo io) {
  const int m = blockIdx.y;
  fr_final_body(s.m[m], io.out[m]);
}

}  // namespace ictr

using namespace ictr;

// ---------------------------------------------------------------- C-ABI
constexpr int kFrPlanes = 12;  // u v du dv bw a11 a12 a22 b1 b2 wr wd (the enum below)
struct ictr_flowrefine {
  int w = 0, h = 0;
  float alpha = 16.0f, gamma = 13.0f, delta = 4.5f, omega = 1.6f;
  int n_outer = 8, n_sor = 5;
  int timing = 0;
  float *plane[kFrPlanes] = {};
  float *f0 = nullptr;    // interleaved [h][w][2]: the source formed or copied here
  DevBuf<float> arena;    // everything above, then the result
  std::vector<Event> ev;  // timing: four per outer iteration and four around init and final
  int nev = 0;            // events recorded by the last run
  DenseResult res;        // last: its destructor waits for a run in flight
};
enum { FR_U, FR_V, FR_DU, FR_DV, FR_BW, FR_A11, FR_A12, FR_A22, FR_B1, FR_B2, FR_WR, FR_WD };
// ictr_flowrefine_read_stage's `which` -> plane
static const int kFrStage[ICTR_FLOWREFINE_STAGES] = {FR_BW, FR_A11, FR_A12, FR_A22, FR_B1, FR_B2, FR_WR, FR_WD, FR_DU, FR_DV,
                                                     FR_U,  FR_V};

static bool fr_compacted(int plane) { return plane >= FR_A11 && plane <= FR_B2; }  // stored in fr_ci's order
static size_t fr_plane_floats(const ictr_flowrefine *r) { return (size_t)2 * ((r->w + 1) / 2) * r->h; }

// the working planes and the parameters; Bw of channel 0 is the refiner's own
template <int NCH>
static FrArgsT<NCH> fr_args(const ictr_flowrefine *r, int x_only) {
  FrArgsT<NCH> a;
  memset(&a, 0, sizeof(a));
  a.w = r->w;
  a.h = r->h;
  a.u = r->plane[FR_U];
  a.v = r->plane[FR_V];
  a.du = r->plane[FR_DU];
  a.dv = r->plane[FR_DV];
  a.bw[0] = r->plane[FR_BW];
  a.a11 = r->plane[FR_A11];
  a.a12 = r->plane[FR_A12];
  a.a22 = r->plane[FR_A22];
  a.b1 = r->plane[FR_B1];
  a.b2 = r->plane[FR_B2];
  a.wr = r->plane[FR_WR];
  a.wd = r->plane[FR_WD];
  a.alpha = r->alpha;
  a.gamma = r->gamma;
  a.delta = r->delta;
  a.omega = r->omega;
  a.x_only = x_only ? 1 : 0;
  return a;
}
// one half-sweep of n refiners of r's size
static void fr_half_sweep(const ictr_flowrefine *r, const FrSet &a, int n, int colour, hipStream_t s) {
  dim3 g = pixel_rows_grid((r->w + 1) / 2, r->h);
  g.z = n;
  if (colour == 0)
    hipLaunchKernelGGL(k_fr_sor<0>, g, dim3(kBlock), 0, s, a);
  else
    hipLaunchKernelGGL(k_fr_sor<1>, g, dim3(kBlock), 0, s, a);
}

extern "C" void ictr_flowrefine_destroy(ictr_flowrefine *r) { delete r; }
extern "C" int ictr_flowrefine_create(ictr_flowrefine **out, int w, int h) {
  if (!out || w < 4 || h < 4 || w > 32768 || h > 32768)  // (pixel indices are int, rows / 4 a grid dimension)
    return fail(ICTR_ERR_INVALID, "flowrefine: bad arguments (4 <= w, h <= 32768)");
  if (int rc = need_device()) return rc;
  auto r = std::make_unique<ictr_flowrefine>();
  r->w = w;
  r->h = h;
  const size_t n = fr_plane_floats(r.get());  // a plane: two colours of ceil(w / 2) x h (fr_ci)
  if (int rc = r->arena.alloc(sizeof(float) * n * (kFrPlanes + 4), true)) return rc;
  for (int k = 0; k < kFrPlanes; ++k) r->plane[k] = r->arena.get() + n * k;
  r->f0 = r->arena.get() + n * kFrPlanes;
  if (int rc = r->res.bind(r->f0 + 2 * n, w, h)) return rc;
  *out = r.release();
  return ICTR_OK;
}
extern "C" int ictr_flowrefine_set_params(ictr_flowrefine *r, float alpha, float gamma, float delta, int n_outer, int n_sor,
                                          float omega) {
  if (!r) return fail(ICTR_ERR_INVALID, "flowrefine is NULL");
  if (!isfinite(alpha) || !isfinite(gamma) || !isfinite(delta) || !isfinite(omega) || !(alpha > 0.0f) || gamma < 0 ||
      delta < 0 || n_outer < 0 || n_sor < 0 || n_outer > 1024 || n_sor > 1024 || !(omega > 0.0f) || !(omega < 2.0f))
    return fail(ICTR_ERR_INVALID,
                "flowrefine_set_params: finite alpha > 0, gamma, delta >= 0, 0 <= n_outer, n_sor <= 1024, 0 < omega < 2");
  r->alpha = alpha;
  r->gamma = gamma;
  r->delta = delta;
  r->n_outer = n_outer;
  r->n_sor = n_sor;
  r->omega = omega;
  return ICTR_OK;
}
extern "C" int ictr_flowrefine_set_timing(ictr_flowrefine *r, int on) {
  if (!r) return fail(ICTR_ERR_INVALID, "flowrefine is NULL");
  r->timing = on ? 1 : 0;
  return ICTR_OK;
}

// fr_args and the frames' planes of a run on level `level` of NCH pyramids per frame (the refiner of that level's size);
// bw12 (NCH = 3): Bw of channels 1 and 2, [2][h][w]
template <int NCH>
static int fr_frame_args(const ictr_flowrefine *r, const ictr_pyramid *const *pyr_a, const ictr_pyramid *const *pyr_b,
                         int x_only, int level, float *bw12, FrArgsT<NCH> *a) {
  *a = fr_args<NCH>(r, x_only);
  for (int c = 0; c < NCH; ++c) {
    ictr_level0 l[2];
    for (int k = 0; k < 2; ++k) {
      if (int rc = ictr_pyramid_level0(k ? pyr_b[c] : pyr_a[c], "flowrefine_run", &l[k], level)) return rc;
      if (l[k].w != r->w || l[k].h != r->h)
        return fail(ICTR_ERR_INVALID, "flowrefine_run: a pyramid is %d x %d, the refiner %d x %d", l[k].w, l[k].h, r->w, r->h);
    }
    if (c > 0 && (l[0].stride != a->sa || l[1].stride != a->sb))
      return fail(ICTR_ERR_INVALID, "flowrefine_run: the channels' planes differ in stride");
    a->A[c] = l[0].img, a->sa = l[0].stride;
    a->B[c] = l[1].img, a->sb = l[1].stride;
    if (c > 0) a->bw[c] = bw12 + (size_t)(c - 1) * r->w * r->h;
  }
  return ICTR_OK;
}

// The launch sequence of a run of n refiners of one size and one set of parameters, each stage once, on level `level` of
// NCH pyramids per member and frame. Member m starts from the device field field[m] [h][w][2] and reads the pyramids
// pyr_a[m * NCH + c], pyr_b[m * NCH + c]; bw12[m] as in fr_frame_args. ev (NULL: untimed): the events of a timed run, one
// recorded at every mark; *nev takes their number. No member's result event is recorded: that is the caller's to do behind
// the run. *ops takes the launches (and, with n_outer = 0, the copies, one per member) enqueued.
template <int NCH>
static int fr_run(ictr_flowrefine *const *r, const ictr_pyramid *const *pyr_a, const ictr_pyramid *const *pyr_b, int n,
                  const float *const *field, int x_only, int level, float *const *bw12, int *ops,
                  const std::vector<Event> *ev, int *nev, hipStream_t s) {
  SetArgs<FrArgsT<NCH>> a;
  FrSet g;  // of the half-sweeps, k_fr_init and k_fr_final
  FrIo io;
  memset(&a, 0, sizeof(a));
  memset(&g, 0, sizeof(g));
  memset(&io, 0, sizeof(io));
  const ictr_flowrefine *r0 = r[0];
  for (int m = 0; m < n; ++m) {
    if (!r[m] || !field[m] || (NCH == 3 && !bw12[m]))
      return fail(ICTR_ERR_INVALID, "flowrefine_run: member %d: the refiner, the field or the Bw planes are NULL", m);
    if (r[m]->w != r0->w || r[m]->h != r0->h || r[m]->n_outer != r0->n_outer || r[m]->n_sor != r0->n_sor)
      return fail(ICTR_ERR_INVALID, "flowrefine_run: member %d differs in size or iteration counts", m);
    if (int rc = fr_frame_args<NCH>(r[m], pyr_a + m * NCH, pyr_b + m * NCH, x_only, level, bw12[m], &a.m[m])) return rc;
    g.m[m] = fr_args<1>(r[m], x_only);
    io.f0[m] = reinterpret_cast<const float2 *>(field[m]);
    io.out[m] = reinterpret_cast<float2 *>(r[m]->res.get());
  }
  const size_t np = (size_t)r0->w * r0->h;
  int count = 0, marks = 0;
  auto mark = [&]() {
    if (ev) (void)hipEventRecord((*ev)[marks++].get(), s);
  };
  if (r0->n_outer == 0) {  // the input's bits
    for (int m = 0; m < n; ++m, ++count)
      HIPCHK(hipMemcpyAsync(r[m]->res.get(), field[m], sizeof(float) * 2 * np, hipMemcpyDeviceToDevice, s));
  } else {
    const dim3 blk(kBlock), lin((unsigned)((np + kBlock - 1) / kBlock), n);
    const dim3 tiles((r0->w + kFrTile - 1) / kFrTile, (r0->h + kFrTile - 1) / kFrTile, n);
    dim3 rows = pixel_rows_grid(r0->w, r0->h);
    rows.z = n;
    mark();
    hipLaunchKernelGGL(k_fr_init, lin, blk, 0, s, g, io, (int)np);
    mark();
    for (int o = 0; o < r0->n_outer; ++o) {
      mark();
      hipLaunchKernelGGL(k_fr_warp<NCH>, rows, blk, 0, s, a, o > 0 ? 1 : 0);
      mark();
      if constexpr (NCH == 1)
        hipLaunchKernelGGL(k_fr_coef, tiles, blk, 0, s, a);
      else
        hipLaunchKernelGGL(k_fr_coef_rgb, tiles, blk, 0, s, a);
      mark();
      for (int k = 0; k < r0->n_sor; ++k) {
        fr_half_sweep(r0, g, n, 0, s);
        fr_half_sweep(r0, g, n, 1, s);
      }
      mark();
    }
    mark();
    hipLaunchKernelGGL(k_fr_final, lin, blk, 0, s, g, io);
    mark();
    count = 2 + r0->n_outer * (2 + 2 * r0->n_sor);
  }
  HIPCHK(hipGetLastError());
  for (int m = 0; m < n; ++m) r[m]->nev = 0;
  if (ops) *ops = count;
  if (nev) *nev = marks;
  return ICTR_OK;
}
// the coarse-to-fine flow's run (ictr_launch.h): `channels` (1 or 3, the caller's to keep) pyramids per member and frame,
// the fields on the device; untimed (the stage's events are the caller's)
extern "C" int ictr_flowrefine_run_level_(ictr_flowrefine *const *r, const ictr_pyramid *const *pyr_a,
                                          const ictr_pyramid *const *pyr_b, int n, int channels, const float *const *field,
                                          int x_only, int level, float *const *bw12, int *ops, void *hip_stream) {
  if (!r || !r[0] || !pyr_a || !pyr_b || !field || !bw12 || n < 1 || n > kSetMax)
    return fail(ICTR_ERR_INVALID, "flowrefine_run: bad arguments");
  hipStream_t s = (hipStream_t)hip_stream;
  return channels == 3 ? fr_run<3>(r, pyr_a, pyr_b, n, field, x_only, level, bw12, ops, nullptr, nullptr, s)
                       : fr_run<1>(r, pyr_a, pyr_b, n, field, x_only, level, bw12, ops, nullptr, nullptr, s);
}

// a refiner's own run: a set of one at level 0, with the events of a timed run and its result event behind
extern "C" int ictr_flowrefine_run(ictr_flowrefine *r, const ictr_pyramid *pyr_a, const ictr_pyramid *pyr_b,
                                   const ictr_field *src, int x_only, void *hip_stream) {
  if (!r) return fail(ICTR_ERR_INVALID, "flowrefine is NULL");
  if (!src || !src->data) return fail(ICTR_ERR_INVALID, "flowrefine_run: the field (or its data) is NULL");
  if (src->sign != 1) return fail(ICTR_ERR_INVALID, "flowrefine_run: the field's sign is %d (+1)", src->sign);
  FrArgsT<1> a;  // (the frames' refusals come before the field's, and before anything is enqueued)
  if (int rc = fr_frame_args<1>(r, &pyr_a, &pyr_b, x_only, 0, nullptr, &a)) return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  const size_t n = (size_t)r->w * r->h;
  const float *f0 = r->f0;
  if (src->kind == ICTR_FIELD_GRID) {
    FgDev g;
    if (int rc = ictr_flowgrid_view_(static_cast<const ictr_flowgrid *>(src->data), &g)) return rc;
    if (g.w != r->w || g.h != r->h)
      return fail(ICTR_ERR_INVALID, "flowrefine_run: the flow grid is %d x %d, the refiner %d x %d", g.w, g.h, r->w, r->h);
    launch_fg_dense(g, reinterpret_cast<float2 *>(r->f0), s);
  } else if (src->kind == ICTR_FIELD_FLOW) {
    if (src->on_device) {
      f0 = static_cast<const float *>(src->data);
    } else {
      const float *f = static_cast<const float *>(src->data);
      for (size_t i = 0; i < 2 * n; ++i)
        if (!isfinite(f[i])) return fail(ICTR_ERR_INVALID, "flowrefine_run: the host field is not finite at float %zu", i);
      if (int rc = r->res.settle()) return rc;  // the last run has read f0
      HIPCHK(hipMemcpyAsync(r->f0, f, sizeof(float) * 2 * n, hipMemcpyHostToDevice, s));
      HIPCHK(hipStreamSynchronize(s));  // the caller's array is free when this returns; the kernels follow on s
    }
  } else {
    return fail(ICTR_ERR_INVALID, "flowrefine_run: field kind %d (ICTR_FIELD_FLOW or _GRID)", src->kind);
  }
  const int want = r->timing ? 4 * (r->n_outer + 1) : 0;
  while ((int)r->ev.size() < want) {
    r->ev.emplace_back();
    if (int rc = r->ev.back().create()) return rc;
  }
  float *const no_bw12 = nullptr;
  int nev = 0;
  if (int rc = fr_run<1>(&r, &pyr_a, &pyr_b, 1, &f0, x_only, 0, &no_bw12, nullptr, r->timing ? &r->ev : nullptr, &nev, s))
    return rc;
  r->nev = nev;
  return r->res.record(s);
}

// the parameters a set compares its members' refiners by
extern "C" int ictr_flowrefine_get_params_(const ictr_flowrefine *r, float *p4, int *n2) {
  if (!r || !p4 || !n2) return fail(ICTR_ERR_INVALID, "flowrefine is NULL");
  p4[0] = r->alpha, p4[1] = r->gamma, p4[2] = r->delta, p4[3] = r->omega;
  n2[0] = r->n_outer, n2[1] = r->n_sor;
  return ICTR_OK;
}

extern "C" int ictr_flowrefine_result(ictr_flowrefine *r, float *out, int on_device) {
  if (!r) return fail(ICTR_ERR_INVALID, "flowrefine is NULL");
  return r->res.copy_out("flowrefine_result", out, on_device);
}
extern "C" const float *ictr_flowrefine_device_ptr(const ictr_flowrefine *r) { return r ? r->res.get() : nullptr; }
extern "C" int ictr_flowrefine_get_kernel_times(ictr_flowrefine *r, float *ms) {
  if (!r) return fail(ICTR_ERR_INVALID, "flowrefine is NULL");
  if (int rc = r->res.wait("flowrefine_get_kernel_times")) return rc;
  if (!ms) return fail(ICTR_ERR_INVALID, "flowrefine_get_kernel_times: ms is NULL");
  ms[0] = ms[1] = ms[2] = ms[3] = 0.0f;
  if (r->nev < 4) return ICTR_OK;  // timing was off, or n_outer = 0
  auto span = [&](int k, float *acc) {
    float v = 0.0f;
    if (hipEventElapsedTime(&v, r->ev[k].get(), r->ev[k + 1].get()) == hipSuccess) *acc += v;
  };
  span(0, &ms[3]);
  for (int o = 0; 2 + 4 * o + 3 < r->nev - 2; ++o) {
    span(2 + 4 * o, &ms[0]);
    span(3 + 4 * o, &ms[1]);
    span(4 + 4 * o, &ms[2]);
  }
  span(r->nev - 2, &ms[3]);
  return ICTR_OK;
}
extern "C" int ictr_flowrefine_read_stage(ictr_flowrefine *r, int which, float *out) {
  if (!r || !out || which < 0 || which >= ICTR_FLOWREFINE_STAGES)
    return fail(ICTR_ERR_INVALID, "flowrefine_read_stage: bad arguments (which is 0..%d)", ICTR_FLOWREFINE_STAGES - 1);
  if (int rc = r->res.settle()) return rc;
  const int k = kFrStage[which];
  if (!fr_compacted(k)) {
    HIPCHK(hipMemcpy(out, r->plane[k], sizeof(float) * (size_t)r->w * r->h, hipMemcpyDeviceToHost));
    return ICTR_OK;
  }
  std::vector<float> tmp(fr_plane_floats(r));
  HIPCHK(hipMemcpy(tmp.data(), r->plane[k], sizeof(float) * tmp.size(), hipMemcpyDeviceToHost));
  for (int Y = 0; Y < r->h; ++Y)
    for (int X = 0; X < r->w; ++X) out[(size_t)Y * r->w + X] = tmp[fr_ci(X, Y, r->w, r->h)];
  return ICTR_OK;
}
extern "C" int ictr_debug_flowrefine_write_stage(ictr_flowrefine *r, int which, const float *in) {
  if (!r || !in || which < 0 || which >= ICTR_FLOWREFINE_STAGES)
    return fail(ICTR_ERR_INVALID, "flowrefine_write_stage: bad arguments (which is 0..%d)", ICTR_FLOWREFINE_STAGES - 1);
  if (int rc = r->res.settle()) return rc;
  const int k = kFrStage[which];
  if (!fr_compacted(k)) {
    HIPCHK(hipMemcpy(r->plane[k], in, sizeof(float) * (size_t)r->w * r->h, hipMemcpyHostToDevice));
    return ICTR_OK;
  }
  std::vector<float> tmp(fr_plane_floats(r), 0.0f);
  for (int Y = 0; Y < r->h; ++Y)
    for (int X = 0; X < r->w; ++X) tmp[fr_ci(X, Y, r->w, r->h)] = in[(size_t)Y * r->w + X];
  HIPCHK(hipMemcpy(r->plane[k], tmp.data(), sizeof(float) * tmp.size(), hipMemcpyHostToDevice));
  return ICTR_OK;
}
extern "C" int ictr_debug_flowrefine_half_sweep(ictr_flowrefine *r, int colour, int x_only) {
  if (!r || (colour != 0 && colour != 1)) return fail(ICTR_ERR_INVALID, "flowrefine_half_sweep: colour is 0 or 1");
  FrSet g;  // a set of one
  memset(&g, 0, sizeof(g));
  g.m[0] = fr_args<1>(r, x_only);
  fr_half_sweep(r, g, 1, colour, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(nullptr));
  return ICTR_OK;
}
