// ictr_kernels.hip -- hand-written HIP kernels (gfx950 / CDNA4, wave64) for the Gauss-Newton photometric tracker.
//
// Reference steps (odometer.cpp:257-426, /root/reference) -> kernels:
//   step 3   project at the reference pose, all levels      k_project_ref      (pose.cpp:307-488)
//   step 4-6 reference patches + gradients, sd coefficients,
//            Hessian                                        k_ref_level        (utilities.cpp:115-189, odometer.cpp:268-334,428-472)
//   step 7-10 project, fetch current patch, residual,
//            J^T r, solve, pose update, loop condition       k_iter             (utilities.cpp:55-113, odometer.cpp:344-418,509-515)
//   pyramid  2x2 box + [-1 0 1] gradients + padding          k_pyr_*            (utilities.cpp:14-52)
//
// Design: memory-bound gather + rank-1 accumulate, no MFMA. One wave64 owns one 8x8 patch
// (four 4x4 patches): the 64 lanes ARE the 64 patch pixels, so T/Gx/Gy are read as 256-B coalesced rows, the
// bilinear taps are 8 x 32-B row segments, and the six J^T r sums live in per-lane registers across all the
// patches a wave visits -- one shuffle reduction per wave per launch, not per patch. The steepest-descent
// images of the reference (6 planes + 6 projected planes, re-zeroed every iteration) are never materialised:
// a patch carries 12 scalar coefficients. Every workgroup leaves one partial sum per component; a second, tiny
// launch (one workgroup per problem: k_level_tail / k_iter_tail) adds them in a fixed order in f64, solves the
// 6x6 system and updates the pose on the device, so the host never reads anything back inside the loop and the
// sums are reproducible bit for bit. Doing that reduction inside the big kernel ("last workgroup to arrive")
// was measured and rejected: it needs one agent-scope release (an L2 write-back scan, buffer_wbl2 sc1) per
// workgroup, ~4000 per launch, which throttled the L2 for every wave: 310 us per iteration against 141 us for
// the two-launch form (profiles/r01_notes.md).
//
// Arithmetic parity: compiled with -ffp-contract=off; every expression below keeps the reference's
// operand order, so patches, projections and coefficients are bit-identical to the CPU path; only the
// order of the big sums differs.
#include <algorithm>

#include <hip/hip_ext.h>

#include "ictr_dev.h"
#include "ictr_launch.h"
#include "ictr_devfn.h"
#include "se3_math.h"

namespace ictr {

// ---------------------------------------------------------------- step 3: projection at the reference pose
// pose.cpp:400-488 (save rotated, level lv_f) + pose.cpp:307-397 for the other levels (odometer.cpp:251-254).
// The camera-frame point is level independent, so one pass writes every level.
struct AllCams {
  LevelCam lc[16];
};

__global__ __launch_bounds__(kBlock) void k_project_ref(EngineDev e, AllCams cams) {
  const int b = blockIdx.y;
  const ProbState &st = e.st[b];
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i == 0 && b == 0 && e.trace.count != nullptr) *e.trace.count = 0;  // the tracking's trace starts here (begin phase)
  if (i >= st.npts) return;
  const float *p3 = e.pt3d + (size_t)b * 3 * e.M;
  float *p3r = e.pt3d_ref + (size_t)b * 3 * e.M;
  const float X = p3[i], Y = p3[i + e.M], Z = p3[i + 2 * e.M];
  float tx, ty, tz;
  rotate_point(st.G, X, Y, Z, tx, ty, tz);
  p3r[i] = tx;
  p3r[i + e.M] = ty;
  p3r[i + 2 * e.M] = tz;
  for (int l = e.lv_l; l <= e.lv_f; ++l) {
    float *p2 = e.pt2d + ((size_t)b * e.nlev + l) * 2 * e.M;
    project_pinhole(tx, ty, tz, cams.lc[l], p2[i], p2[i + e.M]);
  }
}

// PoseClass::project_pt / project_pt_save_rotated on caller buffers (device copies), SoA stride M
__global__ __launch_bounds__(kBlock) void k_project_generic(const float *__restrict__ pt3d, float *pt3d_rot,
                                                            float *pt2d, int n, int M, const float *__restrict__ G,
                                                            LevelCam lc) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float X = pt3d[i], Y = pt3d[i + M], Z = pt3d[i + 2 * M];
  float tx, ty, tz;
  rotate_point(G, X, Y, Z, tx, ty, tz);
  if (pt3d_rot) {
    pt3d_rot[i] = tx;
    pt3d_rot[i + M] = ty;
    pt3d_rot[i + 2 * M] = tz;
  }
  pt2d[i] = pinhole_axis(tx, tz, lc.fx, lc.cx);  // (stored one by one: pt2d may alias pt3d_rot)
  pt2d[i + M] = pinhole_axis(ty, tz, lc.fy, lc.cy);
}

// ---------------------------------------------------------------- steps 4-6: per level setup (any patch size)
// PT = compile-time patch size (4), or 0 = run-time e.P (any size; a wave loops over the pixels). Writes one
// partial of the 21 unique H entries per workgroup; k_level_tail finishes.
template <int PT>
__global__ __launch_bounds__(kBlock) void k_ref_level(EngineDev e, LevelCam lc, int level) {
  __shared__ float sW[kWaves][kPartHStride];
  const int b = blockIdx.y;
  const ProbState &st = e.st[b];
  const int npts = st.npts;
  const int P = PT ? PT : e.P;
  const int n = P * P;
  const int pszd2 = P / 2;
  const int M = e.M;
  const PlaneSet pl = e.planes[b * e.nlev + level];
  const float *pt2d = e.pt2d + ((size_t)b * e.nlev + level) * 2 * M;
  const float *p3r = e.pt3d_ref + (size_t)b * 3 * M;
  const PatchBufs pb = {e.T + (size_t)b * M * n, e.Gx + (size_t)b * M * n, e.Gy + (size_t)b * M * n};
  float *coefb = e.coef + (size_t)b * M * kCoefStride;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const PatchGeom pg = patch_geom(n, lane);
  const PatchOpts po = {e.dopatchnorm, e.robust, e.huber_k};

  float acc[kHUnique];
#pragma unroll
  for (int j = 0; j < kHUnique; ++j) acc[j] = 0.0f;

  const int nw = gridDim.x * kWaves;
  for (int g = blockIdx.x * kWaves + wave; g * pg.ppw < npts; g += nw) {
    const int i = g * pg.ppw + pg.sub;
    const bool valid = i < npts;
    const float mx = valid ? pt2d[i] : -1.0f;
    const float my = valid ? pt2d[i + M] : -1.0f;
    const bool vis = valid && in_view(mx, my, lc.swo, lc.sho);
    float cx[6], cy[6];
    float4 *c4 = reinterpret_cast<float4 *>(coefb + (size_t)i * kCoefStride);
    if (vis) {
      sd_coefs(p3r[i], p3r[i + M], p3r[i + 2 * M], lc.fx, lc.fy, cx, cy);
      if (pg.q0 == 0) coef_line_store(c4, cx, cy);
    } else if (valid) {  // out of the reference view at this level: keep the stale coefficients (quirk, odometer.cpp:304)
      coef_line_load(c4, cx, cy);
    } else {
#pragma unroll
      for (int k = 0; k < 6; ++k) cx[k] = cy[k] = 0.0f;
    }
    const Taps tp = taps_or_fallback(vis, mx, my, pszd2);
    const int base = tp.row0 * lc.sw + tp.col0;
    setup_patch_body<false>(po, pl.ref, pl.dx, pl.dy, lc.sw, P, n, pg, i, valid, vis, tp, base, cx, cy, pb, pb, acc);
  }

#pragma unroll
  for (int j = 0; j < kHUnique; ++j) {
    const float v = wave_sum(acc[j]);
    if (lane == 0) sW[wave][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < kHUnique) {
    const float v = (sW[0][threadIdx.x] + sW[1][threadIdx.x]) + (sW[2][threadIdx.x] + sW[3][threadIdx.x]);
    e.partH[((size_t)b * gridDim.x + blockIdx.x) * kPartHStride + threadIdx.x] = v;
  }
}

// One workgroup per problem: fixed-order f64 reduction of the H partials of `nblk` workgroups (8 slices x 32
// components, then the slices in order), publish H (or the rank-local sum when sharded), reset the loop state.
// defer_h: the P = 8 fast path accumulates H inside the level's FIRST iteration launch (k_iter8<.., WH = true>: it
// streams Gx, Gy and the coefficients anyway), so the setup kernel is a pure gather/store kernel and this tail only
// resets the loop state; the first k_iter_tail / k_iter_finish of the level reduces and factors H.
// The factorisation and, per iteration, the solve / pose update / loop condition run on ONE wave in registers
// (WaveSolver, ictr_devfn.h) instead of one thread on LDS arrays: 3-4 k cycles instead of ~14 k on the critical path
// between two accumulate launches.
__global__ __launch_bounds__(kBlock) void k_level_tail(EngineDev e, int nblk, int defer_h) {
  __shared__ double sRed[kBlock / 32][32];
  __shared__ float sH[32];
  const int b = blockIdx.x;
  ProbState &st = e.st[b];
  if (defer_h) {
    if (threadIdx.x == 0) level_reset(st, e);
    return;
  }
  reduce_partH<kBlock>(e, b, nblk, sRed, sH);
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  if (e.sharded) {
    if (lane < kHUnique) e.red[(size_t)b * kRedStride + lane] = sH[lane];
  } else {
    WaveSolver S;
    ws_factor(S, sH[h_unique_index(lane)], lane);
    ws_store_factor(S, st, lane);
    if (lane == 0) level_reset(st, e);
  }
}

// sharded mode: adopt the all-reduced H (red[b][0..20]) and reset the iteration state (one wave per problem)
__global__ __launch_bounds__(64) void k_level_finish(EngineDev e, int defer_h) {
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  ProbState &st = e.st[b];
  if (defer_h) {
    if (lane == 0) level_reset(st, e);
    return;
  }
  const float a = e.red[(size_t)b * kRedStride + h_unique_index(lane)];
  __builtin_amdgcn_wave_barrier();
  // leave the slot zeroed: the caller may all-reduce the whole buffer again before it is rewritten
  if (lane < kRedStride) e.red[(size_t)b * kRedStride + lane] = 0.0f;
  WaveSolver S;
  ws_factor(S, a, lane);
  ws_store_factor(S, st, lane);
  if (lane == 0) level_reset(st, e);
}

// inspection (ictr_debug_wave_solve): the solver turn's linear algebra alone, one wave per system. The wave reads the
// 21 upper-triangle values of its H into LDS and feeds ws_factor through h_unique_index, as the tails above do.
// apply = 1: factor and substitute in registers (the one-launch and resident forms); apply = 0: factor and store to
// st[] -- k_debug_wave_apply then reloads the factors in a launch of its own (the per-iteration and sharded forms).
__device__ __forceinline__ void debug_wave_solve_out(const WaveSolver &S, float bi, int sys, int lane, float *x, int *rank,
                                                     int *nonzero, int *rowmap, int *colmap, float *lu) {
  const float xi = ws_apply(S, bi, lane);
  if (lane < 6) {
    x[(size_t)sys * 6 + lane] = xi;
    rowmap[(size_t)sys * 6 + lane] = S.rowmap;
    colmap[(size_t)sys * 6 + lane] = S.colmap;
#pragma unroll
    for (int j = 0; j < 6; ++j) lu[(size_t)sys * 36 + lane * 6 + j] = S.lu[j];
  }
  if (lane == 0) {
    rank[sys] = S.rank;
    nonzero[sys] = S.nonzero;
  }
}
__global__ __launch_bounds__(64) void k_debug_wave_factor(const float *__restrict__ H, const float *__restrict__ b,
                                                          ProbState *st, int apply, float *x, int *rank, int *nonzero,
                                                          int *rowmap, int *colmap, float *lu) {
  __shared__ float sH[32];
  const int sys = blockIdx.x;
  const int lane = threadIdx.x;
  if (lane < 36 && lane / 6 <= lane % 6) sH[h_unique_index(lane)] = H[(size_t)sys * 36 + lane];
  __syncthreads();
  WaveSolver S;
  ws_factor(S, sH[h_unique_index(lane)], lane);
  if (apply)
    debug_wave_solve_out(S, lane < 6 ? b[(size_t)sys * 6 + lane] : 0.0f, sys, lane, x, rank, nonzero, rowmap, colmap, lu);
  else
    ws_store_factor(S, st[sys], lane);
}
__global__ __launch_bounds__(64) void k_debug_wave_apply(const float *__restrict__ b, const ProbState *st, float *x,
                                                         int *rank, int *nonzero, int *rowmap, int *colmap, float *lu) {
  const int sys = blockIdx.x;
  const int lane = threadIdx.x;
  WaveSolver S;
  ws_load_factor(S, st[sys], lane);
  debug_wave_solve_out(S, lane < 6 ? b[(size_t)sys * 6 + lane] : 0.0f, sys, lane, x, rank, nonzero, rowmap, colmap, lu);
}
// inspection (ictr_debug_se3): the device builds of se3_exp<float> (p[6] -> G[12]) and se3_log<float>, one thread each
__global__ __launch_bounds__(64) void k_debug_se3(const float *__restrict__ in, float *__restrict__ out, long long n,
                                                  int log_not_exp) {
  const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  if (log_not_exp) {
    float G[12], p[6];
#pragma unroll
    for (int k = 0; k < 12; ++k) G[k] = in[i * 12 + k];
    se3_log<float>(p, G);
#pragma unroll
    for (int k = 0; k < 6; ++k) out[i * 6 + k] = p[k];
  } else {
    float G[12], p[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) p[k] = in[i * 6 + k];
    se3_exp<float>(G, p);
#pragma unroll
    for (int k = 0; k < 12; ++k) out[i * 12 + k] = G[k];
  }
}

// ---------------------------------------------------------------- steps 7-9a: one Gauss-Newton iteration (any patch size)
template <int PT>
__global__ __launch_bounds__(kBlock) void k_iter(EngineDev e, LevelCam lc, int level) {
  __shared__ float sW[kWaves][kPartBStride];
  const int b = blockIdx.y;
  const ProbState &st = e.st[b];
  if (!st.active) return;  // loop condition of odometer.cpp:344-346, decided on the device by the previous tail
  const int npts = st.npts;
  const int P = PT ? PT : e.P;
  const int n = P * P;
  const int pszd2 = P / 2;
  const int M = e.M;
  const PlaneSet pl = e.planes[b * e.nlev + level];
  const float *__restrict__ p3 = e.pt3d + (size_t)b * 3 * M;
  const PatchBufs pb = {e.T + (size_t)b * M * n, e.Gx + (size_t)b * M * n, e.Gy + (size_t)b * M * n};
  const float *__restrict__ coefb = e.coef + (size_t)b * M * kCoefStride;

  float G[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) G[k] = st.G[k];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const PatchGeom pg = patch_geom(n, lane);
  const PatchOpts po = {e.dopatchnorm, e.robust, e.huber_k};

  float acc[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) acc[k] = 0.0f;

  const int nw = gridDim.x * kWaves;
  for (int g = blockIdx.x * kWaves + wave; g * pg.ppw < npts; g += nw) {
    const int i = g * pg.ppw + pg.sub;
    const bool valid = i < npts;
    const float X = valid ? p3[i] : 0.0f, Y = valid ? p3[i + M] : 0.0f, Z = valid ? p3[i + 2 * M] : 1.0f;
    const IterPoint pt = iter_point(G, X, Y, Z, lc, valid, pszd2);
    float cx[6], cy[6];
    coef_line_load(reinterpret_cast<const float4 *>(coefb + (size_t)(valid ? i : 0) * kCoefStride), cx, cy);
    const int base = pt.tp.row0 * lc.sw + pt.tp.col0;
    iter_patch_body(po, pl.cur, lc.sw, P, n, pg, i, pt.vis, pt.tp, base, cx, cy, pb, acc);
  }

#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const float v = wave_sum(acc[k]);
    if (lane == 0) sW[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const float v = (sW[0][threadIdx.x] + sW[1][threadIdx.x]) + (sW[2][threadIdx.x] + sW[3][threadIdx.x]);
    e.partb[((size_t)b * gridDim.x + blockIdx.x) * kPartBStride + threadIdx.x] = v;
  }
}

// One workgroup per problem: fixed-order f64 reduction of the b partials (32 slices x 8 components, then the
// slices in order) and steps 9b-10 (solve, pose update, loop condition) on wave 0 -- or, when the points are sharded
// over ranks, just the rank-local sums into red[] for the all-reduce.
__global__ __launch_bounds__(kBlock) void k_iter_tail(EngineDev e, int level, int nblk, int first_h) {
  __shared__ double sRed[kBlock / 8][8];
  __shared__ double sRedH[kBlock / 32][32];
  __shared__ float sH[32];
  const int b = blockIdx.x;
  ProbState &st = e.st[b];
  if (!st.active) return;
  // deferred H: the launch before this one also wrote the H partials (workgroup-uniform branch)
  if (first_h) reduce_partH<kBlock>(e, b, nblk, sRedH, sH);
  {
    const int j = threadIdx.x & 7, sl = threadIdx.x >> 3;
    double s = 0.0;
    const float *pb = e.partb + (size_t)b * nblk * kPartBStride + j;
    if (j < 6) {
#pragma unroll 8
      for (int k = sl; k < nblk; k += kBlock / 8) s += (double)pb[(size_t)k * kPartBStride];
    }
    sRed[sl][j] = s;
  }
  __syncthreads();
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  double bs = 0.0;
  if (lane < 6) {
#pragma unroll
    for (int sl = 0; sl < kBlock / 8; ++sl) bs += sRed[sl][lane];
  }
  if (e.sharded) {
    if (first_h && lane < kHUnique) e.red[(size_t)b * kRedStride + lane] = sH[lane];
    if (lane < 6) e.red[(size_t)b * kRedStride + kHUnique + lane] = (float)bs;
    return;
  }
  WaveSolver S;
  float G[12];
  ws_load_state(S, st, lane, G);
  if (first_h) {
    ws_factor(S, sH[h_unique_index(lane)], lane);
    ws_store_factor(S, st, lane);
  } else {
    ws_load_factor(S, st, lane);
  }
  ws_iterate(S, (float)bs, solve_opts(e), level, b, lane, G);
  ws_store_state(S, st, lane, G);
}

// sharded mode: steps 9b-10 on the all-reduced b (red[b][21..26]); every rank does the same arithmetic
// (one wave per problem)
__global__ __launch_bounds__(64) void k_iter_finish(EngineDev e, int level, int first_h) {
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  ProbState &st = e.st[b];
  if (!st.active) return;
  WaveSolver S;
  float G[12];
  ws_load_state(S, st, lane, G);
  float a = 0.0f, bi = 0.0f;
  if (first_h) a = e.red[(size_t)b * kRedStride + h_unique_index(lane)];  // deferred H: adopt the all-reduced sums
  if (lane < 6) bi = e.red[(size_t)b * kRedStride + kHUnique + lane];
  __builtin_amdgcn_wave_barrier();
  if (lane < kRedStride && (first_h || lane >= kHUnique)) e.red[(size_t)b * kRedStride + lane] = 0.0f;
  if (first_h) {
    ws_factor(S, a, lane);
    ws_store_factor(S, st, lane);
  } else {
    ws_load_factor(S, st, lane);
  }
  ws_iterate(S, bi, solve_opts(e), level, b, lane, G);
  ws_store_state(S, st, lane, G);
}

// ================================================================ P = 8 fast path (wave64 == one 8x8 patch)
// Two stages per chunk of up to 64 consecutive points owned by one wave:
//   stage 1  one POINT per lane: coalesced reads of the point arrays; projection / visibility / bilinear weights /
//            tap base index computed once per point (not 64x redundantly per patch), in the reference's exact
//            arithmetic; the per-point constants go into a wave-private LDS record;
//   stage 2  one PATCH per step, the lanes are its 64 pixels: T/Gx/Gy are 256-B coalesced rows with a scalar
//            base, the frame window is read with every cache line requested once, the per-patch constants come
//            back from LDS as broadcast ds_read_b128. The steps are software-pipelined (double-buffered
//            registers): the loads of step s+1 are in flight while step s is reduced.
// XCD-aware workgroup order. The hardware deals consecutive workgroup ids round-robin to the 8 XCDs, each with its
// own L2. Re-labelling id -> (id % 8) * (n / 8) + id / 8 gives every XCD a contiguous band of chunks, so neighbouring
// chunks (which share frame cache lines at their borders) meet in one L2 instead of being fetched twice from the
// fabric. Needs a grid that is a multiple of 8 (the launchers round up; surplus workgroups find no chunk).
__device__ __forceinline__ int xcd_band_block(int bx, int gx) { return (gx & 7) ? bx : (bx & 7) * (gx >> 3) + (bx >> 3); }

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef const f32x4_t __attribute__((address_space(1))) *gconst_f32x4;

// Packed taps: the setup kernel gathers the SAME 9x9 window from three planes. With the planes interleaved as one
// {img, dx, dy, 0} texel per pixel a window row is 144 contiguous bytes (2 cache lines) instead of 3 x 36 bytes in
// 3-6 lines, and two 16-byte loads per lane replace three 8-byte ones. Measured reason: the three separate gathers
// pulled ~7 KB of lines per patch through an L1 that cannot hold the 20 waves' windows, and the kernel ran at the
// L2's pace, not HBM's (ablations in profiles/r01_notes.md).
struct TapLoads4 {
  f32x4_t l, r, tl, tr;  // texels at (x-1, y), (x, y) and, for lanes 0-7, the row above
};
__device__ __forceinline__ TapLoads4 taps_issue4(gconst_f32x4 pack_at_base, int loff, int sw, int lane) {
  TapLoads4 t;
  t.l = pack_at_base[loff - 1];
  t.r = pack_at_base[loff];
  f32x4_t z = {0.0f, 0.0f, 0.0f, 0.0f};
  t.tl = z;
  t.tr = z;
  if (lane < 8) {
    t.tl = pack_at_base[loff - sw - 1];
    t.tr = pack_at_base[loff - sw];
  }
  return t;
}
// same operand order as taps_blend (utilities.cpp:107), plane k of the texels
__device__ __forceinline__ float taps_blend4(const TapLoads4 &t, int k, float w0, float w1, float w2, float w3, int lane) {
  const float a = t.r[k], b = t.l[k];
  const float cu = __shfl_up(a, 8, 64), du = __shfl_up(b, 8, 64);
  const float c = lane < 8 ? t.tr[k] : cu, d = lane < 8 ? t.tl[k] : du;
  return w0 * a + w1 * b + w2 * c + w3 * d;
}

template <int kU>
struct PatchLoads {  // raw load results of one stage-2 step of kU patches (consumers belong to the reduce phase)
  float t[kU], gx[kU], gy[kU];
  TapLoads cur[kU];  // .ab = (x-1,y),(x,y) and .top = (x-1,y-1),(x,y-1) of the lane's own pixel
  int rec[kU];       // LDS record index of the patch, or 64 (the zero record) for the padding of a partial step
};

// Stage-2 addressing (what survived round 2's A/B runs, profiles/r02_notes.md): buffer loads -- plane / patch-buffer
// descriptor in SGPRs, wave-uniform offset in an SGPR, per-lane constant byte offset in a VGPR, no vector address
// arithmetic per load; every lane loads its own two row pairs (x-1,x at y and y-1): no cross-lane traffic, no selects,
// neighbouring lanes' requests hit the same cache lines. The LDS record of a point is
// [w1 w0 w3 w2][cx2..5][cy2..5][cx0 cy1 vis -]: four ds_read_b128 at one address, operands already paired for the packed
// multiply-adds; the window's byte offset is computed per POINT in stage 1 (one v_readlane per patch); the padding of a
// partial pipeline step points at a zero record (an exact zero contribution to b) instead of being branched around.
// A wave issues at most one instruction of any kind per ~4 cycles, so at the coarse levels (frames cached) the
// kernel's pace is its instruction count per patch, not bytes.
// (H is no longer summed here: the setup kernel k_ref8 leaves the level's H partials, from three sums per patch.)
template <bool PN, int kU>
__global__ __launch_bounds__(kBlock) void k_iter8(EngineDev e, LevelCam lc, int level, int cpw) {
  __shared__ __attribute__((aligned(16))) float sRec[kWaves][65 * kRec];  // record 64: zeros
  __shared__ float sW[kWaves][kPartBStride];
  const int b = blockIdx.y;
  const ProbState &st = e.st[b];
  if (!st.active) return;
  const int npts = st.npts;
  const int M = e.M;
  const PlaneSet pl = e.planes[b * e.nlev + level];
  const float *__restrict__ p3 = e.pt3d + (size_t)b * 3 * M;
  const float *__restrict__ T = e.T + (size_t)b * M * 64;
  const float *__restrict__ Gx = e.Gx + (size_t)b * M * 64;
  const float *__restrict__ Gy = e.Gy + (size_t)b * M * 64;
  const float *__restrict__ coefb = e.coef + (size_t)b * M * kCoefStride;
  const int sw = lc.sw;
  // buffer descriptors (base, no stride, max range, raw dword format) of the current frame and the patches
  const __amdgpu_buffer_rsrc_t rcur = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(pl.cur), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rT = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(T), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rGx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(Gx), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rGy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(Gy), 0, 0x7fffffff, 0x00020000);

  float G[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) G[k] = st.G[k];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float *rec = sRec[wave];
  const float4 *rec4 = reinterpret_cast<const float4 *>(rec);
  if (lane < kRec) rec[64 * kRec + lane] = 0.0f;  // (first read behind stage 1's wave barrier)

  f32x2_t acc01 = {0.0f, 0.0f}, acc23 = {0.0f, 0.0f}, acc45 = {0.0f, 0.0f};  // the six J^T r sums as register pairs

  const int nchunks = (npts + cpw - 1) / cpw;
  for (int ch = xcd_band_block(blockIdx.x, gridDim.x) * kWaves + wave; ch < nchunks; ch += gridDim.x * kWaves) {
    const int i0 = ch * cpw;
    const int cnt = min(cpw, npts - i0);
    // ---- stage 1: lane j <-> point i0 + j  (step 7, pose.cpp:384-391; ind_new, odometer.cpp:369-377)
    const bool pv = lane < cnt;
    const int ip = i0 + (pv ? lane : 0);
    const float X = p3[ip], Y = p3[ip + M], Z = p3[ip + 2 * M];
    float cx[6], cy[6];
    coef_line_load(reinterpret_cast<const float4 *>(coefb + (size_t)ip * kCoefStride), cx, cy);
    const IterPoint pt = iter_point(G, X, Y, Z, lc, pv, 4);
    const Taps &tp = pt.tp;
    const int base_v = tp.row0 * sw + tp.col0;
    const int so_v = (base_v - sw - 1) * 4;  // bytes to the window's top-left texel (tap d of pixel 0)
    {
      float4 *r4 = reinterpret_cast<float4 *>(rec + lane * kRec);
      r4[0] = make_float4(tp.w1, tp.w0, tp.w3, tp.w2);
      r4[1] = make_float4(cx[2], cx[3], cx[4], cx[5]);
      r4[2] = make_float4(cy[2], cy[3], cy[4], cy[5]);
      r4[3] = make_float4(cx[0], cy[1], pt.vis ? 1.0f : 0.0f, 0.0f);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // ---- stage 2. The kU patches of a step are nsteps apart (neighbouring points share frame cache lines).
    const int nsteps = (cnt + kU - 1) / kU;
    auto issue = [&](PatchLoads<kU> &L, int sidx) {
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int jraw = sidx + u * nsteps;
        const int jj = min(jraw, cnt - 1);
        constexpr int aux = 2;  // gfx950 cache policy bits of a buffer load: bit 1 = nt (streamed once per launch:
                                // keep them from evicting the re-used frame lines)
        L.rec[u] = (jraw < cnt) ? jj : 64;  // padding: the zero record; its loads repeat the chunk's last patch
        const int so = rlane(so_v, jj);
        const int po4 = (i0 + jj) * 256;  // bytes: one 8x8 float patch = 256 B
        const int off_cd = ((lane >> 3) * sw + (lane & 7)) * 4, off_ab = off_cd + sw * 4;
        L.t[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rT, lane * 4, po4, aux));
        L.gx[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rGx, lane * 4, po4, aux));
        L.gy[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rGy, lane * 4, po4, aux));
        L.cur[u].ab = __builtin_bit_cast(f32x2_a4, __builtin_amdgcn_raw_buffer_load_b64(rcur, off_ab, so, 0));
        L.cur[u].top = __builtin_bit_cast(f32x2_a4, __builtin_amdgcn_raw_buffer_load_b64(rcur, off_cd, so, 0));
      }
    };
    auto reduce = [&](const PatchLoads<kU> &L) {
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        // (compiler barrier tied to the accumulators: keeps the four record reads of patch u behind the sums of patch
        // u - 1 -- hoisted together they cost 64 registers and two waves of occupancy)
        asm volatile("" : "+v"(acc01), "+v"(acc23), "+v"(acc45) : : "memory");
        const float4 *r4 = rec4 + L.rec[u] * 4;
        const float4 wv = r4[0], qx = r4[1], qy = r4[2], qz = r4[3];
        // utilities.cpp:107 in the reference's operand order, never contracted: ((w0 a + w1 b) + w2 c) + w3 d -- template
        // and current patch must round identically so that identical frames give a residual of exactly zero
        float inew = wv.y * L.cur[u].ab.y + wv.x * L.cur[u].ab.x + wv.w * L.cur[u].top.y + wv.z * L.cur[u].top.x;
        if constexpr (PN) inew -= wave_sum(inew) / 64.0f;  // utilities.cpp:111-112
        const float gx = L.gx[u], gy = L.gy[u];
        const float r = (L.t[u] - inew) * qz.z;  // pdiff (odometer.cpp:381); 0 out of view and for padding
        // the J^T r sums are compared to tolerance only: explicit multiply-adds
        // (as register PAIRS: v_pk_fma_f32 does two of the six sums per instruction)
        const f32x2_t g2 = {gx * r, gy * r}, gr2 = {g2.x, g2.x}, hr2 = {g2.y, g2.y};
        acc01 = __builtin_elementwise_fma(g2, (f32x2_t){qz.x, qz.y}, acc01);  // sd1 = Gx cx0, sd2 = Gy cy1
        acc23 = __builtin_elementwise_fma(gr2, (f32x2_t){qx.x, qx.y},         // sd3..sd6 = Gx cxk + Gy cyk
                                          __builtin_elementwise_fma(hr2, (f32x2_t){qy.x, qy.y}, acc23));
        acc45 = __builtin_elementwise_fma(gr2, (f32x2_t){qx.z, qx.w},         // (odometer.cpp:319-326)
                                          __builtin_elementwise_fma(hr2, (f32x2_t){qy.z, qy.w}, acc45));
      }
    };
    PatchLoads<kU> A, B;
    issue(A, 0);
    for (int sidx = 0; sidx < nsteps; sidx += 2) {
      if (sidx + 1 < nsteps) issue(B, sidx + 1);
      reduce(A);
      if (sidx + 2 < nsteps) issue(A, sidx + 2);
      if (sidx + 1 < nsteps) reduce(B);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();  // the records are rewritten by the next chunk
  }

  const float acc[6] = {acc01.x, acc01.y, acc23.x, acc23.y, acc45.x, acc45.y};
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const float v = wave_sum(acc[k]);
    if (lane == 0) sW[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const float v = (sW[0][threadIdx.x] + sW[1][threadIdx.x]) + (sW[2][threadIdx.x] + sW[3][threadIdx.x]);
    e.partb[((size_t)b * gridDim.x + blockIdx.x) * kPartBStride + threadIdx.x] = v;
  }
}

// steps 4-6 for 8x8 patches, same two-stage, software-pipelined form: reference patches + gradients (bit-exact:
// un-contracted blends), sd coefficients, and the level's H partials in the form SURVEY.md §8 a18 prescribes. The
// steepest-descent images are sd_k = Gx cx_k + Gy cy_k with per-POINT constants cx, cy (odometer.cpp:313-326), so
//   H_jk = sum_pixels sd_j sd_k (odometer.cpp:428-455) = sum_points [cx_j cx_k Sxx + (cx_j cy_k + cy_j cx_k) Sxy + cy_j cy_k Syy]
// with three sums per patch, Sxx = sum Gx^2, Sxy = sum Gx Gy, Syy = sum Gy^2 (wave reductions while the kernel waits on
// memory anyway), instead of 21 multiply-adds per pixel in a separate instantiation of the iteration kernel. A point out
// of the reference view keeps its stale patch and coefficients (odometer.cpp:304): its S is summed from the stored
// gradients, so nothing but the patch buffers and the coefficient line carries state from level to level.
// H is compared to tolerance only (summation order differs from the CPU path's whole-buffer sums anyway).
// Gradients on the fly (OTF): a pyramid the builder made has dx = I(x+1) - I(x-1), dy = I(y+1) - I(y-1) inside the image,
// 0 on its border columns / rows (reflect-101) and in the padding (utilities.cpp:30-45), so the blended gradient patches
// can be formed from the IMAGE plane alone: the same f32 subtraction the builder did, the same blend -- the same bits --
// from a 4 x 4 neighbourhood per lane (12 texels: two 16-byte and two 8-byte loads) instead of the three planes' taps
// (or the packed 16-byte texels, a third of which is padding). The reference frame is then read at 4 B per pixel, and a
// pyramid built for this path (getgrad = 2) holds nothing but the image levels.
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef const f32x4_a4 __attribute__((address_space(1))) *gconst_f32x4a;
struct TapLoadsOTF {
  f32x4_a4 r0, r1;   // rows y and y-1: columns x-2 .. x+1   (b = r0[1], a = r0[2], d = r1[1], c = r1[2])
  f32x2_a4 up, dn;   // rows y+1 and y-2: columns x-1, x
};
__device__ __forceinline__ TapLoadsOTF taps_issue_otf(gconst_f32 img_at_base, int loff, int sw) {
  TapLoadsOTF t;
  gconst_f32 q = img_at_base + loff;
  t.r0 = *reinterpret_cast<gconst_f32x4a>(q - 2);
  t.r1 = *reinterpret_cast<gconst_f32x4a>(q - sw - 2);
  t.up = *reinterpret_cast<gconst_f32x2>(q + sw - 1);
  t.dn = *reinterpret_cast<gconst_f32x2>(q - 2 * sw - 1);
  return t;
}
// ix, iy: unpadded image coordinates of tap a of this lane's pixel; w, h: the level's size. interior: every tap of
// every lane of the patch is at least one pixel inside (wave-uniform fast path: no predicates)
__device__ __forceinline__ void taps_blend_otf(const TapLoadsOTF &t, float w0, float w1, float w2, float w3, bool interior,
                                               int ix, int iy, int w, int h, float &tv, float &gx, float &gy) {
  const float a = t.r0[2], b = t.r0[1], c = t.r1[2], d = t.r1[1];
  tv = w0 * a + w1 * b + w2 * c + w3 * d;
  float xa = t.r0[3] - t.r0[1], xb = t.r0[2] - t.r0[0], xc = t.r1[3] - t.r1[1], xd = t.r1[2] - t.r1[0];
  float ya = t.up.y - t.r1[2], yb = t.up.x - t.r1[1], yc = t.r0[2] - t.dn.y, yd = t.r0[1] - t.dn.x;
  if (!interior) {  // the builder's border rules: dx is 0 outside 1 <= X <= w-2 (and outside the image rows), dy alike
    const bool colA = ix >= 0 && ix < w, colB = ix - 1 >= 0 && ix - 1 < w, rowA = iy >= 0 && iy < h, rowC = iy - 1 >= 0 && iy - 1 < h;
    const bool dxA = ix >= 1 && ix <= w - 2, dxB = ix - 1 >= 1 && ix - 1 <= w - 2;
    const bool dyA = iy >= 1 && iy <= h - 2, dyC = iy - 1 >= 1 && iy - 1 <= h - 2;
    xa = (dxA && rowA) ? xa : 0.0f;
    xb = (dxB && rowA) ? xb : 0.0f;
    xc = (dxA && rowC) ? xc : 0.0f;
    xd = (dxB && rowC) ? xd : 0.0f;
    ya = (dyA && colA) ? ya : 0.0f;
    yb = (dyA && colB) ? yb : 0.0f;
    yc = (dyC && colA) ? yc : 0.0f;
    yd = (dyC && colB) ? yd : 0.0f;
  }
  gx = w0 * xa + w1 * xb + w2 * xc + w3 * xd;
  gy = w0 * ya + w1 * yb + w2 * yc + w3 * yd;
}

template <int I, int N, class Fn>
__device__ __forceinline__ void res_static_for(Fn &&fn) {  // fn(integral_constant<I>) ... fn(integral_constant<N - 1>)
  if constexpr (I < N) {
    fn(std::integral_constant<int, I>{});
    res_static_for<I + 1, N>(fn);
  }
}

template <int kU>
struct RefLoads {
  TapLoads4 p4[kU];
  TapLoadsOTF o[kU];
  int rec[kU];
  int vis[kU];
  int inner[kU];  // OTF: the patch's taps are all at least one pixel inside the image (wave-uniform)
  int tx[kU], ty[kU];  // OTF: unpadded coordinates of tap a of pixel (0, 0)
};

// ST (with OTF, without PN): the chunk's patches in statically unrolled groups of SIXTEEN -- three windows in flight,
// and the three sums of S per patch by the transposing wave reduction of the resident kernel (TrAcc, ictr_devfn.h: ~10
// instructions per patch instead of the 42 of three wave sums + selects); everything else as in the dynamic form.
//
// TB > 0 (with ST), the STAGED form: the reference image reaches the lanes through LDS instead of the L1. Per wave and
// 16-patch group the bounding box of the group's windows (rows rmin-2 .. rmax+8, columns cmin-2 .. cmax+8 rounded out to
// 128-byte lines) is copied into a tile of TB bytes that is private to the wave: one direct-to-LDS buffer load per box
// row, 16 bytes per lane, consecutive lanes along the row -- every line of the box is requested once, by one
// instruction, so no load ever finds its line "miss pending" behind another one of the kernel's own. The tile holds the
// padded plane's bytes as they are (row r at r * pitch, from the row's own line boundary on); the twelve texels per lane
// come out of it with LDS reads into the same TapLoadsOTF, and taps_blend_otf runs on them unchanged: the same bits.
// pitch = lines * 128 plus, where the tile has the room, the few bytes that put four consecutive rows on different LDS
// banks. A group whose box does not fit the tile (scattered points) takes the direct taps; the choice is wave-uniform.
// The buffer resource is bounded by the plane: what the rounding to lines adds beyond it reads as zeros and is never
// consumed. The line touches of the ST form go away here.
struct RefBox {
  int on;        // the group's taps come from the tile
  int a0;        // byte address (mod 2^32 of the plane's line grid) of the box's first texel
  int pitch;     // bytes from one tile row to the next
  int r0, c0;    // padded coordinates of the box's first texel
};
template <bool PN, int kU, bool PK, bool OTF = false, bool ST = false, int TB = 0>  // PK: packed {img, dx, dy, 0} planes; OTF: image plane only
__global__ __launch_bounds__(kBlock) void k_ref8(EngineDev e, LevelCam lc, int level, int cpw) {
  static_assert(PK != OTF, "the taps come from either the packed planes or the image plane");
  static_assert(!ST || (OTF && !PN), "the static form exists for on-the-fly gradients without patch normalisation");
  static_assert(TB == 0 || (ST && TB % 16 == 0), "the staged form is a static form; 16-byte pieces");
  constexpr bool STG = TB > 0;
  __shared__ __attribute__((aligned(16))) float sRec[kWaves][64 * kRec];
  __shared__ float sW[kWaves][kPartHStride];
  __shared__ __attribute__((aligned(16))) char sTile[STG ? kWaves * TB : 16];
  const int b = blockIdx.y;
  const ProbState &st = e.st[b];
  const int npts = st.npts;
  const int M = e.M;
  const PlaneSet pl = e.planes[b * e.nlev + level];
  const float *__restrict__ pt2d = e.pt2d + ((size_t)b * e.nlev + level) * 2 * M;
  const float *__restrict__ p3r = e.pt3d_ref + (size_t)b * 3 * M;
  float *T = e.T + (size_t)b * M * 64;
  float *Gx = e.Gx + (size_t)b * M * 64;
  float *Gy = e.Gy + (size_t)b * M * 64;
  float *coefb = e.coef + (size_t)b * M * kCoefStride;
  gconst_f32 pref = (gconst_f32)pl.ref;
  gconst_f32x4 ppack = (gconst_f32x4)pl.pack;
  const int sw = lc.sw;
  const int wl = (int)lc.swo, hl = (int)lc.sho, padl = (sw - wl) / 2;  // (OTF) the level's unpadded size, its padding

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int loff = (lane >> 3) * sw + (lane & 7);
  float *rec = sRec[wave];
  const float4 *rec4 = reinterpret_cast<const float4 *>(rec);

  float accH = 0.0f;  // lane j < 21: the wave's sum of H entry j (upper triangle, row-major)

  // (STG) the wave's tile; the image plane as a bounded buffer (the pointer is wave-uniform but comes out of a table in
  // memory: say so, as the resident prologue does); the plane's position on the 128-byte line grid; the tile rows' bank
  // stagger: image rows are sw floats apart, four consecutive ones are read by one 32-lane half of an LDS read, 8 lanes
  // each -- the pad makes the step from row to row 8 or 24 banks (mod 32) where sw alone would not
  char *const tile = sTile + (STG ? wave * TB : 0);
  const int tile_lds = __builtin_amdgcn_readfirstlane((int)(unsigned long long)(__attribute__((address_space(3))) char *)tile);
  const int sw4 = sw * 4;
  int base_low = 0, pad_b = 0;
  typedef int i32x4_t __attribute__((ext_vector_type(4)));
  i32x4_t rimg = {0, 0, 0, 0};  // the buffer resource: base, no stride, the plane's bytes, raw 32-bit data
  if constexpr (STG) {
    const unsigned long long pr64 = reinterpret_cast<unsigned long long>(pl.ref);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)pr64), hi = __builtin_amdgcn_readfirstlane((unsigned)(pr64 >> 32));
    rimg = (i32x4_t){(int)lo, (int)(hi & 0xffffu), __builtin_amdgcn_readfirstlane(sw4 * (hl + 2 * padl)), 0x00020000};
    base_low = (int)(lo & 127u);
    const int to8 = (8 - sw) & 31, to24 = (24 - sw) & 31;
    pad_b = (min(to8, to24) * 4 + 8) & ~15;
  }
  int bx_rmin = 0, bx_rmax = 0, bx_cmin = 0, bx_cmax = 0;  // (STG) per 16-lane row: the bounding box of its points' windows
  // (STG) box of the chunk's group g0 -> tile: one load per box row, lanes = the row's 16-byte pieces
  auto stage_box = [&](int g0) {
    RefBox bx;
    const int rmin = rlane(bx_rmin, g0), rmax = rlane(bx_rmax, g0), cmin = rlane(bx_cmin, g0), cmax = rlane(bx_cmax, g0);
    const bool any = rmin <= rmax;  // some point of the group is in view
    const int nrows = any ? rmax - rmin + 11 : 0, wb = any ? (cmax - cmin + 11) * 4 : 0;
    bx.r0 = any ? rmin - 2 : 0;
    bx.c0 = any ? cmin - 2 : 0;
    bx.a0 = base_low + (bx.r0 * sw + bx.c0) * 4;
    // lines per tile row: the most that any of the box's rows needs from its own line boundary on
    const int nl_lo = (wb + 127) >> 7;
    const bool more = lane < nrows && ((((bx.a0 + lane * sw4) & 127) + wb + 127) >> 7) > nl_lo;
    const int nl = nl_lo + (__builtin_amdgcn_ballot_w64(more) != 0ull ? 1 : 0);
    int pitch = nl * 128 + pad_b;
    bool fits = nrows * pitch - pad_b <= TB;
    if (!fits) {
      pitch = nl * 128;
      fits = nrows * pitch <= TB;
    }
    bx.pitch = pitch;
    bx.on = (any && fits && nl <= 8) ? 1 : 0;
    if (bx.on) {
      for (int r = 0; r < nrows; ++r) {  // (wave-uniform)
        const int ar = bx.a0 + r * sw4;
        const int need = ((ar & 127) + wb + 127) >> 7;  // whole lines of this row
        // (as a statement of its own: to the compiler a direct-to-LDS load is a pending write of ALL of LDS, and every
        // record read and write of the patch loop would wait for the box and for the patch stores queued before it.
        // The group loop waits for the tile itself, once, before its first read. M0 = the row's place in LDS.)
        if (lane < need * 8) {
          int keep;
          asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, 0 offen lds\n\t"
                       "s_mov_b32 m0, %0"
                       : "=&s"(keep)
                       : "s"(tile_lds + r * pitch), "v"((ar & ~127) - base_low + lane * 16), "s"(rimg)
                       : "memory");
        }
      }
    }
    return bx;
  };

  const int nchunks = (npts + cpw - 1) / cpw;
  for (int ch = xcd_band_block(blockIdx.x, gridDim.x) * kWaves + wave; ch < nchunks; ch += gridDim.x * kWaves) {
    const int i0 = ch * cpw;
    const int cnt = min(cpw, npts - i0);
    // ---- stage 1: one point per lane: visibility (odometer.cpp:273-282), sd coefficients (:313-326)
    const bool pv = lane < cnt;
    const int ip = i0 + (pv ? lane : 0);
    const float mx = pt2d[ip], my = pt2d[ip + M];
    const bool vis = pv && in_view(mx, my, lc.swo, lc.sho);
    const Taps tp = taps_or_fallback(vis, mx, my, 4);
#ifndef ICTR_REF8_TOUCH
#define ICTR_REF8_TOUCH 6  // line touches per lane and chunk (0: none)
#endif
    // (ST) Touch every cache line of the chunk's windows ONCE before the taps ask for them. The taps of a window are four
    // loads over the same eleven rows, and neighbouring patches share lines: with a frame that is not in the L2 each of
    // them finds its line "miss pending" and the L1's tag pipeline stalls until the line arrives -- for every wave of
    // the CU, the stores included (TCP_PENDING_STALL_CYCLES: 278 us of a 448 us launch; 32 distinct 1080p pairs 448 /
    // 325 / 275 us per level, with the touches 342 / 282 / 255; profiles/r03_notes.md 10). Lanes 16 g .. 16 g + 15
    // own the chunk's group g: lane i takes row i of the group's bounding box, touch k the box's k-th line of that row,
    // so no two lanes of one load and no two loads of a group ask for the same line. Issued before the coefficients
    // are formed, waited for before the first window. Boxes of scattered points (more than 16 rows or kTouch lines
    // per row) are not touched.
    constexpr int kTouch = (ST && !STG) ? ICTR_REF8_TOUCH : 0;
    RefBox box0;
    if constexpr (STG) {  // the first group's box is on its way while the coefficients are formed
      const int kBig = 1 << 28;
      bx_rmin = row_min_dpp(vis ? tp.row0 : kBig), bx_rmax = -row_min_dpp(vis ? -tp.row0 : kBig);
      bx_cmin = row_min_dpp(vis ? tp.col0 : kBig), bx_cmax = -row_min_dpp(vis ? -tp.col0 : kBig);
      box0 = stage_box(0);
    }
    float touch[kTouch > 0 ? kTouch : 1];
    if constexpr (kTouch > 0) {
      const int kBig = 1 << 28;
      const int rmin = row_min_dpp(vis ? tp.row0 : kBig), rmax = -row_min_dpp(vis ? -tp.row0 : kBig);
      const int cmin = row_min_dpp(vis ? tp.col0 : kBig), cmax = -row_min_dpp(vis ? -tp.col0 : kBig);
      const int li = lane & 15, nrows = rmax - rmin + 11;
      const unsigned long long a_first = (unsigned long long)(pl.ref + (size_t)(rmin - 2 + li) * sw + (cmin - 2));
      const unsigned long long a_last = (unsigned long long)(pl.ref + (size_t)(rmin - 2 + li) * sw + (cmax + 8)) + 3;
      const unsigned long long a0 = a_first & ~127ull;
      const int nl = (int)(((a_last | 127ull) - a0 + 1) >> 7);
      const bool box = rmin < kBig && nrows <= 16 && li < nrows && nl <= kTouch;
#pragma unroll
      for (int k = 0; k < kTouch; ++k) {
        touch[k] = 0.0f;
        if (box && k < nl) touch[k] = *(gconst_f32)(a0 + 128ull * k);
      }
    }
    float cx[6], cy[6];
    setup_point(vis, p3r, ip, M, lc, reinterpret_cast<float4 *>(coefb + (size_t)ip * kCoefStride), cx, cy);
    const int base_v = tp.row0 * sw + tp.col0;
    const int vis_v = vis ? 1 : 0;
    const int tx_v = tp.col0 - padl, ty_v = tp.row0 - padl;  // (OTF) tap a of pixel (0,0) in unpadded image coordinates
    {
      float4 *r4 = reinterpret_cast<float4 *>(rec + lane * kRec);
      r4[0] = make_float4(tp.w0, tp.w1, tp.w2, tp.w3);
      r4[1] = make_float4(cx[0], cx[1], cx[2], cx[3]);
      r4[2] = make_float4(cx[4], cx[5], cy[0], cy[1]);
      r4[3] = make_float4(cy[2], cy[3], cy[4], cy[5]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // ---- stage 2 (utilities.cpp:115-189); patches of a step are nsteps apart
    float sxx_v = 0.0f, sxy_v = 0.0f, syy_v = 0.0f;  // lane j: S of the chunk's point j (0 beyond the chunk)
    const int nsteps = (cnt + kU - 1) / kU;
    auto issue = [&](RefLoads<kU> &L, int sidx) {
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int jraw = sidx + u * nsteps;
        const int jj = min(jraw, cnt - 1);
        L.rec[u] = (jraw < cnt) ? jj : -1;
        const int base = rlane(base_v, jj);
        L.vis[u] = rlane(vis_v, jj);
        if (L.vis[u]) {  // wave-uniform
          if constexpr (OTF) {
            L.tx[u] = rlane(tx_v, jj);
            L.ty[u] = rlane(ty_v, jj);
            L.inner[u] = (L.tx[u] >= 2 && L.tx[u] + 7 <= wl - 2 && L.ty[u] >= 2 && L.ty[u] + 7 <= hl - 2) ? 1 : 0;
            L.o[u] = taps_issue_otf(pref + base, loff, sw);
          } else {
            L.p4[u] = taps_issue4(ppack + base, loff, sw, lane);
          }
        }
      }
    };
    auto patch_sums = [&](float gx, float gy, int j) {  // the patch's three sums into lane j (the sums are wave-uniform)
      const float sxx = wave_sum_dpp(gx * gx), sxy = wave_sum_dpp(gx * gy), syy = wave_sum_dpp(gy * gy);
      const bool mine = lane == j;
      sxx_v = mine ? sxx : sxx_v;
      sxy_v = mine ? sxy : sxy_v;
      syy_v = mine ? syy : syy_v;
    };
    auto reduce = [&](const RefLoads<kU> &L) {
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        if (L.rec[u] < 0 || !L.vis[u]) continue;  // wave-uniform
        float gx, gy;
        {
          const float4 w = rec4[L.rec[u] * 4 + 0];
          float t;
          if constexpr (OTF) {
            taps_blend_otf(L.o[u], w.x, w.y, w.z, w.w, L.inner[u] != 0, L.tx[u] + (lane & 7), L.ty[u] + (lane >> 3), wl, hl,
                           t, gx, gy);
          } else {
            t = taps_blend4(L.p4[u], 0, w.x, w.y, w.z, w.w, lane);
            gx = taps_blend4(L.p4[u], 1, w.x, w.y, w.z, w.w, lane);
            gy = taps_blend4(L.p4[u], 2, w.x, w.y, w.z, w.w, lane);
          }
          if constexpr (PN) t -= wave_sum(t) / 64.0f;  // utilities.cpp:187-188
          const size_t po = (size_t)(i0 + L.rec[u]) * 64;
          // 400 MB written once per level: do not let them push the pyramid planes out of L2
          __builtin_nontemporal_store(t, T + po + lane);
          __builtin_nontemporal_store(gx, Gx + po + lane);
          __builtin_nontemporal_store(gy, Gy + po + lane);
        }
        patch_sums(gx, gy, L.rec[u]);
      }
    };
    if constexpr (ST) {
      const int inner_v = (tx_v >= 2 && tx_v + 7 <= wl - 2 && ty_v >= 2 && ty_v + 7 <= hl - 2) ? 1 : 0;
      // the wave waits for its touched lines here (the other waves of the CU carry on) rather than let its taps find
      // them pending
      if constexpr (kTouch > 0) {
#pragma unroll
        for (int k = 0; k < kTouch; ++k) asm volatile("" ::"v"(touch[k]));
      }
#ifndef ICTR_REF8_PREFETCH
#define ICTR_REF8_PREFETCH 1  // (STG) 1: the next group's box is requested behind the current group's last window's reads,
#endif                        // 0: behind its last store
      RefBox cur = box0, nxt = box0;
#ifndef ICTR_REF8_D
#define ICTR_REF8_D 3  // windows in flight per wave (12 registers each)
#endif
      constexpr int kD = ICTR_REF8_D;
      // one group of sixteen patches; tiled_c: its taps come out of the wave's tile. (Two bodies, not one with a branch
      // per window: where the same registers could take a window from either source, every LDS read would first wait
      // for a global load that might still be writing them -- on the in-order counter, for the patch stores.)
      auto run_group = [&](int g0, auto tiled_c) {
        constexpr bool kTiled = decltype(tiled_c)::value;
        const unsigned vmask = (unsigned)(__builtin_amdgcn_ballot_w64(vis) >> g0) & 0xffffu;  // the group's visible points
        TapLoadsOTF W3[kD];
        // (STG) the window's twelve texels out of the tile: image row Y of the box is tile row Y - r0, its texel X at
        // ((a0 + (Y - r0) sw4) & 127) + 4 (X - c0) bytes from the tile row's start
        auto taps_lds = [&](int j) {
          TapLoadsOTF t;
          const int trow = rlane(ty_v, g0 + j) + padl - 2 - cur.r0 + (lane >> 3);  // tile row of image row y - 2
          const int xo = (rlane(tx_v, g0 + j) + padl - cur.c0 + (lane & 7)) * 4;   // bytes from column c0 to column x
          int ar = cur.a0 + trow * sw4, lp = trow * cur.pitch + xo;
          auto at = [&](int o) { return *reinterpret_cast<const float *>(tile + o); };
          const int o_dn = lp + (ar & 127);
          ar += sw4, lp += cur.pitch;
          const int o_r1 = lp + (ar & 127);
          ar += sw4, lp += cur.pitch;
          const int o_r0 = lp + (ar & 127);
          ar += sw4, lp += cur.pitch;
          const int o_up = lp + (ar & 127);
          t.r0 = (f32x4_a4){at(o_r0 - 8), at(o_r0 - 4), at(o_r0), at(o_r0 + 4)};
          t.r1 = (f32x4_a4){at(o_r1 - 8), at(o_r1 - 4), at(o_r1), at(o_r1 + 4)};
          t.up = (f32x2_a4){at(o_up - 4), at(o_up)};
          t.dn = (f32x2_a4){at(o_dn - 4), at(o_dn)};
          return t;
        };
        auto issue_s = [&](int j) {
          if (!((vmask >> j) & 1u)) return;
          if constexpr (kTiled) {
            W3[j % kD] = taps_lds(j);
            return;
          }
#if defined(ICTR_REF8_ABL) && (ICTR_REF8_ABL & 2)  // measurement build: every window = the plane's first (L1 hits)
          W3[j % kD] = taps_issue_otf(pref + 2 * sw + 2 + (rlane(base_v, g0 + j) & 7), loff, sw);
#else
          W3[j % kD] = taps_issue_otf(pref + rlane(base_v, g0 + j), loff, sw);
#endif
        };
        if constexpr (kTiled) {  // the tile is written by loads: their counter, then the reads
          __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
          asm volatile("" ::: "memory");
        }
        res_static_for<0, kD>([&](auto jc) { issue_s(decltype(jc)::value); });
        TrAcc<16> accS, accX;
        tr_for_each_patch<16, 0>([&](auto jc) {
          constexpr int j = decltype(jc)::value;
          float gx = 0.0f, gy = 0.0f;
          if ((vmask >> j) & 1u) {  // wave-uniform
            const float4 w = rec4[(g0 + j) * 4 + 0];
            float t;
            taps_blend_otf(W3[j % kD], w.x, w.y, w.z, w.w, rlane(inner_v, g0 + j) != 0, rlane(tx_v, g0 + j) + (lane & 7),
                           rlane(ty_v, g0 + j) + (lane >> 3), wl, hl, t, gx, gy);
            const size_t po = (size_t)(i0 + g0 + j) * 64;
#if defined(ICTR_REF8_ABL) && (ICTR_REF8_ABL & 1)   // measurement build: no patch stores (the sums keep the blends alive)
            gx += t * 1e-30f;
#else
            __builtin_nontemporal_store(t, T + po + lane);
            __builtin_nontemporal_store(gx, Gx + po + lane);
            __builtin_nontemporal_store(gy, Gy + po + lane);
#endif
          }
          if constexpr (j + kD < 16) issue_s(j + kD);
          if constexpr (STG && ICTR_REF8_PREFETCH != 0 && j + kD == 15) {
            if (g0 + 16 < cnt) {  // every read of the tile has been issued: once they are back it is the next group's
              if constexpr (kTiled) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
              nxt = stage_box(g0 + 16);
            }
          }
          accS.template push<j>(gx * gx, gy * gy, lane);
          accX.template push<j>(gx * gy, 0.0f, lane);
        });
        // lane = point again: the group's sixteen points are the lanes g0 .. g0 + 15
        const int pp = lane & 15;
        const float sxx = lane_gather(accS.F, tr_lane_of<16>(pp, 0)), syy = lane_gather(accS.F, tr_lane_of<16>(pp, 1));
        const float sxy = lane_gather(accX.F, tr_lane_of<16>(pp, 0));
        const bool mine = (lane >> 4) == (g0 >> 4);
        sxx_v = mine ? sxx : sxx_v;
        sxy_v = mine ? sxy : sxy_v;
        syy_v = mine ? syy : syy_v;
      };
      for (int g0 = 0; g0 < cnt; g0 += 16) {  // (wave-uniform trip count: cnt is)
        if (STG && cur.on)  // wave-uniform
          run_group(g0, std::integral_constant<bool, STG>{});
        else
          run_group(g0, std::false_type{});
        if constexpr (STG) {
          static_assert(kD < 16, "the prefetch sits behind window 15's reads");
          if (ICTR_REF8_PREFETCH == 0 && g0 + 16 < cnt) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            nxt = stage_box(g0 + 16);
          }
          cur = nxt;
        }
      }
    } else {
    RefLoads<kU> A, B;
    issue(A, 0);
    for (int sidx = 0; sidx < nsteps; sidx += 2) {
      if (sidx + 1 < nsteps) issue(B, sidx + 1);
      reduce(A);
      if (sidx + 2 < nsteps) issue(A, sidx + 2);
      if (sidx + 1 < nsteps) reduce(B);
    }
    }
    // points out of the reference view at this level (rare): S of the stale patch, from the stored gradients
    for (unsigned long long stale = __builtin_amdgcn_ballot_w64(pv && !vis); stale; stale &= stale - 1) {
      const int j = __builtin_ctzll(stale);
      const size_t po = (size_t)(i0 + j) * 64;
      patch_sums((Gx + po)[lane], (Gy + po)[lane], j);
    }
    // ---- H += J^T S J, one point per lane again (its coefficients come back from the wave's records)
    {
      const float4 k0 = rec4[lane * 4 + 1], k1 = rec4[lane * 4 + 2], k2 = rec4[lane * 4 + 3];
      const float ax[6] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y}, ay[6] = {k1.z, k1.w, k2.x, k2.y, k2.z, k2.w};
      float uj[6], vj[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        uj[j] = __builtin_fmaf(ax[j], sxx_v, ay[j] * sxy_v);
        vj[j] = __builtin_fmaf(ax[j], sxy_v, ay[j] * syy_v);
      }
      int jk = 0;
#pragma unroll
      for (int j = 0; j < 6; ++j)
#pragma unroll
        for (int k = j; k < 6; ++k, ++jk) {
          const float h = wave_sum_dpp(__builtin_fmaf(ax[k], uj[j], ay[k] * vj[j]));
          accH += lane == jk ? h : 0.0f;
          if (jk % 3 == 2) asm volatile("" : "+v"(accH));  // three reductions at a time (their row sums sit in SGPRs)
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }

  if (lane < kPartHStride) sW[wave][lane] = lane < kHUnique ? accH : 0.0f;
  __syncthreads();
  if (threadIdx.x < kHUnique) {
    const float v = (sW[0][threadIdx.x] + sW[1][threadIdx.x]) + (sW[2][threadIdx.x] + sW[3][threadIdx.x]);
    e.partH[((size_t)b * gridDim.x + blockIdx.x) * kPartHStride + threadIdx.x] = v;
  }
}

// ================================================================ P = 4 fast path (wave64 == four 4x4 patches)
// The reference's other standard patch size (run_odometer_test.m:140: "4 0 4 5 0.01 0 0"). Same two-stage,
// software-pipelined form as the 8x8 kernels; a wave-step handles FOUR consecutive patches, one per 16-lane group
// (lane = 16 * sub + 4 * row + col): the four patches' T/Gx/Gy rows are one contiguous 256-byte row, the window
// base and the LDS record index are per lane (gathered with ds_bpermute instead of v_readlane), validity and
// visibility are per-lane predicates instead of wave-uniform branches. Requires the packed reference planes.
struct TapLoads4x4 {  // one patch group per 16 lanes; a/b of the own row, top row for the lanes of patch row 0
  f32x2_a4 ab, top;
};
__device__ __forceinline__ TapLoads4x4 taps4_issue(gconst_f32 plane, int idx, int sw, bool ok, bool toprow) {
  TapLoads4x4 t;
  f32x2_a4 z = {0.0f, 0.0f};
  t.ab = z;
  t.top = z;
  if (ok) {
    t.ab = *reinterpret_cast<gconst_f32x2>(plane + (idx - 1));
    if (toprow) t.top = *reinterpret_cast<gconst_f32x2>(plane + (idx - sw - 1));
  }
  return t;
}
__device__ __forceinline__ float taps4_blend(const TapLoads4x4 &t, float w0, float w1, float w2, float w3, bool toprow) {
  const float a = t.ab.y, b = t.ab.x;
  const float cu = __shfl_up(a, 4, 64), du = __shfl_up(b, 4, 64);  // the lane one patch row up (same 16-lane group)
  const float c = toprow ? t.top.y : cu, d = toprow ? t.top.x : du;
  return w0 * a + w1 * b + w2 * c + w3 * d;
}
struct TapLoadsP4 {
  f32x4_t l, r, tl, tr;
};
__device__ __forceinline__ float tapsP4_blend(const TapLoadsP4 &t, int k, float w0, float w1, float w2, float w3, bool toprow) {
  const float a = t.r[k], b = t.l[k];
  const float cu = __shfl_up(a, 4, 64), du = __shfl_up(b, 4, 64);
  const float c = toprow ? t.tr[k] : cu, d = toprow ? t.tl[k] : du;
  return w0 * a + w1 * b + w2 * c + w3 * d;
}

template <int kU>
struct Iter4Loads {
  float t[kU], gx[kU], gy[kU];
  TapLoads4x4 cur[kU];
  int jj[kU];  // per lane: index of its patch inside the chunk, or -1
};

template <bool PN, bool WH, int kU = 2>
__global__ __launch_bounds__(kBlock) void k_iter4(EngineDev e, LevelCam lc, int level, int cpw) {
  __shared__ __attribute__((aligned(16))) float sRec[kWaves][64 * kRec];
  __shared__ float sW[kWaves][kPartBStride];
  __shared__ float sWH[WH ? kWaves : 1][kPartHStride];
  const int b = blockIdx.y;
  const ProbState &st = e.st[b];
  if (!st.active) return;
  const int npts = st.npts;
  const int M = e.M;
  const PlaneSet pl = e.planes[b * e.nlev + level];
  const float *__restrict__ p3 = e.pt3d + (size_t)b * 3 * M;
  const float *__restrict__ T = e.T + (size_t)b * M * 16;
  const float *__restrict__ Gx = e.Gx + (size_t)b * M * 16;
  const float *__restrict__ Gy = e.Gy + (size_t)b * M * 16;
  const float *__restrict__ coefb = e.coef + (size_t)b * M * kCoefStride;
  gconst_f32 cur = (gconst_f32)pl.cur;
  const int sw = lc.sw;

  float G[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) G[k] = st.G[k];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int sub = lane >> 4, q = lane & 15;
  const bool toprow = q < 4;
  const int loff = (q >> 2) * sw + (q & 3);
  float *rec = sRec[wave];
  const float4 *rec4 = reinterpret_cast<const float4 *>(rec);

  float acc[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) acc[k] = 0.0f;
  float accH[WH ? kHUnique : 1];
#pragma unroll
  for (int j = 0; j < (WH ? kHUnique : 1); ++j) accH[j] = 0.0f;

  const int nchunks = (npts + cpw - 1) / cpw;
  for (int ch = xcd_band_block(blockIdx.x, gridDim.x) * kWaves + wave; ch < nchunks; ch += gridDim.x * kWaves) {
    const int i0 = ch * cpw;
    const int cnt = min(cpw, npts - i0);
    // ---- stage 1: lane j <-> point i0 + j (as k_iter8, half-size 2)
    const bool pv = lane < cnt;
    const int ip = i0 + (pv ? lane : 0);
    const float X = p3[ip], Y = p3[ip + M], Z = p3[ip + 2 * M];
    float cx[6], cy[6];
    coef_line_load(reinterpret_cast<const float4 *>(coefb + (size_t)ip * kCoefStride), cx, cy);
    const IterPoint pt = iter_point(G, X, Y, Z, lc, pv, 2);
    const Taps &tp = pt.tp;
    const int base_v = tp.row0 * sw + tp.col0;
    {
      float4 *r4 = reinterpret_cast<float4 *>(rec + lane * kRec);
      r4[0] = make_float4(tp.w0, tp.w1, tp.w2, tp.w3);
      r4[1] = make_float4(cx[0], cx[2], cx[3], cx[4]);
      r4[2] = make_float4(cx[5], cy[1], cy[2], cy[3]);
      r4[3] = make_float4(cy[4], cy[5], pt.vis ? 1.0f : 0.0f, 0.0f);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // ---- stage 2: wave-steps of four patches; kU wave-steps per pipeline step, nsteps apart
    const int nws = (cnt + 3) >> 2;
    const int nsteps = (nws + kU - 1) / kU;
    auto issue = [&](Iter4Loads<kU> &L, int sidx) {
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int ws = sidx + u * nsteps;
        const int j = 4 * ws + sub;
        const bool ok = (ws < nws) & (j < cnt);
        L.jj[u] = ok ? j : -1;
        const int base = __shfl(base_v, ok ? j : 0, 64);
        const size_t po = (size_t)(i0 + 4 * min(ws, nws - 1)) * 16;  // wave-uniform: 4 patches = one 256-byte row
        L.t[u] = L.gx[u] = L.gy[u] = 0.0f;
        if (ok) {
          L.t[u] = __builtin_nontemporal_load(T + po + lane);
          L.gx[u] = __builtin_nontemporal_load(Gx + po + lane);
          L.gy[u] = __builtin_nontemporal_load(Gy + po + lane);
        }
        L.cur[u] = taps4_issue(cur, base + loff, sw, ok, toprow);
      }
    };
    auto reduce = [&](const Iter4Loads<kU> &L) {
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const bool ok = L.jj[u] >= 0;
        const int ri = (ok ? L.jj[u] : 0) * 4;
        const float4 w = rec4[ri + 0], k0 = rec4[ri + 1], k1 = rec4[ri + 2], k2 = rec4[ri + 3];
        float inew = taps4_blend(L.cur[u], w.x, w.y, w.z, w.w, toprow);
        if constexpr (PN) inew -= group_sum(inew, 16) / 16.0f;  // utilities.cpp:111-112
        const float r = ok ? (L.t[u] - inew) * k2.z : 0.0f;  // pdiff (odometer.cpp:381); k2.z = 0 out of the new view
        const float gx = L.gx[u], gy = L.gy[u];                // zero for lanes without a patch
        {
#pragma clang fp contract(fast)
          acc[0] += (gx * k0.x) * r;
          acc[1] += (gy * k1.y) * r;
          acc[2] += (gx * k0.y + gy * k1.z) * r;
          acc[3] += (gx * k0.z + gy * k1.w) * r;
          acc[4] += (gx * k0.w + gy * k2.x) * r;
          acc[5] += (gx * k1.x + gy * k2.y) * r;
          if constexpr (WH) {
            float sd[6];
            sd[0] = gx * k0.x;
            sd[1] = gy * k1.y;
            sd[2] = gx * k0.y + gy * k1.z;
            sd[3] = gx * k0.z + gy * k1.w;
            sd[4] = gx * k0.w + gy * k2.x;
            sd[5] = gx * k1.x + gy * k2.y;
            int jk = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
              for (int c = a; c < 6; ++c) accH[jk++] += sd[a] * sd[c];
          }
        }
      }
    };
    Iter4Loads<kU> A, B;
    issue(A, 0);
    for (int sidx = 0; sidx < nsteps; sidx += 2) {
      if (sidx + 1 < nsteps) issue(B, sidx + 1);
      reduce(A);
      if (sidx + 2 < nsteps) issue(A, sidx + 2);
      if (sidx + 1 < nsteps) reduce(B);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }

#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const float v = wave_sum(acc[k]);
    if (lane == 0) sW[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 6)
    e.partb[((size_t)b * gridDim.x + blockIdx.x) * kPartBStride + threadIdx.x] =
        (sW[0][threadIdx.x] + sW[1][threadIdx.x]) + (sW[2][threadIdx.x] + sW[3][threadIdx.x]);
  if constexpr (WH) {
#pragma unroll
    for (int j = 0; j < kHUnique; ++j) {
      const float v = wave_sum(accH[j]);
      if (lane == 0) sWH[wave][j] = v;
    }
    __syncthreads();
    if (threadIdx.x < kHUnique)
      e.partH[((size_t)b * gridDim.x + blockIdx.x) * kPartHStride + threadIdx.x] =
          (sWH[0][threadIdx.x] + sWH[1][threadIdx.x]) + (sWH[2][threadIdx.x] + sWH[3][threadIdx.x]);
  }
}

template <int kU>
struct Ref4Loads {
  TapLoadsP4 p4[kU];
  int jj[kU];   // per lane: patch index inside the chunk, -1 = none
  int vis[kU];  // per lane: that patch is inside the reference view at this level
};

// steps 4-5 for 4x4 patches (H deferred to the first k_iter4<.., WH = true> launch; packed reference planes)
template <bool PN>
__global__ __launch_bounds__(kBlock) void k_ref4(EngineDev e, LevelCam lc, int level, int cpw) {
  constexpr int kU = 2;
  const int b = blockIdx.y;
  const ProbState &st = e.st[b];
  const int npts = st.npts;
  const int M = e.M;
  const PlaneSet pl = e.planes[b * e.nlev + level];
  const float *__restrict__ pt2d = e.pt2d + ((size_t)b * e.nlev + level) * 2 * M;
  const float *__restrict__ p3r = e.pt3d_ref + (size_t)b * 3 * M;
  float *T = e.T + (size_t)b * M * 16;
  float *Gx = e.Gx + (size_t)b * M * 16;
  float *Gy = e.Gy + (size_t)b * M * 16;
  float *coefb = e.coef + (size_t)b * M * kCoefStride;
  gconst_f32x4 ppack = (gconst_f32x4)pl.pack;
  const int sw = lc.sw;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int sub = lane >> 4, q = lane & 15;
  const bool toprow = q < 4;
  const int loff = (q >> 2) * sw + (q & 3);

  const int nchunks = (npts + cpw - 1) / cpw;
  for (int ch = xcd_band_block(blockIdx.x, gridDim.x) * kWaves + wave; ch < nchunks; ch += gridDim.x * kWaves) {
    const int i0 = ch * cpw;
    const int cnt = min(cpw, npts - i0);
    // ---- stage 1: one point per lane: visibility (odometer.cpp:273-282), sd coefficients (:313-326)
    const bool pv = lane < cnt;
    const int ip = i0 + (pv ? lane : 0);
    const float mx = pt2d[ip], my = pt2d[ip + M];
    const bool vis = pv && in_view(mx, my, lc.swo, lc.sho);
    if (vis) {  // invisible points keep their stale coefficients (odometer.cpp:304): nothing to do for them
      float cx[6], cy[6];
      sd_coefs(p3r[ip], p3r[ip + M], p3r[ip + 2 * M], lc.fx, lc.fy, cx, cy);
      coef_line_store(reinterpret_cast<float4 *>(coefb + (size_t)ip * kCoefStride), cx, cy);
    }
    const Taps tp = taps_or_fallback(vis, mx, my, 2);
    const int base_v = tp.row0 * sw + tp.col0;
    const int vis_v = vis ? 1 : 0;
    const float w0 = tp.w0, w1 = tp.w1, w2 = tp.w2, w3 = tp.w3;

    // ---- stage 2: wave-steps of four patches (utilities.cpp:115-189)
    const int nws = (cnt + 3) >> 2;
    const int nsteps = (nws + kU - 1) / kU;
    auto issue = [&](Ref4Loads<kU> &L, int sidx) {
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int ws = sidx + u * nsteps;
        const int j = 4 * ws + sub;
        const bool ok = (ws < nws) & (j < cnt);
        const int js = ok ? j : 0;
        L.jj[u] = ok ? j : -1;
        const int v = __shfl(vis_v, js, 64);
        const int base = __shfl(base_v, js, 64);
        L.vis[u] = (ok && v) ? 1 : 0;
        f32x4_t z = {0.0f, 0.0f, 0.0f, 0.0f};
        L.p4[u].l = L.p4[u].r = L.p4[u].tl = L.p4[u].tr = z;
        if (L.vis[u]) {
          gconst_f32x4 pp = ppack + (base + loff);
          L.p4[u].l = pp[-1];
          L.p4[u].r = pp[0];
          if (toprow) {
            L.p4[u].tl = pp[-sw - 1];
            L.p4[u].tr = pp[-sw];
          }
        }
      }
    };
    auto reduce = [&](const Ref4Loads<kU> &L, int sidx) {
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int ws = sidx + u * nsteps;
        const int js = L.jj[u] >= 0 ? L.jj[u] : 0;
        const float a0 = __shfl(w0, js, 64), a1 = __shfl(w1, js, 64), a2 = __shfl(w2, js, 64), a3 = __shfl(w3, js, 64);
        float t = tapsP4_blend(L.p4[u], 0, a0, a1, a2, a3, toprow);
        const float gx = tapsP4_blend(L.p4[u], 1, a0, a1, a2, a3, toprow);
        const float gy = tapsP4_blend(L.p4[u], 2, a0, a1, a2, a3, toprow);
        if constexpr (PN) t -= group_sum(t, 16) / 16.0f;  // utilities.cpp:187-188
        if (L.vis[u]) {
          const size_t po = (size_t)(i0 + 4 * ws) * 16;
          __builtin_nontemporal_store(t, T + po + lane);
          __builtin_nontemporal_store(gx, Gx + po + lane);
          __builtin_nontemporal_store(gy, Gy + po + lane);
        }
      }
    };
    Ref4Loads<kU> A, B;
    issue(A, 0);
    for (int sidx = 0; sidx < nsteps; sidx += 2) {
      if (sidx + 1 < nsteps) issue(B, sidx + 1);
      reduce(A, sidx);
      if (sidx + 2 < nsteps) issue(A, sidx + 2);
      if (sidx + 1 < nsteps) reduce(B, sidx + 1);
    }
  }
}

// ---------------------------------------------------------------- util_getPatch(_grad) for callers (NCC scoring etc.)
__global__ __launch_bounds__(kBlock) void k_getpatch(const float *__restrict__ img, const float *__restrict__ dx,
                                                     const float *__restrict__ dy, const float *__restrict__ mids,
                                                     int K, int P, int sw, int dopatchnorm, float *out, float *out_dx,
                                                     float *out_dy) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int n = P * P;
  for (int i = blockIdx.x * kWaves + wave; i < K; i += gridDim.x * kWaves) {
    const Taps tp = make_taps(mids[i], mids[i + K], P / 2);
    const int base = tp.row0 * sw + tp.col0;
    float s = 0.0f;
    for (int q = lane; q < n; q += 64) {
      const int idx = base + (q / P) * sw + (q % P);
      const float t = tap4(img, idx, sw, tp);
      out[(size_t)i * n + q] = t;
      s += t;
      if (dx) out_dx[(size_t)i * n + q] = tap4(dx, idx, sw, tp);
      if (dy) out_dy[(size_t)i * n + q] = tap4(dy, idx, sw, tp);
    }
    if (dopatchnorm) {
      const float mean = wave_sum(s) / (float)n;
      for (int q = lane; q < n; q += 64) out[(size_t)i * n + q] -= mean;
    }
  }
}

// ---------------------------------------------------------------- patch NCC of run_track_nposes (run_track_nposes.cpp:271-355)
// One wave per point: the mean-subtracted patches (util_getPatch with dopatchnorm forced on, :281) around the point's
// position in the backward-most, the reference and the forward-most frame, each scaled to unit norm, and the two
// correlations back-ref / ref-forward combined with the weights nBack^2 / nFwd^2. Only the K correlations leave the
// device. NV = patch values per lane (psz^2 <= 64 NV). Validity tests are the reference's strict ones (:290,:297,:305).
struct NccFrame {
  const float *img;  // padded plane of the frame at the scoring level
};
template <int NV>
__global__ __launch_bounds__(kBlock) void k_ncc(NccFrame fb, NccFrame fr, NccFrame ff, const float *__restrict__ mids,
                                                int K, int P, int sw, float swo, float sho, float w_back, float w_fwd,
                                                float *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int n = P * P;
  for (int i = blockIdx.x * kWaves + wave; i < K; i += gridDim.x * kWaves) {
    float pat[3][NV];
    float nrm[3];
    bool val[3];
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      const float mx = mids[(2 * f) * K + i], my = mids[(2 * f + 1) * K + i];
      val[f] = (mx > 0.0f) & (my > 0.0f) & (mx < swo) & (my < sho);
      const float *img = f == 0 ? fb.img : (f == 1 ? fr.img : ff.img);
      const Taps tp = make_taps(val[f] ? mx : 1.0f, val[f] ? my : 1.0f, P / 2);
      const int base = tp.row0 * sw + tp.col0;
      float s = 0.0f;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int q = lane + 64 * v;
        pat[f][v] = (q < n && val[f]) ? tap4(img, base + (q / P) * sw + (q % P), sw, tp) : 0.0f;
        s += pat[f][v];
      }
      const float mean = wave_sum(s) / (float)n;  // utilities.cpp:111-112
      float ss = 0.0f;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int q = lane + 64 * v;
        pat[f][v] = q < n ? pat[f][v] - mean : 0.0f;
        ss += pat[f][v] * pat[f][v];
      }
      nrm[f] = sqrtf(wave_sum(ss));  // patch.norm()
    }
    float dbr = 0.0f, drf = 0.0f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const float b = pat[0][v] / nrm[0], r = pat[1][v] / nrm[1], f = pat[2][v] / nrm[2];  // patch /= patch.norm()
      if (lane + 64 * v < n) {
        dbr += b * r;
        drf += r * f;
      }
    }
    dbr = wave_sum(dbr);
    drf = wave_sum(drf);
    if (lane == 0) {
      float corr = -1.0f;
      if (val[1]) {
        const float cbr = val[0] ? fmaxf(0.0f, dbr) : -1.0f, w0 = val[0] ? w_back : 0.0f;
        const float crf = val[2] ? fmaxf(0.0f, drf) : -1.0f, w1 = val[2] ? w_fwd : 0.0f;
        corr = fmaxf(0.0f, (cbr * w0 + crf * w1) / (w0 + w1));  // std::max(0.0f, NaN) == 0.0f, as fmaxf
      }
      out[i] = corr;
    }
  }
}
void launch_ncc(const float *img_b, const float *img_r, const float *img_f, const float *mids, int K, int P, int sw,
                float swo, float sho, float w_back, float w_fwd, float *out, hipStream_t s) {
  int gx = (K + kWaves - 1) / kWaves;
  gx = std::max(1, std::min(gx, kMaxGridX));
  const NccFrame fb{img_b}, fr{img_r}, ff{img_f};
  const int n = P * P;
  if (n <= 64)
    hipLaunchKernelGGL((k_ncc<1>), dim3(gx), dim3(kBlock), 0, s, fb, fr, ff, mids, K, P, sw, swo, sho, w_back, w_fwd, out);
  else if (n <= 256)
    hipLaunchKernelGGL((k_ncc<4>), dim3(gx), dim3(kBlock), 0, s, fb, fr, ff, mids, K, P, sw, swo, sho, w_back, w_fwd, out);
  else if (n <= 1024)
    hipLaunchKernelGGL((k_ncc<16>), dim3(gx), dim3(kBlock), 0, s, fb, fr, ff, mids, K, P, sw, swo, sho, w_back, w_fwd, out);
  else
    hipLaunchKernelGGL((k_ncc<64>), dim3(gx), dim3(kBlock), 0, s, fb, fr, ff, mids, K, P, sw, swo, sho, w_back, w_fwd, out);
}

// ---------------------------------------------------------------- Python flow-tracking surface on the device
// func_get_transf_position (misc_src/classoftrack.py:4-34): K sub-pixel points moved by a displacement field sampled
// bilinearly at the points, in float64 with NumPy's operation order (field value widened, times weight, summed left
// to right), so the result is bit-identical to the NumPy restatement and to the reference's goldens. A point whose four
// taps are not all inside the field comes back as NaN. F = float or double (the field's dtype).
template <typename F>
__global__ __launch_bounds__(kBlock) void k_flow_gather(const F *__restrict__ du, const F *__restrict__ dv, int H, int W,
                                                        const double *__restrict__ xy, int K, double *__restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= K) return;
  const double x = xy[2 * i], y = xy[2 * i + 1];
  const double flx = floor(x), fly = floor(y);
  const double nan = __builtin_nan("");
  double ox = nan, oy = nan;
  // NaN / out-of-range coordinates fail the range test (written positively), like the INT_MIN cast in NumPy
  if (flx >= 0.0 && fly >= 0.0 && flx + 1.0 < (double)W && fly + 1.0 < (double)H) {
    const int x0 = (int)flx, y0 = (int)fly, x1 = x0 + 1, y1 = y0 + 1;
    const double fx = x - flx, fy = y - fly;
    const double w0 = fx * fy, w1 = (1 - fx) * fy, w2 = fx * (1 - fy), w3 = (1 - fx) * (1 - fy);
    const size_t a = (size_t)y1 * W + x1, b = (size_t)y1 * W + x0, c = (size_t)y0 * W + x1, d = (size_t)y0 * W + x0;
    ox = x + ((double)du[a] * w0 + (double)du[b] * w1 + (double)du[c] * w2 + (double)du[d] * w3);
    oy = y;
    if (dv) oy = y + ((double)dv[a] * w0 + (double)dv[b] * w1 + (double)dv[c] * w2 + (double)dv[d] * w3);
  }
  out[2 * i] = ox;
  out[2 * i + 1] = oy;
}
void launch_flow_gather(const void *du, const void *dv, int is_f64, int H, int W, const double *xy, int K, double *out,
                        hipStream_t s) {
  const dim3 g((K + kBlock - 1) / kBlock), blk(kBlock);
  if (is_f64)
    hipLaunchKernelGGL((k_flow_gather<double>), g, blk, 0, s, (const double *)du, (const double *)dv, H, W, xy, K, out);
  else
    hipLaunchKernelGGL((k_flow_gather<float>), g, blk, 0, s, (const float *)du, (const float *)dv, H, W, xy, K, out);
}

// func_extract_bil_patch (misc_src/func_OF_util.py:87-129), batched: K points, raw (side x side x C) bilinear patches
// of an (H, W, C) float64 image, side = 2 (pz / 2) (Python-2 integer division), patch-constant weights on four
// integer-shifted windows in NumPy's operation order. One thread per output value; windows that leave the image are
// the caller's error (checked on the host).
__global__ __launch_bounds__(kBlock) void k_bil_patches(const double *__restrict__ img, int H, int W, int C,
                                                        const double *__restrict__ pts, int K, int half,
                                                        double *__restrict__ out) {
  const int side = 2 * half;
  const size_t per = (size_t)side * side * C;
  const size_t n = (size_t)K * per;
  for (size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x; t < n; t += (size_t)gridDim.x * kBlock) {
    const int k = (int)(t / per);
    const size_t r = t - (size_t)k * per;
    const int c = (int)(r % C), px = (int)((r / C) % side), py = (int)(r / ((size_t)C * side));
    const double x = pts[2 * k], y = pts[2 * k + 1];
    const double flx = floor(x), fly = floor(y);
    const double fx = x - flx, fy = y - fly;
    const int x0 = (int)flx - half + px, y0 = (int)fly - half + py;
    const double a = img[((size_t)(y0 + 1) * W + (x0 + 1)) * C + c], b = img[((size_t)(y0 + 1) * W + x0) * C + c];
    const double cc = img[((size_t)y0 * W + (x0 + 1)) * C + c], d = img[((size_t)y0 * W + x0) * C + c];
    out[t] = a * (fx * fy) + b * ((1 - fx) * fy) + cc * (fx * (1 - fy)) + d * ((1 - fx) * (1 - fy));
  }
}
void launch_bil_patches(const double *img, int H, int W, int C, const double *pts, int K, int half, double *out,
                        hipStream_t s) {
  const size_t n = (size_t)K * 4 * half * half * C;
  const int g = (int)std::min<size_t>((n + kBlock - 1) / kBlock, 8192);
  hipLaunchKernelGGL(k_bil_patches, dim3(std::max(g, 1)), dim3(kBlock), 0, s, img, H, W, C, pts, K, half, out);
}

// ---------------------------------------------------------------- pyramid (utilities.cpp:14-52)
__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  if (i < 0) return -i;
  if (i >= n) return 2 * n - 2 - i;
  return i;
}

// One launch per level: every thread owns one pixel of the PADDED level and evaluates the level image where it needs it
// straight from the level above (level 0: the input frame; level l: cv::resize(.5, .5, INTER_LINEAR) == 2x2 box mean for
// even sizes, clamped bilinear otherwise) -- its own value (clamped: replicate padding), and for interior pixels the four
// reflect-101 neighbours of the Sobel pair (cv::Sobel(ksize=1) = I(x+1) - I(x-1), zero padding); the redundant
// evaluations are cache hits, the level is written once (img, dx, dy, packed texel).
template <bool FIRST>
__device__ __forceinline__ float pyr_level_value(const float *__restrict__ src, int pw, int ph, int psw, int pad, int w,
                                                 int h, int x, int y) {
  if constexpr (FIRST) return src[(size_t)y * w + x];
  const float *s = src + (size_t)pad * psw + pad;  // interior origin of the previous level
  if (pw == 2 * w && ph == 2 * h) {
    const float *r0 = s + (size_t)(2 * y) * psw + 2 * x;
    const float *r1 = r0 + psw;
    return ((r0[0] + r1[0]) + (r0[1] + r1[1])) * 0.25f;
  }
  int y0 = 2 * y, y1 = y0 + 1, x0 = 2 * x, x1 = x0 + 1;
  y0 = min(y0, ph - 1);
  y1 = min(y1, ph - 1);
  x0 = min(x0, pw - 1);
  x1 = min(x1, pw - 1);
  const float top = s[(size_t)y0 * psw + x0] * 0.5f + s[(size_t)y0 * psw + x1] * 0.5f;
  const float bot = s[(size_t)y1 * psw + x0] * 0.5f + s[(size_t)y1 * psw + x1] * 0.5f;
  return top * 0.5f + bot * 0.5f;
}
template <bool FIRST>
__global__ __launch_bounds__(kBlock) void k_pyr_level(const float *__restrict__ src, int pw, int ph, int psw, float *img,
                                                      float *dx, float *dy, f32x4_t *pack, int w, int h, int pad, int sw,
                                                      int sh, int getgrad) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = blockIdx.y * kWaves + (threadIdx.x >> 6);
  if (x >= sw || y >= sh) return;
  const int ix = x - pad, iy = y - pad;
  const bool inside = (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h);
  const int cxx = min(max(ix, 0), w - 1), cyy = min(max(iy, 0), h - 1);
  const size_t o = (size_t)y * sw + x;
  const float v = pyr_level_value<FIRST>(src, pw, ph, psw, pad, w, h, cxx, cyy);
  img[o] = v;
  if (!getgrad) return;
  float gx = 0.0f, gy = 0.0f;
  if (inside) {
    gx = pyr_level_value<FIRST>(src, pw, ph, psw, pad, w, h, reflect101(ix + 1, w), iy) -
         pyr_level_value<FIRST>(src, pw, ph, psw, pad, w, h, reflect101(ix - 1, w), iy);
    gy = pyr_level_value<FIRST>(src, pw, ph, psw, pad, w, h, ix, reflect101(iy + 1, h)) -
         pyr_level_value<FIRST>(src, pw, ph, psw, pad, w, h, ix, reflect101(iy - 1, h));
  }
  dx[o] = gx;
  dy[o] = gy;
  const f32x4_t t = {v, gx, gy, 0.0f};
  pack[o] = t;
}

// ---------------------------------------------------------------- host-side launchers
static inline dim3 grid2d(int w, int h) { return dim3((w + 63) / 64, (h + kWaves - 1) / kWaves); }

// plain streaming read (16-byte non-temporal loads, 8 in flight per lane): the practical HBM read ceiling of the
// box, reported next to the vendor peak (ictr_stream_read_bandwidth)
__global__ __launch_bounds__(kBlock) void k_stream_read(const f32x4_t *__restrict__ src, size_t nvec, float *sink) {
  const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x, nth = (size_t)gridDim.x * kBlock;
  float acc = 0.0f;
  size_t i = tid;
  for (; i + 7 * nth < nvec; i += 8 * nth) {
    f32x4_t v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = __builtin_nontemporal_load(src + i + u * nth);
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += (v[u].x + v[u].y) + (v[u].z + v[u].w);
  }
  for (; i < nvec; i += nth) {
    const f32x4_t v = __builtin_nontemporal_load(src + i);
    acc += (v.x + v.y) + (v.z + v.w);
  }
  if (acc == 1.2345e30f) sink[tid] = acc;
}
void launch_stream_read(const float *src, size_t nfloats, float *sink, hipStream_t s) {
  hipLaunchKernelGGL(k_stream_read, dim3(8192), dim3(kBlock), 0, s, reinterpret_cast<const f32x4_t *>(src), nfloats / 4,
                     sink);
}

// interleave a finished level into {img, dx, dy, 0} texels (read by k_ref8's packed taps)
__global__ __launch_bounds__(kBlock) void k_pyr_pack(const float *__restrict__ img, const float *__restrict__ dx,
                                                     const float *__restrict__ dy, f32x4_t *pack, size_t n) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
    f32x4_t v = {img[i], dx[i], dy[i], 0.0f};
    pack[i] = v;
  }
}
void launch_pyr_pack(const float *img, const float *dx, const float *dy, float *pack, size_t n, hipStream_t s) {
  const int g = (int)std::min<size_t>((n + kBlock - 1) / kBlock, 8192);
  hipLaunchKernelGGL(k_pyr_pack, dim3(g), dim3(kBlock), 0, s, img, dx, dy, reinterpret_cast<f32x4_t *>(pack), n);
}
// src: the input frame (first, unpadded, stride w) or the previous level's padded image plane (pw x ph, stride psw)
void launch_pyr_level(const float *src, int first, int pw, int ph, int psw, float *img, float *dx, float *dy,
                      float *pack, int w, int h, int pad, int sw, int sh, int getgrad, hipStream_t s) {
  if (first)
    hipLaunchKernelGGL(k_pyr_level<true>, grid2d(sw, sh), dim3(kBlock), 0, s, src, pw, ph, psw, img, dx, dy,
                       reinterpret_cast<f32x4_t *>(pack), w, h, pad, sw, sh, getgrad);
  else
    hipLaunchKernelGGL(k_pyr_level<false>, grid2d(sw, sh), dim3(kBlock), 0, s, src, pw, ph, psw, img, dx, dy,
                       reinterpret_cast<f32x4_t *>(pack), w, h, pad, sw, sh, getgrad);
}
void launch_getpatch(const float *img, const float *dx, const float *dy, const float *mids, int K, int P, int sw,
                     int dopatchnorm, float *out, float *out_dx, float *out_dy, hipStream_t s) {
  int gx = (K + kWaves - 1) / kWaves;
  if (gx > kMaxGridX) gx = kMaxGridX;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(k_getpatch, dim3(gx), dim3(kBlock), 0, s, img, dx, dy, mids, K, P, sw, dopatchnorm, out, out_dx,
                     out_dy);
}
void launch_project_generic(const float *pt3d, float *pt3d_rot, float *pt2d, int n, int M, const float *G,
                            LevelCam lc, hipStream_t s) {
  hipLaunchKernelGGL(k_project_generic, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, pt3d, pt3d_rot, pt2d, n, M,
                     G, lc);
}
void launch_project_ref(const EngineDev &e, const LevelCam *cams, int maxpts, hipStream_t s) {
  AllCams ac;
  for (int l = 0; l < e.nlev && l < 16; ++l) ac.lc[l] = cams[l];
  hipLaunchKernelGGL(k_project_ref, dim3((maxpts + kBlock - 1) / kBlock, e.B), dim3(kBlock), 0, s, e, ac);
}
// Deferred H: on the wave64 fast paths the level's H partials are reduced and factored by the level's FIRST iteration
// tail (k_iter_tail / k_iter_finish with first_h), not by k_level_tail -- in sharded mode H then travels in the same
// 27-float message as the first b and the level phase needs no collective of its own. Where the partials come from:
// P = 8: the setup kernel k_ref8 (three sums per patch, H = sum J^T S J); P = 4: the first k_iter4<.., WH> launch.
// ICTR_VARIANT_H_BY_SETUP lets k_level_tail reduce and factor H for P = 8 (cross-check in the tests).
// wave64 fast paths: 8x8 always, 4x4 when every reference pyramid carries the packed planes (otf != 2)
static bool fast8(const EngineDev &e, int variant) { return e.P == 8 && !(variant & ICTR_VARIANT_ANY_SIZE); }
static bool fast4(const EngineDev &e, int variant) { return e.P == 4 && e.otf != 2 && !(variant & ICTR_VARIANT_ANY_SIZE); }
bool defer_h(const EngineDev &e, int variant) {
  return (fast8(e, variant) && !(variant & ICTR_VARIANT_H_BY_SETUP)) || fast4(e, variant);
}
// (the host sets ICTR_VARIANT_ANY_SIZE whenever a robustness option is on, see engine_variant in ictr_host.hip)
// the wave64 fast paths leave one partial per workgroup of their own grid, the any-size kernels one per gridx workgroup
int tail_partials(const EngineDev &e, const LevelLaunch &ll) {
  return (fast8(e, ll.variant) || fast4(e, ll.variant)) ? ll.gridx8 : ll.gridx;
}

// steps 4-6 of one level for every problem: accumulate kernel + per-problem tail. tail = false (the resident path on the
// 8x8 fast path): no k_level_tail -- the resident-iteration launch that follows reduces and factors H itself (its solver
// workgroups are idle while the workers load their templates)
void launch_ref_level(const EngineDev &e, const LevelCam &lc, const LevelLaunch &ll, bool tail, hipStream_t s) {
  const dim3 blk(kBlock);
  const int level = ll.level, gridx = ll.gridx, variant = ll.variant, cpw = ll.cpw, gridx8 = ll.gridx8;
  const bool dh = defer_h(e, variant);
  if (fast8(e, variant)) {
    const dim3 g8(gridx8, e.B);
    // gradients on the fly from the image plane whenever the reference pyramids are builder-made (r03: 287 -> 242 us per
    // level-0 launch of 32 pairs; a must for image-only pyramids, e.otf == 2); ICTR_VARIANT_GRAD_PLANES: read the
    // packed planes instead (cross-check). Every pyramid that is not image-only carries the packed planes.
    const bool otf = e.otf == 2 || (e.otf == 1 && !(variant & ICTR_VARIANT_GRAD_PLANES));
    // patches per pipeline step: two with the packed planes (measured r02: 1 -> 2 saves 50-120 us per level, 4 adds
    // nothing), one otherwise
    if (otf && e.dopatchnorm)
      hipLaunchKernelGGL((k_ref8<true, 1, false, true>), g8, blk, 0, s, e, lc, level, cpw);
    else if (otf && cpw % 16 == 0 && !(variant & ICTR_VARIANT_DYNAMIC_LOOP)) {  // (the dynamic patch loop: cross-check)
      // the static form, per level with the reference windows staged through a per-wave LDS tile of this many bytes or
      // (0, and always with ICTR_REF8_DIRECT_TAPS) with the direct taps and their line touches. 32 distinct dense
      // 1080p pairs, us per level 0 / 1 / 2 (profiles/r04_notes.md): direct taps 355 / 275 / 232; 9216 bytes (12 rows x
      // 6 lines, the box of sixteen neighbours of a dense 8-px grid: the most that leaves three workgroups per CU)
      // 260 / 243 / 218; 6016 bytes (four workgroups per CU; the level-0 box does not fit) 448 / 239 / 204; 14592
      // bytes (two) 317 / 298 / 273.
#ifndef ICTR_REF8_TILE0
#define ICTR_REF8_TILE0 9216  // level 0
#endif
#ifndef ICTR_REF8_TILE1
#define ICTR_REF8_TILE1 9216  // level 1
#endif
#ifndef ICTR_REF8_TILE2
#define ICTR_REF8_TILE2 6016  // levels 2 and up (227 / 222 / 221 with the direct taps -> 205 / 195 / 196)
#endif
      const int tb = (variant & ICTR_REF8_DIRECT_TAPS) ? 0 : level == 0 ? ICTR_REF8_TILE0 : level == 1 ? ICTR_REF8_TILE1 : ICTR_REF8_TILE2;
      if (tb != 0 && tb == ICTR_REF8_TILE0)
        hipLaunchKernelGGL((k_ref8<false, 2, false, true, true, ICTR_REF8_TILE0>), g8, blk, 0, s, e, lc, level, cpw);
      else if (tb != 0 && tb == ICTR_REF8_TILE1)
        hipLaunchKernelGGL((k_ref8<false, 2, false, true, true, ICTR_REF8_TILE1>), g8, blk, 0, s, e, lc, level, cpw);
      else if (tb != 0)
        hipLaunchKernelGGL((k_ref8<false, 2, false, true, true, ICTR_REF8_TILE2>), g8, blk, 0, s, e, lc, level, cpw);
      else
        hipLaunchKernelGGL((k_ref8<false, 2, false, true, true>), g8, blk, 0, s, e, lc, level, cpw);
    } else if (otf)
      hipLaunchKernelGGL((k_ref8<false, 2, false, true>), g8, blk, 0, s, e, lc, level, cpw);
    else if (e.dopatchnorm)
      hipLaunchKernelGGL((k_ref8<true, 1, true>), g8, blk, 0, s, e, lc, level, cpw);
    else
      hipLaunchKernelGGL((k_ref8<false, 2, true>), g8, blk, 0, s, e, lc, level, cpw);
  } else if (fast4(e, variant)) {
    if (e.dopatchnorm)
      hipLaunchKernelGGL((k_ref4<true>), dim3(gridx8, e.B), blk, 0, s, e, lc, level, cpw);
    else
      hipLaunchKernelGGL((k_ref4<false>), dim3(gridx8, e.B), blk, 0, s, e, lc, level, cpw);
  } else if (e.P == 4)
    hipLaunchKernelGGL(k_ref_level<4>, dim3(gridx, e.B), blk, 0, s, e, lc, level);
  else
    hipLaunchKernelGGL(k_ref_level<0>, dim3(gridx, e.B), blk, 0, s, e, lc, level);
  if (tail || !fast8(e, variant))
    hipLaunchKernelGGL(k_level_tail, dim3(e.B), blk, 0, s, e, tail_partials(e, ll), dh ? 1 : 0);
}
void launch_level_finish(const EngineDev &e, const LevelLaunch &ll, hipStream_t s) {
  hipLaunchKernelGGL(k_level_finish, dim3(e.B), dim3(64), 0, s, e, defer_h(e, ll.variant) ? 1 : 0);
}
// steps 7-9a of one Gauss-Newton iteration for every problem (the accumulate kernel) ...
// first: the level's first iteration (P = 4 with deferred H: it also accumulates the H partials)
// ev0 / ev1 (optional, timing runs): HIP events that take the kernel's own start and end time stamps (hipExtLaunchKernelGGL:
// the dispatch's completion-signal times, what rocprofv3's kernel trace lists), not the time between two event packets
void launch_iter_main(const EngineDev &e, const LevelCam &lc, const LevelLaunch &ll, int first, hipStream_t s,
                      hipEvent_t ev0, hipEvent_t ev1) {
  const dim3 blk(kBlock);
  const int level = ll.level, gridx = ll.gridx, variant = ll.variant, cpw = ll.cpw, gridx8 = ll.gridx8;
#define ICTR_LAUNCH(kern, grid, ...)                                                      \
  do {                                                                                    \
    if (ev0 && ev1)                                                                       \
      hipExtLaunchKernelGGL(kern, grid, blk, 0, s, ev0, ev1, 0, __VA_ARGS__);             \
    else                                                                                  \
      hipLaunchKernelGGL(kern, grid, blk, 0, s, __VA_ARGS__);                             \
  } while (0)
  if (fast8(e, variant)) {
    const dim3 g8(gridx8, e.B);
    // patches per pipeline step: 4 measured best (profiles/r01_notes.md)
    if (e.dopatchnorm)
      ICTR_LAUNCH((k_iter8<true, 2>), g8, e, lc, level, cpw);
    else
      ICTR_LAUNCH((k_iter8<false, 4>), g8, e, lc, level, cpw);
  } else if (fast4(e, variant)) {
    const dim3 g8(gridx8, e.B);
    if (first) {
      if (e.dopatchnorm)
        ICTR_LAUNCH((k_iter4<true, true>), g8, e, lc, level, cpw);
      else
        ICTR_LAUNCH((k_iter4<false, true>), g8, e, lc, level, cpw);
    } else if (e.dopatchnorm)
      ICTR_LAUNCH((k_iter4<true, false>), g8, e, lc, level, cpw);
    else
      ICTR_LAUNCH((k_iter4<false, false>), g8, e, lc, level, cpw);
  } else if (e.P == 4)
    ICTR_LAUNCH((k_iter<4>), dim3(gridx, e.B), e, lc, level);
  else
    ICTR_LAUNCH((k_iter<0>), dim3(gridx, e.B), e, lc, level);
#undef ICTR_LAUNCH
}
// ... and steps 9b-10 (one workgroup per problem)
void launch_iter_tail(const EngineDev &e, const LevelLaunch &ll, int first, hipStream_t s) {
  hipLaunchKernelGGL(k_iter_tail, dim3(e.B), dim3(kBlock), 0, s, e, ll.level, tail_partials(e, ll),
                     (first && defer_h(e, ll.variant)) ? 1 : 0);
}
void launch_iter_finish(const EngineDev &e, const LevelLaunch &ll, int first, hipStream_t s) {
  hipLaunchKernelGGL(k_iter_finish, dim3(e.B), dim3(64), 0, s, e, ll.level, (first && defer_h(e, ll.variant)) ? 1 : 0);
}

hipError_t launch_debug_wave_solve(const float *H, const float *b, int n, ProbState *st, int through_state, float *x,
                                   int *rank, int *nonzero, int *rowmap, int *colmap, float *lu, hipStream_t s) {
  hipLaunchKernelGGL(k_debug_wave_factor, dim3(n), dim3(64), 0, s, H, b, st, through_state ? 0 : 1, x, rank, nonzero,
                     rowmap, colmap, lu);
  if (through_state)
    hipLaunchKernelGGL(k_debug_wave_apply, dim3(n), dim3(64), 0, s, b, st, x, rank, nonzero, rowmap, colmap, lu);
  return hipGetLastError();
}
hipError_t launch_debug_se3(const float *in, float *out, long long n, int log_not_exp, hipStream_t s) {
  hipLaunchKernelGGL(k_debug_se3, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, in, out, n, log_not_exp);
  return hipGetLastError();
}

}  // namespace ictr
