// ictr_triang.hip -- batched multi-view point triangulation: the four routines of the reference's misc_src/triang.c
// (triangulate_DLT :262-322, triangulate_full3D :193-238, triangulate_full3D_LM :241-259, 327-373,
// triangulate_depthonly :80-132, 378-435) for a whole track set at once.
//
//   k_tri_tiles / k_tri_scan / k_tri_pack   (ictr_triang_set_tracks) the ragged track list -> tile-major slots: the 64
//                    points of a wave form a tile as long as its longest track; slot k of the tile holds observation k
//                    of its 64 points side by side, so a wave reads view / x / y of one slot with one coalesced load each.
//                    Lengths (>= 2) and view indices (< F) are checked here, on the device.
//   k_triang<MODE>   one lane per point, the views of a point a serial loop in that lane. Every product and sum is f32,
//                    in the reference's order and grouping (the library is built with -ffp-contract=off; / and sqrtf are
//                    the correctly rounded sequences), so the results carry the reference binary's bits. The Jacobian and
//                    residual rows the C keeps in malloc'ed arrays are recomputed where they are used (the same
//                    operations on the same inputs give the same bits): an iteration is two sweeps over the views (all
//                    x-rows, then all y-rows), Levenberg-Marquardt adds one per trial point. Camera rows come through the
//                    caches as three 16-byte loads per view. A lane whose stop test fires idles and keeps its result.
//
// One stream, no host wait between the upload of the start points, the kernel and the read-back.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "ictr_dev.h"
#include "ictr_launch.h"

namespace ictr {

constexpr int kTriBlock = 256;  // four waves = four tiles of 64 points

struct TriArgs {
  const float *P;          // [F][12] row-major 3x4
  const long long *off;    // [n + 1]
  const long long *tbase;  // [tiles] first slot word of each tile
  const int *pv;           // tile-major: word tbase[t] + k * 64 + lane = observation k of point t * 64 + lane
  const float *px, *py;
  int n;
  int noiter;
  float minres, damp_init, damp_fct, maxdamp;
  const float *init, *campos, *ptdir;  // [n][3]
  float *pts, *cov;                    // [n][3], [n][9]
  int *iters, *status;                 // [n]
};

struct TriPack {
  const long long *off;  // [n + 1]
  const int *view;       // [M]
  const float *x, *y;
  int n, tiles, F;
  int *tlen;             // [tiles] longest track of the tile
  long long *tbase;      // [tiles]
  long long *meta;       // [0] slot words in all, [1] error bits: 1 = a track of fewer than 2 views, 2 = a view >= F
  int *pv;
  float *px, *py;
};

__global__ void __launch_bounds__(kTriBlock) k_tri_tiles(TriPack a) {
  const int t = blockIdx.x * kTriBlock + threadIdx.x;
  if (t >= a.tiles) return;
  const int p1 = min(a.n, t * 64 + 64);
  long long mx = 0;
  bool bad = false;
  for (int p = t * 64; p < p1; ++p) {
    const long long l = a.off[p + 1] - a.off[p];
    bad |= l < 2;
    mx = max(mx, l);
  }
  a.tlen[t] = (int)mx;
  if (bad) atomicOr((unsigned long long *)&a.meta[1], 1ull);
}

// one workgroup: tbase = 64 x the exclusive prefix sums of tlen
__global__ void __launch_bounds__(kTriBlock) k_tri_scan(TriPack a) {
  __shared__ long long sPart[kTriBlock];
  const int tid = threadIdx.x;
  const int per = (a.tiles + kTriBlock - 1) / kTriBlock;
  const int t0 = min(a.tiles, tid * per), t1 = min(a.tiles, t0 + per);
  long long s = 0;
  for (int t = t0; t < t1; ++t) s += a.tlen[t];
  sPart[tid] = s;
  __syncthreads();
  long long before = 0;
  for (int q = 0; q < tid; ++q) before += sPart[q];
  for (int t = t0; t < t1; ++t) {
    a.tbase[t] = before * 64;
    before += a.tlen[t];
  }
  if (tid == kTriBlock - 1) a.meta[0] = before * 64;
}

__global__ void __launch_bounds__(kTriBlock) k_tri_pack(TriPack a) {
  const int p = blockIdx.x * kTriBlock + threadIdx.x;
  if (p >= a.n) return;
  const long long o = a.off[p], base = a.tbase[p >> 6] + (p & 63);
  const int len = (int)(a.off[p + 1] - o);
  bool bad = false;
  for (int k = 0; k < len; ++k) {
    int v = a.view[o + k];
    if ((unsigned)v >= (unsigned)a.F) {
      bad = true;
      v = 0;
    }
    a.pv[base + (long long)k * 64] = v;
    a.px[base + (long long)k * 64] = a.x[o + k];
    a.py[base + (long long)k * 64] = a.y[o + k];
  }
  if (bad) atomicOr((unsigned long long *)&a.meta[1], 2ull);
}

// ---------------------------------------------------------------- the arithmetic of triang.c, one point per lane
// the observations of one lane: slot k at word k * 64 of its tile column
struct TriLane {
  const float *P;
  const int *pv;
  const float *px, *py;
  int len;
  __device__ __forceinline__ void view(int k, float *p, float &x, float &y) const {
    const float4 *q = reinterpret_cast<const float4 *>(P + (size_t)pv[(size_t)k * 64] * 12);
    const float4 a = q[0], b = q[1], c = q[2];
    p[0] = a.x, p[1] = a.y, p[2] = a.z, p[3] = a.w;
    p[4] = b.x, p[5] = b.y, p[6] = b.z, p[7] = b.w;
    p[8] = c.x, p[9] = c.y, p[10] = c.z, p[11] = c.w;
    x = px[(size_t)k * 64];
    y = py[(size_t)k * 64];
  }
};

// comp_matrix_inverse_3x3_symmetric; m = {m0, m1, m2, m4, m5, m8}
__device__ __forceinline__ void tri_inv3(const float *m, float *inv) {
  const float i0 = m[5] * m[3] - m[4] * m[4];
  const float i1 = m[2] * m[4] - m[5] * m[1];
  const float i2 = m[1] * m[4] - m[2] * m[3];
  const float i4 = m[5] * m[0] - m[2] * m[2];
  const float i5 = m[1] * m[2] - m[0] * m[4];
  const float i8 = m[0] * m[3] - m[1] * m[1];
  const float det = (m[0] * i0 + m[1] * i1) + m[2] * i2;
  inv[0] = i0 / det;
  inv[1] = i1 / det;
  inv[2] = i2 / det;
  inv[3] = i1 / det;
  inv[4] = i4 / det;
  inv[5] = i5 / det;
  inv[6] = i2 / det;
  inv[7] = i5 / det;
  inv[8] = i8 / det;
}

// one row of comp_residuals: obs - proj
template <int ROW>
__device__ __forceinline__ float tri_res_row(const float *p, float o, const float *X) {
  const float n = ((p[4 * ROW] * X[0] + p[4 * ROW + 1] * X[1]) + p[4 * ROW + 2] * X[2]) + p[4 * ROW + 3];
  const float w = ((p[8] * X[0] + p[9] * X[1]) + p[10] * X[2]) + p[11];
  return o - n / w;
}

// one row of comp_jacobian_full_3D (each c?n? term leaves out a different addend)
template <int ROW>
__device__ __forceinline__ void tri_jac_row(const float *p, const float *X, float *j) {
  float den = ((p[8] * X[0] + p[9] * X[1]) + p[10] * X[2]) + p[11];
  den *= den;
  const float *r = p + 4 * ROW;
  const float c0n = (r[1] * X[1] + r[2] * X[2]) + r[3];
  const float c1n = (r[0] * X[0] + r[2] * X[2]) + r[3];
  const float c2n = (r[0] * X[0] + r[1] * X[1]) + r[3];
  const float c0n2 = (p[9] * X[1] + p[10] * X[2]) + p[11];
  const float c1n2 = (p[8] * X[0] + p[10] * X[2]) + p[11];
  const float c2n2 = (p[8] * X[0] + p[9] * X[1]) + p[11];
  j[0] = (r[0] * c0n2 - p[8] * c0n) / den;
  j[1] = (r[1] * c1n2 - p[9] * c1n) / den;
  j[2] = (r[2] * c2n2 - p[10] * c2n) / den;
}

// comp_residuals' res_msq at X
__device__ __forceinline__ float tri_res_msq(const TriLane &L, const float *X) {
  float s = 0.0f;
  for (int k = 0; k < L.len; ++k) {
    float p[12], x, y;
    L.view(k, p, x, y);
    const float rx = tri_res_row<0>(p, x, X), ry = tri_res_row<1>(p, y, X);
    s += rx * rx + ry * ry;
  }
  return s / (float)(2 * L.len);
}

// comp_jactjac (h = the 6 unique sums, when JTJ) and compute_update_vector's J^T r, with the Jacobian at X and the
// residuals at Xr: all x-rows in view order, then all y-rows. RES: also res_msq at Xr, gathered in the x-row sweep.
template <int ROW, bool JTJ, bool RES>
__device__ __forceinline__ void tri_sweep(const TriLane &L, const float *X, const float *Xr, float *h, float *g,
                                          float &res) {
  for (int k = 0; k < L.len; ++k) {
    float p[12], x, y, j[3];
    L.view(k, p, x, y);
    tri_jac_row<ROW>(p, X, j);
    const float r = tri_res_row<ROW>(p, ROW == 0 ? x : y, Xr);
    if (RES) {
      const float ry = tri_res_row<1>(p, y, Xr);
      res += r * r + ry * ry;
    }
    if (JTJ) {
      h[0] += j[0] * j[0];
      h[1] += j[0] * j[1];
      h[2] += j[0] * j[2];
      h[3] += j[1] * j[1];
      h[4] += j[1] * j[2];
      h[5] += j[2] * j[2];
    }
    g[0] += j[0] * r;
    g[1] += j[1] * r;
    g[2] += j[2] * r;
  }
}
template <bool JTJ, bool RES>
__device__ __forceinline__ void tri_normal_sums(const TriLane &L, const float *X, const float *Xr, float *h, float *g,
                                                float &res) {
  if (JTJ)
    for (int q = 0; q < 6; ++q) h[q] = 0.0f;
  g[0] = g[1] = g[2] = 0.0f;
  if (RES) res = 0.0f;
  tri_sweep<0, JTJ, RES>(L, X, Xr, h, g, res);
  tri_sweep<1, JTJ, false>(L, X, Xr, h, g, res);
  if (RES) res /= (float)(2 * L.len);
}

// comp_LM_update up to its residual call: the damped inverse (into cov) and out = X + step
__device__ __forceinline__ void tri_lm_step(const float *h, float damp, const float *g, const float *X, float *cov,
                                            float *out) {
  const float m[6] = {h[0] + damp * h[0], h[1], h[2], h[3] + damp * h[3], h[4], h[5] + damp * h[5]};
  tri_inv3(m, cov);
  out[0] = X[0] + ((cov[0] * g[0] + cov[1] * g[1]) + cov[2] * g[2]);
  out[1] = X[1] + ((cov[1] * g[0] + cov[4] * g[1]) + cov[5] * g[2]);
  out[2] = X[2] + ((cov[2] * g[0] + cov[5] * g[1]) + cov[8] * g[2]);
}

template <int MODE>
__global__ void __launch_bounds__(kTriBlock) k_triang(TriArgs a) {
  const int pid = blockIdx.x * kTriBlock + threadIdx.x;
  if (pid >= a.n) return;
  const long long base = a.tbase[pid >> 6] + (pid & 63);
  TriLane L;
  L.P = a.P;
  L.pv = a.pv + base;
  L.px = a.px + base;
  L.py = a.py + base;
  L.len = (int)(a.off[pid + 1] - a.off[pid]);
  float X[3], cov[9];
  for (int q = 0; q < 9; ++q) cov[q] = 0.0f;
  int it = 0;
  if (MODE == ICTR_TRIANG_DLT) {
    float h[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, g[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int row = 0; row < 2; ++row)
      for (int k = 0; k < L.len; ++k) {
        float p[12], x, y;
        L.view(k, p, x, y);
        const float o = row == 0 ? x : y;
        const float *r = p + 4 * row;
        const float a0 = o * p[8] - r[0], a1 = o * p[9] - r[1], a2 = o * p[10] - r[2], a3 = o * p[11] - r[3];
        h[0] += a0 * a0;
        h[1] += a0 * a1;
        h[2] += a0 * a2;
        h[3] += a1 * a1;
        h[4] += a1 * a2;
        h[5] += a2 * a2;
        g[0] -= a0 * a3;
        g[1] -= a1 * a3;
        g[2] -= a2 * a3;
      }
    tri_inv3(h, cov);
    X[0] = (cov[0] * g[0] + cov[1] * g[1]) + cov[2] * g[2];
    X[1] = (cov[3] * g[0] + cov[4] * g[1]) + cov[5] * g[2];
    X[2] = (cov[6] * g[0] + cov[7] * g[1]) + cov[8] * g[2];
  } else {
    for (int c = 0; c < 3; ++c) X[c] = a.init[(size_t)pid * 3 + c];
    float res = INFINITY;  // the C's `float res_msq = 1e300`
    if (MODE == ICTR_TRIANG_GN) {
      for (; it < a.noiter && res > a.minres; ++it) {
        float h[6], g[3];
        tri_normal_sums<true, true>(L, X, X, h, g, res);
        tri_inv3(h, cov);
        X[0] += (cov[0] * g[0] + cov[1] * g[1]) + cov[2] * g[2];
        X[1] += (cov[1] * g[0] + cov[4] * g[1]) + cov[5] * g[2];
        X[2] += (cov[2] * g[0] + cov[5] * g[1]) + cov[8] * g[2];
      }
    } else if (MODE == ICTR_TRIANG_LM) {
      float damp = a.damp_init;
      float res_old = tri_res_msq(L, X);
      for (; it < a.noiter && res > a.minres && damp < a.maxdamp; ++it) {
        float h[6], g[3], Xt[3], dummy = 0.0f;
        tri_normal_sums<true, false>(L, X, X, h, g, dummy);  // the stored residuals are those at X
        tri_lm_step(h, damp, g, X, cov, Xt);
        res = tri_res_msq(L, Xt);
        if (res < res_old - a.minres) {
          damp /= a.damp_fct;
          for (int c = 0; c < 3; ++c) X[c] = Xt[c];
        } else {
          // the trial has overwritten the residual vector: the second step multiplies the Jacobian taken at X with
          // the residuals at the trial point, and is applied whatever it gives
          damp *= a.damp_fct;
          tri_normal_sums<false, false>(L, X, Xt, h, g, dummy);
          tri_lm_step(h, damp, g, X, cov, X);
          res = tri_res_msq(L, X);
        }
        res_old = res;
      }
    } else {
      float c[3], d[3];
      for (int q = 0; q < 3; ++q) {
        c[q] = a.campos[(size_t)pid * 3 + q];
        d[q] = a.ptdir[(size_t)pid * 3 + q];
      }
      const float j0 = X[0] - c[0], j1 = X[1] - c[1], j2 = X[2] - c[2];
      float depth = sqrtf((j0 * j0 + j1 * j1) + j2 * j2);
      for (int q = 0; q < 3; ++q) X[q] = d[q] * depth + c[q];
      for (; it < a.noiter && res > a.minres; ++it) {
        float jtj = 0.0f, dp = 0.0f;
        res = 0.0f;
        for (int k = 0; k < L.len; ++k) {
          float p[12], x, y;
          L.view(k, p, x, y);
          const float rx = tri_res_row<0>(p, x, X), ry = tri_res_row<1>(p, y, X);
          res += rx * rx + ry * ry;
          // prep_jacobian_depth_only's terms do not depend on the depth: recomputed, the same bits every time
          const float den1 = ((p[8] * c[0] + p[9] * c[1]) + p[10] * c[2]) + p[11];
          const float den2 = (p[8] * d[0] + p[9] * d[1]) + p[10] * d[2];
          const float aa0 = (p[0] * d[0] + p[1] * d[1]) + p[2] * d[2];
          const float aa1 = (p[4] * d[0] + p[5] * d[1]) + p[6] * d[2];
          const float bb0 = ((p[0] * c[0] + p[1] * c[1]) + p[2] * c[2]) + p[3];
          const float bb1 = ((p[4] * c[0] + p[5] * c[1]) + p[6] * c[2]) + p[7];
          const float n0 = aa0 * den1 - bb0 * den2, n1 = aa1 * den1 - bb1 * den2;
          float den = den2 * depth + den1;
          den *= den;
          const float q0 = n0 / den, q1 = n1 / den;
          jtj += q0 * q0 + q1 * q1;
          dp += q0 * rx + q1 * ry;
        }
        res /= (float)(2 * L.len);
        cov[0] = 1.0f / jtj;
        dp *= cov[0];
        depth += dp;
        for (int q = 0; q < 3; ++q) X[q] = d[q] * depth + c[q];
      }
    }
  }
  bool finite = isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]);
  for (int q = 0; q < 9; ++q) finite = finite && isfinite(cov[q]);
  float p[12], x, y;
  L.view(0, p, x, y);
  const float w = ((p[8] * X[0] + p[9] * X[1]) + p[10] * X[2]) + p[11];
  for (int c = 0; c < 3; ++c) a.pts[(size_t)pid * 3 + c] = X[c];
  for (int q = 0; q < 9; ++q) a.cov[(size_t)pid * 9 + q] = cov[q];
  a.iters[pid] = it;
  a.status[pid] = (finite ? 0 : ICTR_TRIANG_NONFINITE) | (w <= 0.0f ? ICTR_TRIANG_BEHIND : 0);
}

static void launch_triang(int mode, const TriArgs &a, hipStream_t s) {
  const dim3 grid((a.n + kTriBlock - 1) / kTriBlock), block(kTriBlock);
  if (mode == ICTR_TRIANG_DLT) hipLaunchKernelGGL(k_triang<ICTR_TRIANG_DLT>, grid, block, 0, s, a);
  else if (mode == ICTR_TRIANG_GN) hipLaunchKernelGGL(k_triang<ICTR_TRIANG_GN>, grid, block, 0, s, a);
  else if (mode == ICTR_TRIANG_LM) hipLaunchKernelGGL(k_triang<ICTR_TRIANG_LM>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(k_triang<ICTR_TRIANG_DEPTH>, grid, block, 0, s, a);
}

}  // namespace ictr

using namespace ictr;

// ---------------------------------------------------------------- host side
struct ictr_triang {
  int64_t max_points = 0, max_obs = 0, max_frames = 0;
  int64_t n = 0, m = 0, F = 0, packed_cap = 0;
  DevBuf<float> d_P;
  DevBuf<long long> d_off, d_tbase, d_meta;
  DevBuf<int> d_view, d_tlen, d_pv;
  DevBuf<float> d_x, d_y, d_px, d_py;
  DevBuf<float> d_in;  // init | campos | ptdir, [max_points][3] each
  PinBuf<float> h_in;
  bool cams_set = false, tracks_set = false;
  Readback out;  // (tri_layout) declared last, so destroyed first: a run in flight ends before a buffer goes
};

struct TriLayout {  // pts [n][3] | cov [n][9] | iters [n] | status [n], packed
  Part pts, cov, iters, status, end;  // end: empty, at the block's size
};
static TriLayout tri_layout(int64_t n) {
  Carve c;
  const size_t f = sizeof(float) * (size_t)n, i = sizeof(int32_t) * (size_t)n;
  return {c.take(3 * f), c.take(9 * f), c.take(i), c.take(i), c.take(0)};  // braces: evaluated in this order
}

extern "C" int ictr_triang_create(ictr_triang **out, int64_t max_points, int64_t max_obs, int64_t max_frames) {
  if (!out) return fail(ICTR_ERR_INVALID, "triang_create: NULL argument");
  if (max_points < 1 || max_points > ((int64_t)1 << 24))
    return fail(ICTR_ERR_INVALID, "triang_create: max_points %lld (1 .. 2^24)", (long long)max_points);
  if (max_obs < 2 * max_points || max_obs > ((int64_t)1 << 28))
    return fail(ICTR_ERR_INVALID, "triang_create: max_obs %lld (2 * max_points .. 2^28)", (long long)max_obs);
  if (max_frames < 1 || max_frames > ((int64_t)1 << 20))
    return fail(ICTR_ERR_INVALID, "triang_create: max_frames %lld (1 .. 2^20)", (long long)max_frames);
  if (int rc = need_device()) return rc;
  auto t = std::make_unique<ictr_triang>();
  t->max_points = max_points;
  t->max_obs = max_obs;
  t->max_frames = max_frames;
  const size_t N = (size_t)max_points, M = (size_t)max_obs, tiles = (N + 63) / 64;
  if (int rc = t->d_P.alloc(sizeof(float) * 12 * (size_t)max_frames)) return rc;
  if (int rc = t->d_off.alloc(sizeof(long long) * (N + 1))) return rc;
  if (int rc = t->d_tbase.alloc(sizeof(long long) * tiles)) return rc;
  if (int rc = t->d_tlen.alloc(sizeof(int) * tiles)) return rc;
  if (int rc = t->d_meta.alloc(sizeof(long long) * 2)) return rc;
  if (int rc = t->d_view.alloc(sizeof(int) * M)) return rc;
  if (int rc = t->d_x.alloc(sizeof(float) * M)) return rc;
  if (int rc = t->d_y.alloc(sizeof(float) * M)) return rc;
  if (int rc = t->d_in.alloc(sizeof(float) * 9 * N)) return rc;
  if (int rc = t->h_in.alloc(sizeof(float) * 9 * N)) return rc;
  if (int rc = t->out.reserve(tri_layout(max_points).end.at, false)) return rc;
  *out = t.release();
  return ICTR_OK;
}

extern "C" void ictr_triang_destroy(ictr_triang *t) { delete t; }

extern "C" int ictr_triang_set_cameras(ictr_triang *t, const float *P, int64_t nframes) {
  if (!t || !P) return fail(ICTR_ERR_INVALID, "triang_set_cameras: NULL argument");
  if (int rc = t->out.refuse("triang_set_cameras", "triang")) return rc;
  if (nframes < 1 || nframes > t->max_frames)
    return fail(ICTR_ERR_INVALID, "triang_set_cameras: %lld frames (1 .. %lld, the size given at creation)",
                (long long)nframes, (long long)t->max_frames);
  HIPCHK(hipMemcpy(t->d_P.get(), P, sizeof(float) * 12 * (size_t)nframes, hipMemcpyHostToDevice));
  if (nframes < t->F) t->tracks_set = false;  // the tracks were checked against more frames
  t->F = nframes;
  t->cams_set = true;
  return ICTR_OK;
}

extern "C" int ictr_triang_set_tracks(ictr_triang *t, int64_t n, const int64_t *offsets, const int32_t *view,
                                      const float *x, const float *y) {
  if (!t || !offsets || !view || !x || !y) return fail(ICTR_ERR_INVALID, "triang_set_tracks: NULL argument");
  if (int rc = t->out.refuse("triang_set_tracks", "triang")) return rc;
  if (!t->cams_set) return fail(ICTR_ERR_STATE, "triang_set_tracks: ictr_triang_set_cameras has not been called");
  if (n < 1 || n > t->max_points)
    return fail(ICTR_ERR_INVALID, "triang_set_tracks: %lld points (1 .. %lld, the size given at creation)", (long long)n,
                (long long)t->max_points);
  const int64_t M = offsets[n];
  if (offsets[0] != 0 || M < 2 * n || M > t->max_obs)
    return fail(ICTR_ERR_INVALID,
                "triang_set_tracks: offsets run from %lld to %lld (0 .. at least 2 views per point, at most %lld, the "
                "size given at creation)", (long long)offsets[0], (long long)M, (long long)t->max_obs);
  t->tracks_set = false;
  HIPCHK(hipMemcpy(t->d_off.get(), offsets, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(t->d_view.get(), view, sizeof(int32_t) * (size_t)M, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(t->d_x.get(), x, sizeof(float) * (size_t)M, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(t->d_y.get(), y, sizeof(float) * (size_t)M, hipMemcpyHostToDevice));
  TriPack a;
  a.off = t->d_off.get();
  a.view = t->d_view.get();
  a.x = t->d_x.get();
  a.y = t->d_y.get();
  a.n = (int)n;
  a.tiles = (int)((n + 63) / 64);
  a.F = (int)t->F;
  a.tlen = t->d_tlen.get();
  a.tbase = t->d_tbase.get();
  a.meta = t->d_meta.get();
  a.pv = nullptr;
  a.px = a.py = nullptr;
  HIPCHK(hipMemset(t->d_meta.get(), 0, sizeof(long long) * 2));
  hipLaunchKernelGGL(k_tri_tiles, dim3((a.tiles + kTriBlock - 1) / kTriBlock), dim3(kTriBlock), 0, nullptr, a);
  hipLaunchKernelGGL(k_tri_scan, dim3(1), dim3(kTriBlock), 0, nullptr, a);
  HIPCHK(hipGetLastError());
  long long meta[2] = {0, 0};
  HIPCHK(hipMemcpy(meta, t->d_meta.get(), sizeof(meta), hipMemcpyDeviceToHost));
  if (meta[1] & 1) return fail(ICTR_ERR_INVALID, "triang_set_tracks: a track has fewer than 2 views");
  // every length is >= 2 and the offsets end at M: they ascend inside 0 .. M, and no tile is longer than M
  if (meta[0] < 64 || meta[0] > 64 * M || meta[0] > ((long long)1 << 31))
    return fail(ICTR_ERR_INVALID, "triang_set_tracks: the tile-major track table needs %lld slots (at most 2^31)", meta[0]);
  if (meta[0] > t->packed_cap) {
    t->packed_cap = 0;
    t->d_pv.reset();
    t->d_px.reset();
    t->d_py.reset();
    if (int rc = t->d_pv.alloc(sizeof(int) * (size_t)meta[0])) return rc;
    if (int rc = t->d_px.alloc(sizeof(float) * (size_t)meta[0])) return rc;
    if (int rc = t->d_py.alloc(sizeof(float) * (size_t)meta[0])) return rc;
    t->packed_cap = meta[0];
  }
  a.pv = t->d_pv.get();
  a.px = t->d_px.get();
  a.py = t->d_py.get();
  // slots beyond a track's end are never read; the index table still starts from zeros, not from stale words
  HIPCHK(hipMemset(t->d_pv.get(), 0, sizeof(int) * (size_t)meta[0]));
  hipLaunchKernelGGL(k_tri_pack, dim3((a.n + kTriBlock - 1) / kTriBlock), dim3(kTriBlock), 0, nullptr, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(meta, t->d_meta.get(), sizeof(meta), hipMemcpyDeviceToHost));
  if (meta[1] & 2)
    return fail(ICTR_ERR_INVALID, "triang_set_tracks: a view index is outside 0 .. %lld (the frames set)",
                (long long)t->F - 1);
  t->n = n;
  t->m = M;
  t->tracks_set = true;
  return ICTR_OK;
}

extern "C" int ictr_triang_run(ictr_triang *t, int mode, const ictr_triang_params *params, const float *init_pts,
                               const float *campos, const float *ptdir, void *hip_stream) {
  if (!t) return fail(ICTR_ERR_INVALID, "triang is NULL");
  if (int rc = t->out.refuse("triang_run", "triang")) return rc;
  if (mode < ICTR_TRIANG_DLT || mode > ICTR_TRIANG_DEPTH) return fail(ICTR_ERR_INVALID, "triang_run: mode %d (0 .. 3)", mode);
  if (!t->cams_set || !t->tracks_set)
    return fail(ICTR_ERR_STATE, "triang_run: cameras and tracks have to be set first");
  const bool iterative = mode != ICTR_TRIANG_DLT;
  if (iterative) {
    if (!params) return fail(ICTR_ERR_INVALID, "triang_run: an iterative mode needs its parameters");
    if (!init_pts) return fail(ICTR_ERR_INVALID, "triang_run: an iterative mode needs initial points");
    if (params->noiter < 0 || params->noiter > 100000)
      return fail(ICTR_ERR_INVALID, "triang_run: noiter %d (0 .. 100000)", (int)params->noiter);
    if (mode == ICTR_TRIANG_DEPTH && (!campos || !ptdir))
      return fail(ICTR_ERR_INVALID, "triang_run: the depth-only mode needs camera centres and rays");
  }
  hipStream_t s = (hipStream_t)hip_stream;
  const size_t n = (size_t)t->n;
  TriArgs a;
  memset(&a, 0, sizeof(a));
  a.P = t->d_P.get();
  a.off = t->d_off.get();
  a.tbase = t->d_tbase.get();
  a.pv = t->d_pv.get();
  a.px = t->d_px.get();
  a.py = t->d_py.get();
  a.n = (int)t->n;
  if (iterative) {
    a.noiter = params->noiter;
    a.minres = params->minres;
    a.damp_init = params->damp_init;
    a.damp_fct = params->damp_fct;
    a.maxdamp = params->maxdamp;
    // through the object's pinned buffer: the copies below are then asynchronous for any caller memory
    memcpy(t->h_in.get(), init_pts, sizeof(float) * 3 * n);
    size_t words = 3 * n;
    if (mode == ICTR_TRIANG_DEPTH) {
      memcpy(t->h_in.get() + 3 * n, campos, sizeof(float) * 3 * n);
      memcpy(t->h_in.get() + 6 * n, ptdir, sizeof(float) * 3 * n);
      words = 9 * n;
    }
    HIPCHK(hipMemcpyAsync(t->d_in.get(), t->h_in.get(), sizeof(float) * words, hipMemcpyHostToDevice, s));
    a.init = t->d_in.get();
    a.campos = t->d_in.get() + 3 * n;
    a.ptdir = t->d_in.get() + 6 * n;
  }
  const TriLayout L = tri_layout(t->n);
  a.pts = reinterpret_cast<float *>(t->out.dev() + L.pts.at);
  a.cov = reinterpret_cast<float *>(t->out.dev() + L.cov.at);
  a.iters = reinterpret_cast<int *>(t->out.dev() + L.iters.at);
  a.status = reinterpret_cast<int *>(t->out.dev() + L.status.at);
  launch_triang(mode, a, s);
  HIPCHK(hipGetLastError());
  return t->out.post(L.end.at, s);
}

extern "C" int ictr_triang_wait(ictr_triang *t, float *pts, float *cov, int32_t *iters, int32_t *status) {
  if (!t) return fail(ICTR_ERR_INVALID, "triang is NULL");
  if (!t->out.pending()) return fail(ICTR_ERR_STATE, "triang_wait: nothing has been run");
  if (int rc = t->out.wait()) return rc;
  const TriLayout L = tri_layout(t->n);
  if (pts) memcpy(pts, t->out.host() + L.pts.at, L.pts.bytes);
  if (cov) memcpy(cov, t->out.host() + L.cov.at, L.cov.bytes);
  if (iters) memcpy(iters, t->out.host() + L.iters.at, L.iters.bytes);
  if (status) memcpy(status, t->out.host() + L.status.at, L.status.bytes);
  return ICTR_OK;
}

// ---------------------------------------------------------------- the reference's four entry points, one point each
// Layouts as libtriang.so: P [12][noviews], pt2d [2][noviews], pt3d in place. The same kernels on a batch of one.
static int tri_single(int mode, float *pt3d, float *cov, const float *campos, const float *ptdir, const float *pt2d,
                      const float *P, int noviews, const ictr_triang_params *prm) {
  if (!pt3d || !cov || !pt2d || !P) return fail(ICTR_ERR_INVALID, "triangulate: NULL argument");
  if (noviews < 2 || noviews > (1 << 20)) return fail(ICTR_ERR_INVALID, "triangulate: %d views (2 .. 2^20)", noviews);
  ictr_triang *t = nullptr;
  if (int rc = ictr_triang_create(&t, 1, noviews, noviews)) return rc;
  const std::unique_ptr<ictr_triang> own(t);
  std::vector<float> Pt((size_t)noviews * 12);
  std::vector<int32_t> view((size_t)noviews);
  for (int v = 0; v < noviews; ++v) {
    view[v] = v;
    for (int q = 0; q < 12; ++q) Pt[(size_t)v * 12 + q] = P[(size_t)q * noviews + v];
  }
  const int64_t off[2] = {0, noviews};
  float out[3], c9[9];
  int32_t it = 0;
  int rc = ictr_triang_set_cameras(t, Pt.data(), noviews);
  if (!rc) rc = ictr_triang_set_tracks(t, 1, off, view.data(), pt2d, pt2d + noviews);
  if (!rc) rc = ictr_triang_run(t, mode, prm, pt3d, campos, ptdir, nullptr);
  if (!rc) rc = ictr_triang_wait(t, out, c9, &it, nullptr);
  if (rc) return rc;
  memcpy(pt3d, out, sizeof(out));
  // a loop that never ran leaves the caller's covariance as it was, as the reference does
  if (mode == ICTR_TRIANG_DLT || it > 0) memcpy(cov, c9, sizeof(float) * (mode == ICTR_TRIANG_DEPTH ? 1 : 9));
  return ICTR_OK;
}

extern "C" int ictr_triangulate_DLT(float *pt3d, float *AtAinv, const float *pt2d, const float *P, const int noviews) {
  return tri_single(ICTR_TRIANG_DLT, pt3d, AtAinv, nullptr, nullptr, pt2d, P, noviews, nullptr);
}

extern "C" int ictr_triangulate_full3D(float *pt3d, float *pt3d_cov, const float *pt2d, const float *P, const int noviews,
                                       const int noiter, const float minres) {
  const ictr_triang_params prm = {noiter, minres, 0.0f, 0.0f, 0.0f};
  return tri_single(ICTR_TRIANG_GN, pt3d, pt3d_cov, nullptr, nullptr, pt2d, P, noviews, &prm);
}

extern "C" int ictr_triangulate_full3D_LM(float *pt3d, float *pt3d_cov, const float *pt2d, const float *P,
                                          const int noviews, const int noiter, const float damp_init,
                                          const float damp_fct, const float minres, const float maxdamp) {
  const ictr_triang_params prm = {noiter, minres, damp_init, damp_fct, maxdamp};
  return tri_single(ICTR_TRIANG_LM, pt3d, pt3d_cov, nullptr, nullptr, pt2d, P, noviews, &prm);
}

extern "C" int ictr_triangulate_depthonly(float *pt3d, float *depth_cov, const float *campos, const float *ptdir,
                                          const float *pt2d, const float *P, const int noviews, const int noiter,
                                          const float minres) {
  if (!campos || !ptdir) return fail(ICTR_ERR_INVALID, "triangulate_depthonly: NULL argument");
  const ictr_triang_params prm = {noiter, minres, 0.0f, 0.0f, 0.0f};
  return tri_single(ICTR_TRIANG_DEPTH, pt3d, depth_cov, campos, ptdir, pt2d, P, noviews, &prm);
}
