// ictr_densify.hip -- photometric densification of a patch flow grid at level 0 (DESIGN.md §4 "Densification of a flow
// grid"). The rule is build-defined; its statement of record is patchflow.densify_flow_host (NumPy, f64). This file is the
// same rule in f32 with one fixed operation order, restated in NumPy f32 by tests/densify_f32.py.
//
// k_densify, one launch per field: a lane per pixel, one wave per 64 consecutive pixels of a row, four rows per workgroup
// (k_fr_warp's mapping). Node (i, j) at (X, Y) = step / 2 + (i, j) step covers the pixels X - (psz - psz / 2) ..
// X + psz / 2 - 1 (and Y likewise): the pixels k_patchflow samples at an integer centre. The records (dx, dy) of the nodes
// whose footprint reaches the workgroup's 64 x 4 pixels are staged once in LDS, a lost node as dx = NaN: its position is
// then not inside, which is how a vote is dropped anyway. A lane walks its covering nodes in ascending node row, then
// ascending node column, warps B by each node's displacement (fr_bilinear, the refinement's warp) and weighs it with
// wgt = 1 / max(|Bw - A|, minerr)^power. A pixel without a vote takes fg_value. f32 throughout.
// The mean is taken about the pixel's first vote d0: F = d0 + sum(wgt (d - d0)) / sum(wgt), which is sum(wgt d) / sum(wgt).
// In f32 the plain form carries one rounding per vote into a value of d's size: a constant table came back up to 18 ulp
// off over the 64 votes of psz 32 at step 4, and a single vote an ulp off. About d0 the roundings act on the differences:
// a constant table and a single vote come back to the bit (d - d0 = 0, and d0 + 0 = d0; a d0 of -0.0 comes back +0.0).
// B's taps come from global memory: neighbouring lanes share the node for most votes, so a vote's four tap loads of a
// wave are four contiguous row segments. Plain vector loads and stores, no atomics; enqueued on the caller's stream.
// k_densify<BIAS, NCH>: BIAS is the form of the coarse-to-fine flow's patch-mean normalisation, where the record carries
// the node's brightness offset beta next to (dx, dy) and the residual is (Bw - A) - beta (tests/patnorm_f32.py restates
// it). NCH = 3 is the form of the coarse-to-fine flow's colour frames (DESIGN.md "Colour"): three planes per frame and,
// with BIAS, three betas per node; a vote warps the three channels of B at ONE position, with one inside decision, and
// weighs the channel mean e = ((|r0| + |r1|) + |r2|) / 3 of r_c = (Bw_c - A_c)(- beta_c), so that minerr keeps its meaning
// in grey levels (tests/c2frgb_f32.py restates it).
#include <math.h>
#include <string.h>

#include <memory>
#include <type_traits>

#include "ictr_dev.h"
#include "ictr_launch.h"
#include "ictr_flowgrid_dev.h"
#include "ictr_warp_dev.h"

namespace ictr {

constexpr int kDzMaxPsz = 32;          // the tracker's forms allow 1 .. 32
constexpr size_t kDzMaxLds = 65536;    // bytes of LDS a workgroup may ask for

template <int NCH>
struct DzArgsT {
  const float *A[NCH], *B[NCH];  // per channel, level planes at pixel (0, 0), strides sa, sb
  int sa, sb, w, h;
  FgDev g;
  const unsigned char *lost;  // [ny][nx]
  int lo, hi;                 // a node at X covers X - lo .. X + hi
  float minerr;
  int power;
  float2 *out;       // [h][w]
  float *cnt, *sw;   // [h][w]: votes taken, and their summed weight
  const float *bias; // [ny][nx][NCH] node brightness offsets (k_densify<true, NCH> only)
};

// the nodes i >= 0 with a <= i step, and those i <= n - 1 with i step <= b (-1: none)
__host__ __device__ __forceinline__ int dz_first(int a, int step) { return a <= 0 ? 0 : (a + step - 1) / step; }
__host__ __device__ __forceinline__ int dz_last(int b, int step, int n) { return b < 0 ? -1 : min(b / step, n - 1); }
// the most nodes along an axis whose footprints reach `span` consecutive pixels: node positions step apart in an interval
// of span - 1 + psz - 1 pixels
static int dz_capacity(int span, int psz, int step) { return (span + psz - 2) / step + 1; }

// the LDS record of a node: (dx, dy), and with BIAS the node's brightness offsets beta next to them
template <int NCH>
struct DzRecBias {
  float x, y, beta[NCH];
};
template <bool BIAS, int NCH>
using DzRec = std::conditional_t<BIAS, DzRecBias<NCH>, float2>;

// BIAS: the vote weighs |Bw - A - beta| with the node's beta (the coarse-to-fine flow under patch-mean normalisation).
// NCH: the planes per frame. The rule's only fork is how e is formed: one channel takes |r|, with no division.
// The body of k_densify (below) for one member, whose arguments it takes by value.
template <bool BIAS, int NCH>
__device__ __forceinline__ void dz_body(DzArgsT<NCH> a) {
  static_assert(NCH == 1 || NCH == 3, "one channel or three");
  extern __shared__ float2 s_node_raw[];  // [ncy][ncx] records of the nodes i0 .. i1 x j0 .. j1
  DzRec<BIAS, NCH> *s_node = reinterpret_cast<DzRec<BIAS, NCH> *>(s_node_raw);
  const int step = a.g.step, half = step / 2;
  const int bx0 = blockIdx.x * 64, by0 = blockIdx.y * kWaves;
  const int i0 = dz_first(bx0 - a.hi - half, step), i1 = dz_last(bx0 + 63 + a.lo - half, step, a.g.nx);
  const int j0 = dz_first(by0 - a.hi - half, step), j1 = dz_last(by0 + kWaves - 1 + a.lo - half, step, a.g.ny);
  const int ncx = max(i1 - i0 + 1, 0), ncy = max(j1 - j0 + 1, 0);
  const float nanv = __int_as_float(0x7fc00000);
  for (int q = threadIdx.x; q < ncx * ncy; q += kBlock) {
    const int jj = q / ncx, ii = q - jj * ncx;
    const int k = (j0 + jj) * a.g.nx + (i0 + ii);
    float2 d = reinterpret_cast<const float2 *>(a.g.d)[k];
    if (a.lost[k]) d.x = nanv;
    if constexpr (BIAS) {
      DzRecBias<NCH> rec{d.x, d.y, {}};
#pragma unroll
      for (int c = 0; c < NCH; ++c) rec.beta[c] = a.bias[NCH * k + c];
      s_node[q] = rec;
    } else {
      s_node[q] = d;
    }
  }
  __syncthreads();
  const int X = bx0 + (threadIdx.x & 63), Y = by0 + (threadIdx.x >> 6);
  if (X >= a.w || Y >= a.h) return;
  // this pixel's nodes: a part of the workgroup's, since bx0 <= X <= bx0 + 63 and by0 <= Y <= by0 + kWaves - 1
  const int li0 = dz_first(X - a.hi - half, step), li1 = dz_last(X + a.lo - half, step, a.g.nx);
  const int lj0 = dz_first(Y - a.hi - half, step), lj1 = dz_last(Y + a.lo - half, step, a.g.ny);
  float av[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) av[c] = a.A[c][(size_t)Y * a.sa + X];
  float su = 0.0f, sv = 0.0f, sw = 0.0f;
  float2 d0 = make_float2(0.0f, 0.0f);  // the first vote's displacement
  int n = 0;
  for (int j = lj0; j <= lj1; ++j) {
    const DzRec<BIAS, NCH> *row = s_node + (j - j0) * ncx - i0;
    for (int i = li0; i <= li1; ++i) {
      const DzRec<BIAS, NCH> d = row[i];
      const float px = (float)X + d.x, py = (float)Y + d.y;
      if (!fr_inside(px, py, a.w, a.h)) continue;  // a lost node (NaN) too
      float r[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        r[c] = fr_bilinear(a.B[c], a.sb, a.w, a.h, px, py) - av[c];
        if constexpr (BIAS) r[c] = r[c] - d.beta[c];
      }
      float e;
      if constexpr (NCH == 1)
        e = fabsf(r[0]);
      else
        e = ((fabsf(r[0]) + fabsf(r[1])) + fabsf(r[2])) / 3.0f;
      const float m = fmaxf(e, a.minerr);
      const float m2 = m * m;
      const float mp = a.power == 1 ? m : a.power == 2 ? m2 : a.power == 3 ? m2 * m : m2 * m2;
      const float wgt = 1.0f / mp;
      if (n == 0) d0 = make_float2(d.x, d.y);
      su = su + wgt * (d.x - d0.x);
      sv = sv + wgt * (d.y - d0.y);
      sw = sw + wgt;
      ++n;
    }
  }
  float u, v;
  if (n > 0) {
    u = d0.x + su / sw;
    v = d0.y + sv / sw;
  } else {
    fg_value(a.g, X, Y, &u, &v);
  }
  const size_t o = (size_t)Y * a.w + X;
  a.out[o] = make_float2(u, v);
  a.cnt[o] = (float)n;
  a.sw[o] = sw;
}
// 1 .. kSetMax densifiers of one geometry at once (DESIGN.md §4 "Lockstep sets"; a single densifier is a set of one): a
// member's workgroups along x and y, the members along z. One count of dynamic LDS serves them all.
template <bool BIAS, int NCH>
__global__ __launch_bounds__(kBlock) void k_densify(SetArgs<DzArgsT<NCH>> s) {
  static_assert(sizeof(s) <= kKernargLimit, "the argument block of a set exceeds the kernel-argument limit");
  dz_body<BIAS, NCH>(s.m[blockIdx.z]);
}

}  // namespace ictr

using namespace ictr;

// ---------------------------------------------------------------- C-ABI
struct ictr_flowdensify {
  int w = 0, h = 0;
  float minerr = 2.0f;
  int power = 1;
  int timing = 0, timed = 0;
  float *cnt = nullptr, *sw = nullptr;  // [h][w], [h][w]
  DevBuf<float> arena;                  // the result [h][w][2], then the two above
  Event ev0, ev1;                       // around the launch when timing is on
  DenseResult res;                      // last: its destructor waits for a run in flight
};

extern "C" void ictr_flowdensify_destroy(ictr_flowdensify *z) { delete z; }
extern "C" int ictr_flowdensify_create(ictr_flowdensify **out, int w, int h) {
  if (!out || w < 2 || h < 2 || w > 32768 || h > 32768)  // (the warp needs two taps each way; pixel indices are int)
    return fail(ICTR_ERR_INVALID, "flowdensify: bad arguments (2 <= w, h <= 32768)");
  if (int rc = need_device()) return rc;
  auto z = std::make_unique<ictr_flowdensify>();
  z->w = w;
  z->h = h;
  const size_t n = (size_t)w * h;
  if (int rc = z->arena.alloc(sizeof(float) * 4 * n, true)) return rc;
  z->cnt = z->arena.get() + 2 * n;
  z->sw = z->cnt + n;
  if (int rc = z->res.bind(z->arena.get(), w, h)) return rc;
  if (int rc = z->ev0.create()) return rc;
  if (int rc = z->ev1.create()) return rc;
  *out = z.release();
  return ICTR_OK;
}
extern "C" int ictr_flowdensify_set_params(ictr_flowdensify *z, float minerr, int power) {
  if (!z) return fail(ICTR_ERR_INVALID, "flowdensify is NULL");
  if (!isfinite(minerr) || !(minerr > 0.0f) || power < 1 || power > 4)
    return fail(ICTR_ERR_INVALID, "flowdensify_set_params: finite minerr > 0, 1 <= power <= 4");
  z->minerr = minerr;
  z->power = power;
  return ICTR_OK;
}
extern "C" int ictr_flowdensify_set_timing(ictr_flowdensify *z, int on) {
  if (!z) return fail(ICTR_ERR_INVALID, "flowdensify is NULL");
  z->timing = on ? 1 : 0;
  return ICTR_OK;
}

// the checks of a run (below), its kernel arguments and its bytes of LDS
template <int NCH>
static int dz_args(ictr_flowdensify *z, const ictr_flowgrid *grid, const ictr_pyramid *const *pyr_a,
                   const ictr_pyramid *const *pyr_b, int psz, int level, const float *bias, DzArgsT<NCH> *out, size_t *out_lds) {
  if (!z) return fail(ICTR_ERR_INVALID, "flowdensify is NULL");
  if (psz < 1 || psz > kDzMaxPsz) return fail(ICTR_ERR_INVALID, "flowdensify_run: psz is %d (1 .. %d)", psz, kDzMaxPsz);
  DzArgsT<NCH> &a = *out;
  memset(&a, 0, sizeof(a));
  if (int rc = ictr_flowgrid_view_lost_(grid, &a.g, &a.lost)) return rc;
  if (a.g.w != z->w || a.g.h != z->h)
    return fail(ICTR_ERR_INVALID, "flowdensify_run: the flow grid is %d x %d, the object %d x %d", a.g.w, a.g.h, z->w, z->h);
  for (int c = 0; c < NCH; ++c) {
    ictr_level0 l[2];
    for (int k = 0; k < 2; ++k) {
      if (int rc = ictr_pyramid_level0(k ? pyr_b[c] : pyr_a[c], "flowdensify_run", &l[k], level)) return rc;
      if (l[k].w != z->w || l[k].h != z->h)
        return fail(ICTR_ERR_INVALID, "flowdensify_run: a pyramid is %d x %d, the object %d x %d", l[k].w, l[k].h, z->w, z->h);
    }
    if (c > 0 && (l[0].stride != a.sa || l[1].stride != a.sb))
      return fail(ICTR_ERR_INVALID, "flowdensify_run: the channels' planes differ in stride");
    a.A[c] = l[0].img, a.sa = l[0].stride;
    a.B[c] = l[1].img, a.sb = l[1].stride;
  }
  a.w = z->w;
  a.h = z->h;
  a.lo = psz - psz / 2;
  a.hi = psz / 2 - 1;
  a.minerr = z->minerr;
  a.power = z->power;
  a.out = reinterpret_cast<float2 *>(z->res.get());
  a.cnt = z->cnt;
  a.sw = z->sw;
  a.bias = bias;
  const size_t lds = (bias ? sizeof(DzRec<true, NCH>) : sizeof(DzRec<false, NCH>)) *
                     (size_t)dz_capacity(64, psz, a.g.step) * dz_capacity(kWaves, psz, a.g.step);
  if (lds > kDzMaxLds)
    return fail(ICTR_ERR_INVALID, "flowdensify_run: step %d with psz %d needs a node table of %zu bytes of LDS (limit %zu)",
                a.g.step, psz, lds, kDzMaxLds);
  *out_lds = lds;
  return ICTR_OK;
}
// n densifiers of one size on level `level` of NCH pyramids per member and frame (grids and objects of that level's
// size), one launch: member m reads grid[m], the node bias bias[m] [ny][nx][NCH] on the device (all NULL: none,
// k_densify<false, NCH>) and the pyramids pyr_a[m * NCH + c], pyr_b[m * NCH + c]. Untimed, and no member's own event is
// recorded: that is the caller's to do behind the run.
template <int NCH>
static int dz_run(ictr_flowdensify *const *z, const ictr_flowgrid *const *grid, const ictr_pyramid *const *pyr_a,
                  const ictr_pyramid *const *pyr_b, int n, int psz, int level, const float *const *bias, hipStream_t s) {
  SetArgs<DzArgsT<NCH>> a;
  memset(&a, 0, sizeof(a));
  size_t lds = 0;
  for (int m = 0; m < n; ++m) {
    size_t l = 0;
    if (int rc = dz_args<NCH>(z[m], grid[m], pyr_a + m * NCH, pyr_b + m * NCH, psz, level, bias[m], &a.m[m], &l)) return rc;
    if (m > 0 && (l != lds || z[m]->w != z[0]->w || z[m]->h != z[0]->h || !bias[m] != !bias[0]))
      return fail(ICTR_ERR_INVALID, "flowdensify_run: member %d differs in geometry", m);
    lds = l;
  }
  dim3 g = pixel_rows_grid(z[0]->w, z[0]->h);
  g.z = n;
  if (bias[0])
    hipLaunchKernelGGL((k_densify<true, NCH>), g, dim3(kBlock), lds, s, a);
  else
    hipLaunchKernelGGL((k_densify<false, NCH>), g, dim3(kBlock), lds, s, a);
  HIPCHK(hipGetLastError());
  for (int m = 0; m < n; ++m) z[m]->timed = 0;
  return ICTR_OK;
}
// the coarse-to-fine flow's run (ictr_launch.h): `channels` (1 or 3, the caller's to keep) pyramids per member and frame
extern "C" int ictr_flowdensify_run_level_(ictr_flowdensify *const *z, const ictr_flowgrid *const *grid,
                                           const ictr_pyramid *const *pyr_a, const ictr_pyramid *const *pyr_b, int n,
                                           int channels, int psz, int level, const float *const *bias, void *hip_stream) {
  if (!z || !grid || !pyr_a || !pyr_b || !bias || n < 1 || n > kSetMax)
    return fail(ICTR_ERR_INVALID, "flowdensify_run: bad arguments");
  return channels == 3 ? dz_run<3>(z, grid, pyr_a, pyr_b, n, psz, level, bias, (hipStream_t)hip_stream)
                       : dz_run<1>(z, grid, pyr_a, pyr_b, n, psz, level, bias, (hipStream_t)hip_stream);
}
// a densifier's own run: a set of one at level 0 without bias, with its timing events around it and its result event behind
extern "C" int ictr_flowdensify_run(ictr_flowdensify *z, const ictr_flowgrid *grid, const ictr_pyramid *pyr_a,
                                    const ictr_pyramid *pyr_b, int psz, void *hip_stream) {
  if (!z) return fail(ICTR_ERR_INVALID, "flowdensify is NULL");
  hipStream_t s = (hipStream_t)hip_stream;
  const int timed = z->timing;
  const float *bias = nullptr;
  if (timed) HIPCHK(hipEventRecord(z->ev0.get(), s));
  if (int rc = ictr_flowdensify_run_level_(&z, &grid, &pyr_a, &pyr_b, 1, 1, psz, 0, &bias, s)) return rc;
  if (timed) HIPCHK(hipEventRecord(z->ev1.get(), s));
  z->timed = timed;
  return z->res.record(s);
}

// the parameters a set compares its members' densifiers by
extern "C" int ictr_flowdensify_get_params_(const ictr_flowdensify *z, float *minerr, int *power) {
  if (!z || !minerr || !power) return fail(ICTR_ERR_INVALID, "flowdensify is NULL");
  *minerr = z->minerr;
  *power = z->power;
  return ICTR_OK;
}

extern "C" int ictr_flowdensify_result(ictr_flowdensify *z, float *out, int on_device) {
  if (!z) return fail(ICTR_ERR_INVALID, "flowdensify is NULL");
  return z->res.copy_out("flowdensify_result", out, on_device);
}
extern "C" const float *ictr_flowdensify_device_ptr(const ictr_flowdensify *z) { return z ? z->res.get() : nullptr; }
extern "C" int ictr_flowdensify_get_kernel_ms(ictr_flowdensify *z, float *ms) {
  if (!z) return fail(ICTR_ERR_INVALID, "flowdensify is NULL");
  if (int rc = z->res.wait("flowdensify_get_kernel_ms")) return rc;
  if (!ms) return fail(ICTR_ERR_INVALID, "flowdensify_get_kernel_ms: ms is NULL");
  *ms = 0.0f;
  if (z->timed) HIPCHK(hipEventElapsedTime(ms, z->ev0.get(), z->ev1.get()));
  return ICTR_OK;
}
extern "C" int ictr_flowdensify_read_stage(ictr_flowdensify *z, int which, float *out) {
  if (!out || which < 0 || which >= ICTR_FLOWDENSIFY_STAGES)
    return fail(ICTR_ERR_INVALID, "flowdensify_read_stage: bad arguments (which is 0..%d)", ICTR_FLOWDENSIFY_STAGES - 1);
  if (!z) return fail(ICTR_ERR_INVALID, "flowdensify is NULL");
  if (int rc = z->res.wait("flowdensify_read_stage")) return rc;
  HIPCHK(hipMemcpy(out, which == 0 ? z->cnt : z->sw, sizeof(float) * (size_t)z->w * z->h, hipMemcpyDeviceToHost));
  return ICTR_OK;
}
