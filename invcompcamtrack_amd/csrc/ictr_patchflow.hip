// ictr_patchflow.hip -- per-patch translation inverse-compositional Lucas-Kanade ("point tracker").
//
// Role (BASELINE config 4): the reference's misc_src/run_*OF* drivers obtain their
// displacement fields from an EXTERNAL optical-flow binary (run_OF_RGB / run_DE_RGB of the author's OF_DIS repo,
// misc_src/run_test_OF_track.py:90-108) that is not part of the repository. This kernel is the in-tree
// producer that replaces it: K independent P x P patches, each with its own 2-parameter translation, pyramidal,
// same Gauss-Newton skeleton as the camera tracker with J = identity:
//     H = sum [Gx Gy]^T [Gx Gy] over the template patch (once per level),
//     b = sum [Gx Gy]^T (T - I(x + p)),   p += H^-1 b.
// Sampling convention = util_getPatch's (utilities.cpp:55-113: patch-constant bilinear weights from x - floor(x),
// offsets -(P - P/2)...) except for the first tap: util_getPatch takes it at ceil(x + 1e-5f), this kernel at
// floor(x) + 1. The two agree wherever x + 1e-5f is not rounded across an integer; they differ at integer x >= 256
// (the sum rounds back to x: taps (x-1, x) with all the weight on x-1, the patch one pixel left or up) and at the f32
// value one ulp below an integer n <= 64 (ceil gives n + 1 against floor's n - 1: the weight lands one pixel right or
// down). floor(x) + 1 is the pair the weights are taken for at every x. The algorithm itself is build-defined: there is
// no reference implementation to pin it ("parity unpinned by the reference"); the oracle is oracle/np_patchflow.py.
//
// MI355X mapping: one wave64 per patch does ALL levels and ALL iterations of its patch inside one launch (the
// problems are independent: no global reduction, no launch per iteration). The template T/Gx/Gy of the patch lives
// in registers (<= 16 pixels per lane => P <= 32), H and b are wave shuffle reductions, every lane solves the 2x2.
//
// r02: an iteration is a latency chain per wave (4096 patches = 4096 waves = one round of four per SIMD), so what
// counts is how few dependent steps it has: the four taps of a pixel are TWO 8-byte loads ((x-1,x) at y and at y-1),
// every lane's loads of an iteration are issued before the first is consumed (pixels beyond the patch read the patch's
// first pixel and carry zero templates: no branch in the loop), and the wave sums use DPP (11 instructions) instead of
// six dependent ds_bpermute round trips each. Same expressions in the same order per pixel: same values.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "ictr_dev.h"
#include "ictr_launch.h"
#include "ictr_devfn.h"
#include "ictr_patchflow_dev.h"

namespace ictr {

// pf_taps, pf_load, pf_blend, pf_fetch, pf_in_view, pf_wave_sum: ictr_patchflow_dev.h

// WPP waves share a patch (pixels per lane NPL = ceil(P*P / (64 WPP))). One wave per patch needs no synchronisation at
// all; for large patches (more than 4 pixels per lane) TWO waves per patch halve each wave's chain of pixels and double
// the waves that hide each other's loads (+2 % at 4096 patches of 31x31, +9 % at 65536): the wave sums then meet in LDS (partials of the two waves added in wave order by
// both: the same bits in both), one workgroup barrier per reduction. Barriers need a uniform loop structure: every
// patch of a workgroup runs every level and iteration slot; a patch that is lost or converged only stops updating.
template <int NPL, int WPP>
__global__ __launch_bounds__(kBlock) void k_patchflow(PFArgs a) {
  constexpr int PPB = kWaves / WPP;  // patches per workgroup
  __shared__ float sSum[WPP > 1 ? kWaves : 1][4];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wsub = wave % WPP;
  const int k = blockIdx.x * PPB + wave / WPP;
  const bool valid = k < a.K;
  if (WPP == 1 && !valid) return;
  const int P = a.P, n = P * P;
  const int kk = valid ? k : 0;
  const float x0 = a.pts[kk], y0 = a.pts[kk + a.K];
  float px = 0.0f, py = 0.0f;
  bool ok = valid & (x0 == x0) & (y0 == y0);
  int nit = 0;
  int off[NPL];
#pragma unroll
  for (int i = 0; i < NPL; ++i) off[i] = 0;
  // sum over the patch's WPP waves of three / two per-wave totals (all waves of the patch get the same bits)
  auto patch_sum3 = [&](float &u, float &v, float &w) {
    u = pf_wave_sum(u);
    v = pf_wave_sum(v);
    w = pf_wave_sum(w);
    if constexpr (WPP > 1) {
      __syncthreads();  // (the previous reduction's partials have been read)
      if (lane == 0) {
        sSum[wave][0] = u;
        sSum[wave][1] = v;
        sSum[wave][2] = w;
      }
      __syncthreads();
      const int w0 = wave - wsub;
      u = v = w = 0.0f;
#pragma unroll
      for (int q = 0; q < WPP; ++q) {
        u += sSum[w0 + q][0];
        v += sSum[w0 + q][1];
        w += sSum[w0 + q][2];
      }
    }
  };

  for (int l = a.lv_f; l >= a.lv_l && (WPP > 1 || ok); --l) {
    const PFLevel L = a.lv[l];
    if (l != a.lv_f) {
      px *= 2.0f;
      py *= 2.0f;
    }
    const float xl = x0 * L.scale, yl = y0 * L.scale;
    if (ok && !pf_in_view(xl, yl, L.swo, L.sho)) ok = false;
    if (WPP == 1 && !ok) break;
    const PFTaps ta = pf_taps(ok ? xl : 1.0f, ok ? yl : 1.0f, P, L.sw, L.shift);  // (1,1): a harmless in-plane window
    gconst_f32 pa = (gconst_f32)L.a, pax = (gconst_f32)L.ax, pay = (gconst_f32)L.ay, pb = (gconst_f32)L.b;
    float T[NPL], Gx[NPL], Gy[NPL];
    float hxx = 0.0f, hxy = 0.0f, hyy = 0.0f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      const int q = wsub * 64 + lane + 64 * WPP * i;
      const bool in = q < n;
      off[i] = in ? (q / P) * L.sw + (q % P) : 0;  // beyond the patch: its first pixel, with zero templates
      const int idx = ta.base + off[i];
      const float t = pf_fetch(pa, idx, L.sw, ta), gx = pf_fetch(pax, idx, L.sw, ta), gy = pf_fetch(pay, idx, L.sw, ta);
      T[i] = in ? t : 0.0f;
      Gx[i] = in ? gx : 0.0f;
      Gy[i] = in ? gy : 0.0f;
      hxx += Gx[i] * Gx[i];
      hxy += Gx[i] * Gy[i];
      hyy += Gy[i] * Gy[i];
    }
    patch_sum3(hxx, hxy, hyy);
    const float det = hxx * hyy - hxy * hxy;
    const float tr = hxx + hyy;
    if (ok && (!(det > a.min_det * tr * tr) || !(tr > 0.0f))) ok = false;  // textureless or 1-D structure
    if (WPP == 1 && !ok) break;
    const float idet = 1.0f / det;
    bool run = ok;  // this patch still iterates at this level
    for (int it = 0; it < a.maxiter; ++it) {
      if (WPP == 1 && !run) break;
      const float cx = xl + px, cy = yl + py;
      if (run && !pf_in_view(cx, cy, L.swo, L.sho)) {
        ok = false;
        run = false;
        if (WPP == 1) break;
      }
      const PFTaps tb = pf_taps(run ? cx : 1.0f, run ? cy : 1.0f, P, L.sw, L.shift);
      float bx = 0.0f, by = 0.0f, dummy = 0.0f;
      PFWin w[NPL];
#pragma unroll
      for (int i = 0; i < NPL; ++i) w[i] = pf_load(pb, tb.base + off[i], L.sw);  // all in flight before the first use
#pragma unroll
      for (int i = 0; i < NPL; ++i) {
        float r = T[i] - pf_blend(w[i], tb);
        r = (wsub * 64 + lane + 64 * WPP * i < n) ? r : 0.0f;  // (T = 0 there, but the frame value is not)
        bx += Gx[i] * r;
        by += Gy[i] * r;
      }
      patch_sum3(bx, by, dummy);
      if (run) {
        const float dx = (hyy * bx - hxy * by) * idet;
        const float dy = (hxx * by - hxy * bx) * idet;
        px += dx;
        py += dy;
        ++nit;
        if (dx * dx + dy * dy < a.eps2) run = false;
      }
    }
  }
  if (lane == 0 && wsub == 0 && valid) {
    const float s = 1.0f / a.lv[a.lv_l].scale;  // back to level-0 pixels
    const float nanv = __int_as_float(0x7fc00000);
    a.out[k] = ok ? x0 + px * s : nanv;
    a.out[k + a.K] = ok ? y0 + py * s : nanv;
    a.status[k] = ok ? 1 : 0;
    a.iters[k] = nit;
  }
}

static thread_local int g_pf_form = 0;
int patchflow_last_form() { return g_pf_form; }

void launch_patchflow(const PFArgs &a, hipStream_t s) {
  const int n = a.P * a.P;
  const int npl = (n + 63) / 64;
  const dim3 blk(kBlock);
  // few large patches: two waves per patch (see k_patchflow); ICTR_PF_WPP=1 keeps one wave per patch (A/B)
  static const int wpp_env = [] {
    const char *e = getenv("ICTR_PF_WPP");
    return e ? atoi(e) : 0;
  }();
  // measured (31x31 patches, 3 levels x 10 iterations): 4096 patches 168 against 173 us, 65536 patches 2.74 against 2.99 ms
  const bool two = wpp_env ? wpp_env == 2 : npl > 4;
  if (two) {
    const dim3 g((a.K + kWaves / 2 - 1) / (kWaves / 2));
    g_pf_form = 82;
    hipLaunchKernelGGL((k_patchflow<8, 2>), g, blk, 0, s, a);
    return;
  }
  const dim3 g((a.K + kWaves - 1) / kWaves);
  g_pf_form = npl <= 1 ? 11 : npl <= 4 ? 41 : 161;
  if (npl <= 1)
    hipLaunchKernelGGL((k_patchflow<1, 1>), g, blk, 0, s, a);
  else if (npl <= 4)
    hipLaunchKernelGGL((k_patchflow<4, 1>), g, blk, 0, s, a);
  else
    hipLaunchKernelGGL((k_patchflow<16, 1>), g, blk, 0, s, a);
}

// ---------------------------------------------------------------- 1-D (x only) search for a rectified stereo pair
// The same patches, pyramid walk and stopping rule as k_patchflow with ONE parameter: p moves along x, y never moves.
//     hxx = sum Gx^2 (once per level),  bx = sum Gx (T - I(x + p, y)),  p += bx * (1 / hxx).
// Conditioning: the patch is lost iff !(tr > 0) or !(hxx > min_hx * tr), tr = hxx + hyy: horizontal edges alone carry
// no disparity, vertical edges alone (which the 2x2 system refuses) are kept. Gy lives only until hyy is summed; T and
// Gx stay in registers; one wave sum per iteration sits on the chain. Forms and the two-wave exchange are
// k_patchflow's (above): every patch of a two-wave workgroup runs every level and iteration slot.
template <int NPL, int WPP>
__global__ __launch_bounds__(kBlock) void k_patchdisp(PFArgs a) {
  constexpr int PPB = kWaves / WPP;  // patches per workgroup
  __shared__ float sSum[WPP > 1 ? kWaves : 1][2];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wsub = wave % WPP;
  const int k = blockIdx.x * PPB + wave / WPP;
  const bool valid = k < a.K;
  if (WPP == 1 && !valid) return;
  const int P = a.P, n = P * P;
  const int kk = valid ? k : 0;
  const float x0 = a.pts[kk], y0 = a.pts[kk + a.K];
  float px = 0.0f;
  bool ok = valid & (x0 == x0) & (y0 == y0);
  int nit = 0;
  int off[NPL];
#pragma unroll
  for (int i = 0; i < NPL; ++i) off[i] = 0;
  // sum over the patch's WPP waves of two / one per-wave totals (all waves of the patch get the same bits)
  auto patch_sum2 = [&](float &u, float &v) {
    u = pf_wave_sum(u);
    v = pf_wave_sum(v);
    if constexpr (WPP > 1) {
      __syncthreads();  // (the previous reduction's partials have been read)
      if (lane == 0) {
        sSum[wave][0] = u;
        sSum[wave][1] = v;
      }
      __syncthreads();
      const int w0 = wave - wsub;
      u = v = 0.0f;
#pragma unroll
      for (int q = 0; q < WPP; ++q) {
        u += sSum[w0 + q][0];
        v += sSum[w0 + q][1];
      }
    }
  };
  auto patch_sum1 = [&](float &u) {
    u = pf_wave_sum(u);
    if constexpr (WPP > 1) {
      __syncthreads();
      if (lane == 0) sSum[wave][0] = u;
      __syncthreads();
      const int w0 = wave - wsub;
      u = 0.0f;
#pragma unroll
      for (int q = 0; q < WPP; ++q) u += sSum[w0 + q][0];
    }
  };

  for (int l = a.lv_f; l >= a.lv_l && (WPP > 1 || ok); --l) {
    const PFLevel L = a.lv[l];
    if (l != a.lv_f) px *= 2.0f;
    const float xl = x0 * L.scale, yl = y0 * L.scale;
    if (ok && !pf_in_view(xl, yl, L.swo, L.sho)) ok = false;
    if (WPP == 1 && !ok) break;
    const PFTaps ta = pf_taps(ok ? xl : 1.0f, ok ? yl : 1.0f, P, L.sw, L.shift);  // (1,1): a harmless in-plane window
    gconst_f32 pa = (gconst_f32)L.a, pax = (gconst_f32)L.ax, pay = (gconst_f32)L.ay, pb = (gconst_f32)L.b;
    float T[NPL], Gx[NPL];
    float hxx = 0.0f, hyy = 0.0f;
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      const int q = wsub * 64 + lane + 64 * WPP * i;
      const bool in = q < n;
      off[i] = in ? (q / P) * L.sw + (q % P) : 0;  // beyond the patch: its first pixel, with zero templates
      const int idx = ta.base + off[i];
      const float t = pf_fetch(pa, idx, L.sw, ta), gx = pf_fetch(pax, idx, L.sw, ta), gy = pf_fetch(pay, idx, L.sw, ta);
      T[i] = in ? t : 0.0f;
      Gx[i] = in ? gx : 0.0f;
      const float gyi = in ? gy : 0.0f;
      hxx += Gx[i] * Gx[i];
      hyy += gyi * gyi;
    }
    patch_sum2(hxx, hyy);
    const float tr = hxx + hyy;
    if (ok && (!(tr > 0.0f) || !(hxx > a.min_hx * tr))) ok = false;  // textureless, or horizontal edges alone
    if (WPP == 1 && !ok) break;
    const float ihx = 1.0f / hxx;
    bool run = ok;  // this patch still iterates at this level
    for (int it = 0; it < a.maxiter; ++it) {
      if (WPP == 1 && !run) break;
      const float cx = xl + px;
      if (run && !pf_in_view(cx, yl, L.swo, L.sho)) {
        ok = false;
        run = false;
        if (WPP == 1) break;
      }
      const PFTaps tb = pf_taps(run ? cx : 1.0f, run ? yl : 1.0f, P, L.sw, L.shift);
      float bx = 0.0f;
      PFWin w[NPL];
#pragma unroll
      for (int i = 0; i < NPL; ++i) w[i] = pf_load(pb, tb.base + off[i], L.sw);  // all in flight before the first use
#pragma unroll
      for (int i = 0; i < NPL; ++i) {
        float r = T[i] - pf_blend(w[i], tb);
        r = (wsub * 64 + lane + 64 * WPP * i < n) ? r : 0.0f;  // (T = 0 there, but the frame value is not)
        bx += Gx[i] * r;
      }
      patch_sum1(bx);
      if (run) {
        const float dx = bx * ihx;
        px += dx;
        ++nit;
        if (dx * dx < a.eps2) run = false;
      }
    }
  }
  if (lane == 0 && wsub == 0 && valid) {
    const float s = 1.0f / a.lv[a.lv_l].scale;  // back to level-0 pixels
    const float nanv = __int_as_float(0x7fc00000);
    a.out[k] = ok ? x0 + px * s : nanv;
    a.out[k + a.K] = ok ? y0 : nanv;  // the input's bits
    a.status[k] = ok ? 1 : 0;
    a.iters[k] = nit;
  }
}

static thread_local int g_pd_form = 0;
int patchdisp_last_form() { return g_pd_form; }

// the form follows from the patch size alone: up to 4 pixels per lane one wave per patch, above that two
void launch_patchdisp(const PFArgs &a, hipStream_t s) {
  const int npl = (a.P * a.P + 63) / 64;
  const dim3 blk(kBlock);
  if (npl > 4) {
    g_pd_form = 82;
    hipLaunchKernelGGL((k_patchdisp<8, 2>), dim3((a.K + kWaves / 2 - 1) / (kWaves / 2)), blk, 0, s, a);
    return;
  }
  const dim3 g((a.K + kWaves - 1) / kWaves);
  g_pd_form = npl <= 1 ? 11 : 41;
  if (npl <= 1)
    hipLaunchKernelGGL((k_patchdisp<1, 1>), g, blk, 0, s, a);
  else
    hipLaunchKernelGGL((k_patchdisp<4, 1>), g, blk, 0, s, a);
}

}  // namespace ictr

using namespace ictr;

// ---------------------------------------------------------------- C-ABI
static thread_local float g_pf_ms = -1.0f;
extern "C" float ictr_patchflow_last_kernel_ms(void) { return g_pf_ms; }
extern "C" int ictr_patchflow_last_form(void) { return patchflow_last_form(); }
// the argument checks of a patch tracking and the level table of its launch (a.pts / out / status / iters and a.K are the
// caller's): shared by ictr_patchflow and the flow grid of ictr_frontend.hip, so that both launch the same kernel on the
// same arguments
int ictr::patchflow_args(const ictr_pyramid *pyr_a, const ictr_pyramid *pyr_b, int psz, int lv_f, int lv_l, int maxiter,
                         float eps, PFArgs *out) {
  if (!pyr_a || !pyr_b || psz < 1 || psz > 32 || lv_l < 0 || lv_f < lv_l || maxiter < 0)
    return fail(ICTR_ERR_INVALID, "patchflow: bad arguments (psz must be 1..32)");
  ictr_pyramid_view pa, pb;
  ictr_pyramid_view_(pyr_a, &pa);
  ictr_pyramid_view_(pyr_b, &pb);
  if (lv_f >= pa.nlev || lv_f >= pb.nlev || lv_f > 15)
    return fail(ICTR_ERR_INVALID, "patchflow: pyramids have fewer than lv_f+1 levels");
  if (!pa.getgrad) return fail(ICTR_ERR_INVALID, "patchflow: the first pyramid needs gradient planes (getgrad = 1)");
  if (pa.pad < psz || pb.pad < psz) return fail(ICTR_ERR_INVALID, "patchflow: pyramid padding must be >= psz");
  for (int l = lv_l; l <= lv_f; ++l)
    if (pa.w[l] != pb.w[l] || pa.h[l] != pb.h[l] || pa.sw[l] != pb.sw[l])
      return fail(ICTR_ERR_INVALID, "patchflow: the two pyramids differ in size at level %d", l);
  PFArgs &a = *out;
  memset(&a, 0, sizeof(a));
  for (int l = lv_l; l <= lv_f; ++l) {
    a.lv[l].a = pa.img[l];
    a.lv[l].ax = pa.dx[l];
    a.lv[l].ay = pa.dy[l];
    a.lv[l].b = pb.img[l];
    a.lv[l].sw = pa.sw[l];
    a.lv[l].shift = (pa.pad - psz) * (pa.sw[l] + 1);
    a.lv[l].swo = (float)pa.w[l];
    a.lv[l].sho = (float)pa.h[l];
    a.lv[l].scale = (float)(1 / pow(2, l));
  }
  a.lv_f = lv_f;
  a.lv_l = lv_l;
  a.P = psz;
  a.maxiter = maxiter;
  a.eps2 = eps * eps;
  a.min_det = 1e-4f;
  a.min_hx = 1e-2f;
  return ICTR_OK;
}
// one tracking call from host arrays: the 2-D launch (ictr_patchflow) or the 1-D one (ictr_patchdisp), timed into *ms
static int pf_track_host(const ictr_pyramid *pa, const ictr_pyramid *pb, const float *pts, int64_t K, int psz, int lv_f,
                         int lv_l, int maxiter, float eps, float *out, int *status, int *iters,
                         void (*launch)(const PFArgs &, hipStream_t), float *ms) {
  if (K < 0 || (K > 0 && (!pts || !out))) return fail(ICTR_ERR_INVALID, "patchflow: bad arguments (psz must be 1..32)");
  PFArgs a;
  if (int rc = patchflow_args(pa, pb, psz, lv_f, lv_l, maxiter, eps, &a)) return rc;
  if (K == 0) return ICTR_OK;
  if (int rc = need_device()) return rc;
  a.K = (int)K;
  DevBuf<float> buf;  // pts [2 K] | out [2 K] | status [K] i32 | iters [K] i32
  if (int rc = buf.alloc(sizeof(float) * 6 * K)) return rc;
  float *d = buf.get();
  a.pts = d;
  a.out = d + 2 * K;
  a.status = reinterpret_cast<int *>(d + 4 * K);
  a.iters = reinterpret_cast<int *>(d + 5 * K);
  HIPCHK(hipMemcpy(d, pts, sizeof(float) * 2 * K, hipMemcpyHostToDevice));
  // duration of the one kernel, for callers that report it; the two events live as long as their thread
  static thread_local hipEvent_t ev0 = nullptr, ev1 = nullptr;
  if (!ev0 && (hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess)) ev0 = ev1 = nullptr;
  if (ev0) (void)hipEventRecord(ev0, nullptr);
  launch(a, nullptr);
  if (ev0) (void)hipEventRecord(ev1, nullptr);
  *ms = -1.0f;  // ... unless the launch and the first copy back succeed
  HIPCHK(hipMemcpy(out, a.out, sizeof(float) * 2 * K, hipMemcpyDeviceToHost));
  if (ev0 && hipEventElapsedTime(ms, ev0, ev1) != hipSuccess) *ms = -1.0f;
  if (status) HIPCHK(hipMemcpy(status, a.status, sizeof(int) * K, hipMemcpyDeviceToHost));
  if (iters) HIPCHK(hipMemcpy(iters, a.iters, sizeof(int) * K, hipMemcpyDeviceToHost));
  return ICTR_OK;
}
extern "C" int ictr_patchflow(const ictr_pyramid *pa, const ictr_pyramid *pb, const float *pts, int64_t K, int psz,
                              int lv_f, int lv_l, int maxiter, float eps, float *out, int *status, int *iters) {
  return pf_track_host(pa, pb, pts, K, psz, lv_f, lv_l, maxiter, eps, out, status, iters, launch_patchflow, &g_pf_ms);
}
static thread_local float g_pd_ms = -1.0f;
extern "C" float ictr_patchdisp_last_kernel_ms(void) { return g_pd_ms; }
extern "C" int ictr_patchdisp_last_form(void) { return patchdisp_last_form(); }
extern "C" int ictr_patchdisp(const ictr_pyramid *pa, const ictr_pyramid *pb, const float *pts, int64_t K, int psz,
                              int lv_f, int lv_l, int maxiter, float eps, float *out, int *status, int *iters) {
  return pf_track_host(pa, pb, pts, K, psz, lv_f, lv_l, maxiter, eps, out, status, iters, launch_patchdisp, &g_pd_ms);
}
