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
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "ictr_dev.h"
#include "ictr_launch.h"
#include "ictr_devfn.h"
#include "ictr_patchflow_dev.h"

namespace ictr {

// The search at one level (template, H sums, conditioning, iterations, the two-wave exchange) is pf_level_search of
// ictr_patchflow_dev.h, for both kernels here. A kernel keeps the point, the walk down the pyramid with the doubling
// and the level-entry view test, and the write-back. With two waves per patch (WPP = 2) every patch of a workgroup
// runs every level: a patch that is lost only stops updating.
template <int NPL, int WPP, bool XONLY>
__device__ __forceinline__ void pf_track(const PFArgs &a) {
  constexpr int PPB = kWaves / WPP;  // patches per workgroup
  __shared__ float sSum[WPP > 1 ? kWaves : 1][4];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int k = blockIdx.x * PPB + wave / WPP;
  const bool valid = k < a.K;
  if (WPP == 1 && !valid) return;
  const int kk = valid ? k : 0;
  const float x0 = a.pts[kk], y0 = a.pts[kk + a.K];
  float px = 0.0f, py = 0.0f;
  bool ok = valid & (x0 == x0) & (y0 == y0);
  int nit = 0;
  for (int l = a.lv_f; l >= a.lv_l && (WPP > 1 || ok); --l) {
    const PFLevel &lv = a.lv[l];
    const PFPlanes L{(gconst_f32)lv.a, (gconst_f32)lv.ax, (gconst_f32)lv.ay, (gconst_f32)lv.b,
                     lv.sw, lv.shift, lv.swo, lv.sho};
    if (l != a.lv_f) {
      px *= 2.0f;
      py *= 2.0f;
    }
    const float xl = x0 * lv.scale, yl = y0 * lv.scale;
    if (ok && !pf_in_view(xl, yl, L.swo, L.sho)) ok = false;
    if (WPP == 1 && !ok) break;
    const float min_cond = XONLY ? a.min_hx : a.min_det;
    float mean_t;  // (only patch-mean normalisation writes it; these kernels have none)
    if (pf_level_search<NPL, WPP, XONLY, false>(L, a.P, xl, yl, ok, px, py, nit, a.maxiter, a.eps2, min_cond, sSum, mean_t))
      ok = false;
  }
  if (lane == 0 && wave % WPP == 0 && valid) {
    const float s = 1.0f / a.lv[a.lv_l].scale;  // back to level-0 pixels
    const float nanv = __int_as_float(0x7fc00000);
    a.out[k] = ok ? x0 + px * s : nanv;
    a.out[k + a.K] = !ok ? nanv : XONLY ? y0 : y0 + py * s;  // (1-D: the input's bits)
    a.status[k] = ok ? 1 : 0;
    a.iters[k] = nit;
  }
}

template <int NPL, int WPP>
__global__ __launch_bounds__(kBlock) void k_patchflow(PFArgs a) {
  pf_track<NPL, WPP, false>(a);
}

static thread_local int g_pf_form = 0;
int patchflow_last_form() { return g_pf_form; }

void launch_patchflow(const PFArgs &a, hipStream_t s) {
  const int n = a.P * a.P;
  const int npl = (n + 63) / 64;
  const dim3 blk(kBlock);
  // few large patches: two waves per patch (see pf_patch_sum); ICTR_PF_WPP=1 keeps one wave per patch (A/B)
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
// The same patches, pyramid walk and stopping rule with ONE parameter: p moves along x, y never moves (pf_level_search's
// XONLY rule). Forms and the two-wave exchange are k_patchflow's.
template <int NPL, int WPP>
__global__ __launch_bounds__(kBlock) void k_patchdisp(PFArgs a) {
  pf_track<NPL, WPP, true>(a);
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
