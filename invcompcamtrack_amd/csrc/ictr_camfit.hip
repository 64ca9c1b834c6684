// ictr_camfit.hip -- "Fit cameras" (misc_src/run_test_OF_track.py:374-411) on the device: one pose per frame of a track
// window by Levenberg-Marquardt on the reprojection error of the same N points, and the reprojection means that follow.
//
// A run is 2 + 2 noiter launches on one stream with no host wait in between: pass, step, then noiter times pass, step.
//
//   k_camfit_pass    grid (chunks of kCfChunk points, frames), kCfPerLane points per lane read once from the [3][N] and
//                    [F][2][N] planes: the 28 terms of cf_point summed lane-serially, by xor shuffles inside a wave and
//                    through LDS across the four waves; 28 partials and the count in one vector store per chunk and frame.
//   k_camfit_step    one workgroup per frame: one lane per term adds the chunk partials in chunk order, then one lane
//                    runs cf_step (accept test, damping, stops, solve, update). A frame that has stopped makes its later
//                    launches return at once.
//   k_camfit_reproj  the pass with cf_reproj_point as its only term.
//
// Every result is fixed-order f64 arithmetic (ictr_camfit_hd.h): the same bits on every run and every device.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <memory>
#include <vector>

#include "ictr_camfit_hd.h"
#include "ictr_dev.h"
#include "ictr_launch.h"
#include "ictr_wininputs.h"

namespace ictr {

constexpr int kCfStepBlock = 64;
constexpr int kCfMaxFrames = 4096;
constexpr int kCfMaxIter = 1000;

struct CamfitArgs {
  const double *X;                  // [3][n]
  const double *xy;                 // [F][2][n]
  const unsigned long long *words;  // [ceil(n / 64)] inlier bits, or NULL: every point
  int n, nchunks, sums_only;
  CfCam cam;
  CfParams prm;
  double dt[3];   // k_camfit_reproj
  double *part;   // [F][nchunks][kCfSlots]
  CfState *st;    // [F]
};

// one chunk of one frame at the frame's Gt: NT terms per observation
template <int NT, bool REPROJ>
__device__ __forceinline__ void cf_chunk(const CamfitArgs &a) {
  __shared__ double sW[kCfBlock / 64][NT];
  __shared__ int sC[kCfBlock / 64];
  const int f = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const CfState *st = a.st + f;
  if (!REPROJ && st->status != kCfRunning) return;
  double G[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) G[q] = st->Gt[q];
  const size_t n = (size_t)a.n;
  const double *xo = a.xy + (size_t)f * 2 * n;
  double acc[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) acc[q] = 0.0;
  int cnt = 0;
#pragma unroll
  for (int r = 0; r < kCfPerLane; ++r) {
    const size_t m = (size_t)ch * kCfChunk + (size_t)r * kCfBlock + tid;
    const bool in = m < n;
    const size_t mm = in ? m : n - 1;
    const double X = a.X[mm], Y = a.X[n + mm], Z = a.X[2 * n + mm], x = xo[mm], y = xo[n + mm];
    const bool bit = a.words ? ((a.words[mm >> 6] >> (mm & 63)) & 1ull) != 0 : true;
    const bool counted = in && cf_counted(bit, X, Y, Z, x, y);
    cnt += counted ? 1 : 0;
    if (REPROJ) {
      acc[0] = acc[0] + cf_reproj_point(G, a.dt, a.cam, X, Y, Z, x, y, counted);
    } else {
      double t[kCfTerms];
      cf_point(G, a.cam, X, Y, Z, x, y, counted, t);
#pragma unroll
      for (int q = 0; q < NT; ++q) acc[q] = acc[q] + t[q];
    }
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
#pragma unroll
    for (int q = 0; q < NT; ++q) acc[q] = acc[q] + __shfl_xor(acc[q], s, 64);
    cnt += __shfl_xor(cnt, s, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < NT; ++q) sW[wave][q] = acc[q];
    sC[wave] = cnt;
  }
  __syncthreads();
  if (tid < kCfSlots) {
    double v = 0.0;
    if (tid < NT) v = (sW[0][tid] + sW[1][tid]) + (sW[2][tid] + sW[3][tid]);
    if (tid == kCfCountSlot) v = (double)((sC[0] + sC[1]) + (sC[2] + sC[3]));
    a.part[((size_t)f * a.nchunks + ch) * kCfSlots + tid] = v;
  }
}

__global__ void __launch_bounds__(kCfBlock) k_camfit_pass(CamfitArgs a) { cf_chunk<kCfTerms, false>(a); }
__global__ void __launch_bounds__(kCfBlock) k_camfit_reproj(CamfitArgs a) { cf_chunk<1, true>(a); }

__global__ void __launch_bounds__(kCfStepBlock) k_camfit_step(CamfitArgs a) {
  __shared__ double sS[kCfSlots];
  const int f = blockIdx.x, t = threadIdx.x;
  CfState *st = a.st + f;
  if (!a.sums_only && st->status != kCfRunning) return;
  if (t < kCfSlots) {
    const double *p = a.part + (size_t)f * a.nchunks * kCfSlots + t;
    double acc = 0.0;
    for (int c = 0; c < a.nchunks; ++c) acc = acc + p[(size_t)c * kCfSlots];
    sS[t] = t < kCfTerms ? cf_canon(acc) : acc;
  }
  __syncthreads();
  if (a.sums_only) {
    if (t < kCfSlots) st->sums[t] = sS[t];
    return;
  }
  if (t == 0) {
    double sums[kCfSlots];
#pragma unroll
    for (int q = 0; q < kCfSlots; ++q) sums[q] = sS[q];
    cf_step(*st, sums, a.prm);
  }
}

static void launch_camfit_pass(const CamfitArgs &a, int nframes, hipStream_t s) {
  hipLaunchKernelGGL(k_camfit_pass, dim3(a.nchunks, nframes), dim3(kCfBlock), 0, s, a);
}
static void launch_camfit_reproj(const CamfitArgs &a, int nframes, hipStream_t s) {
  hipLaunchKernelGGL(k_camfit_reproj, dim3(a.nchunks, nframes), dim3(kCfBlock), 0, s, a);
}
static void launch_camfit_step(const CamfitArgs &a, int nframes, hipStream_t s) {
  hipLaunchKernelGGL(k_camfit_step, dim3(nframes), dim3(kCfStepBlock), 0, s, a);
}

}  // namespace ictr

using namespace ictr;

// ---------------------------------------------------------------- host side
struct ictr_camfit {
  WinInputs in;  // one side
  int nchunks = 0;
  DevBuf<double> d_part;
  PinBuf<char> up;  // the frames' initial states of a run, uploaded on its stream
  bool timing = false, timed = false;  // timed: the run in flight (or last waited) carries events
  std::vector<Event> tev;              // one before every launch and one after the last
  float ms[2] = {0, 0};
  // declared last, so destroyed first: a run in flight ends before a buffer or a timing event goes
  Readback out;  // CfState [nframes]
};

static size_t cf_bytes(const ictr_camfit *r) { return sizeof(CfState) * (size_t)r->in.nframes; }

extern "C" int ictr_camfit_create(ictr_camfit **out, int64_t n, int64_t nframes) {
  if (!out) return fail(ICTR_ERR_INVALID, "camfit_create: NULL argument");
  if (n < 1 || n > ((int64_t)1 << 22))
    return fail(ICTR_ERR_INVALID, "camfit_create: %lld points (1 .. 2^22)", (long long)n);
  if (nframes < 1 || nframes > kCfMaxFrames)
    return fail(ICTR_ERR_INVALID, "camfit_create: %lld frames (1 .. %d)", (long long)nframes, kCfMaxFrames);
  if (int rc = need_device()) return rc;
  auto r = std::make_unique<ictr_camfit>();
  r->nchunks = (int)((n + kCfChunk - 1) / kCfChunk);
  if (int rc = r->in.alloc((int)n, (int)nframes, 1)) return rc;
  if (int rc = r->d_part.alloc(sizeof(double) * kCfSlots * (size_t)nframes * (size_t)r->nchunks, true)) return rc;
  if (int rc = r->up.alloc(cf_bytes(r.get()))) return rc;
  if (int rc = r->out.reserve(cf_bytes(r.get()), true)) return rc;
  *out = r.release();
  return ICTR_OK;
}

extern "C" void ictr_camfit_destroy(ictr_camfit *r) { delete r; }

extern "C" int ictr_camfit_set_points(ictr_camfit *r, const double *X) {
  return r ? r->in.set_points("camfit_set_points", "camfit", r->out, X) : null_object("camfit_set_points");
}
extern "C" int ictr_camfit_set_observations(ictr_camfit *r, const double *xy) {
  return r ? r->in.set_observations("camfit_set_observations", "camfit", r->out, xy)
           : null_object("camfit_set_observations");
}
extern "C" int ictr_camfit_set_mask(ictr_camfit *r, const uint64_t *words) {
  return r ? r->in.set_mask("camfit_set_mask", "camfit", r->out, words) : fail(ICTR_ERR_INVALID, "camfit is NULL");
}
extern "C" int ictr_camfit_set_camera(ictr_camfit *r, const double *fc, const double *cc) {
  return r ? r->in.set_camera("camfit_set_camera", "camfit", r->out, fc, cc) : null_object("camfit_set_camera");
}

extern "C" int ictr_camfit_inputs_(ictr_camfit *r, WinDest *d) {
  *d = {&r->in, &r->out, "camfit", "fit"};
  return ICTR_OK;
}

extern "C" int ictr_camfit_set_timing(ictr_camfit *r, int on) {
  if (!r) return fail(ICTR_ERR_INVALID, "camfit is NULL");
  if (int rc = r->out.refuse("camfit_set_timing", "camfit")) return rc;
  r->timing = on != 0;
  return ICTR_OK;
}

static void cf_fill_args(const ictr_camfit *r, const CfParams &p, CamfitArgs &a) {
  memset(&a, 0, sizeof(a));
  a.X = r->in.X.get();
  a.xy = r->in.xy.get();
  a.words = r->in.mask_or_null();
  a.n = r->in.n;
  a.nchunks = r->nchunks;
  a.cam = r->in.cam;
  a.prm = p;
  a.part = r->d_part.get();
  a.st = reinterpret_cast<CfState *>(r->out.dev());
}

static int cf_poses_finite(const double *G, int nframes, const char *what) {
  for (int q = 0; q < 12 * nframes; ++q)
    if (!cf_finite(G[q])) return fail(ICTR_ERR_INVALID, "%s: a pose entry is not finite", what);
  return ICTR_OK;
}

extern "C" int ictr_camfit_run(ictr_camfit *r, const double *G0, int32_t noiter, double damp_init, double damp_fct,
                               double minres, double maxdamp, void *hip_stream) {
  if (!r || !G0) return fail(ICTR_ERR_INVALID, "camfit_run: NULL argument");
  if (int rc = r->in.ready("camfit_run", r->out, "camfit")) return rc;
  if (noiter < 0 || noiter > kCfMaxIter) return fail(ICTR_ERR_INVALID, "camfit_run: noiter %d (0 .. %d)", noiter, kCfMaxIter);
  if (!(damp_init > 0.0) || !cf_finite(damp_init) || !(damp_fct > 1.0) || !cf_finite(damp_fct) || !(minres >= 0.0) ||
      !cf_finite(minres) || !(maxdamp > 0.0))
    return fail(ICTR_ERR_INVALID, "camfit_run: needs damp_init > 0, damp_fct > 1, minres >= 0 (all finite), maxdamp > 0");
  if (int rc = cf_poses_finite(G0, r->in.nframes, "camfit_run")) return rc;
  const CfParams p = {noiter, damp_init, damp_fct, minres, maxdamp};
  CamfitArgs a;
  cf_fill_args(r, p, a);
  std::vector<Event> tev;
  if (r->timing) {
    tev.resize(3 + 2 * (size_t)noiter);
    for (Event &e : tev)
      if (int rc = e.create()) return rc;
  }
  CfState *init = reinterpret_cast<CfState *>(r->up.get());
  for (int f = 0; f < r->in.nframes; ++f) cf_init(init[f], G0 + 12 * f, p);
  hipStream_t s = (hipStream_t)hip_stream;
  HIPCHK(hipMemcpyAsync(r->out.dev(), r->up.get(), cf_bytes(r), hipMemcpyHostToDevice, s));
  size_t e = 0;
  for (int it = 0; it <= noiter; ++it) {
    if (r->timing) HIPCHK(hipEventRecord(tev[e++].get(), s));
    launch_camfit_pass(a, r->in.nframes, s);
    if (r->timing) HIPCHK(hipEventRecord(tev[e++].get(), s));
    launch_camfit_step(a, r->in.nframes, s);
    HIPCHK(hipGetLastError());
  }
  if (r->timing) HIPCHK(hipEventRecord(tev[e++].get(), s));
  if (int rc = r->out.post(cf_bytes(r), s)) return rc;
  r->tev = std::move(tev);
  r->timed = r->timing;
  return ICTR_OK;
}

extern "C" int ictr_camfit_wait(ictr_camfit *r, double *G, double *cost, double *damp, int32_t *iters, int32_t *status,
                                int64_t *n) {
  if (!r) return fail(ICTR_ERR_INVALID, "camfit is NULL");
  if (!r->out.pending()) return fail(ICTR_ERR_STATE, "camfit_wait: nothing has been run");
  if (int rc = r->out.wait()) return rc;
  const CfState *st = reinterpret_cast<const CfState *>(r->out.host());
  for (int f = 0; f < r->in.nframes; ++f) {
    if (G) memcpy(G + 12 * f, st[f].G, sizeof(st[f].G));
    if (cost) cost[f] = st[f].c;
    if (damp) damp[f] = st[f].damp;
    if (iters) iters[f] = st[f].it;
    if (status) status[f] = st[f].status;
    if (n) n[f] = st[f].n;
  }
  if (r->timed) {
    float ms[2] = {0, 0};
    for (size_t k = 0; k + 1 < r->tev.size(); ++k) {
      float t = 0;
      HIPCHK(hipEventElapsedTime(&t, r->tev[k].get(), r->tev[k + 1].get()));
      ms[k & 1] += t;
    }
    memcpy(r->ms, ms, sizeof(ms));
    r->tev.clear();
  }
  return ICTR_OK;
}

extern "C" int ictr_camfit_get_kernel_times(const ictr_camfit *r, float *ms) {
  if (!r || !ms) return fail(ICTR_ERR_INVALID, "camfit_get_kernel_times: NULL argument");
  if (r->out.pending() || !r->timed) return fail(ICTR_ERR_STATE, "camfit_get_kernel_times: no completed timed run");
  memcpy(ms, r->ms, sizeof(r->ms));
  return ICTR_OK;
}

// one pass (or reprojection pass) at the poses G and the ordered sum, on the null stream; st: the frames' states back
static int cf_sums_at(ictr_camfit *r, const double *G, const double *dt, std::vector<CfState> &st) {
  const CfParams p = {0, 1.0, 2.0, 0.0, 1.0};
  CamfitArgs a;
  cf_fill_args(r, p, a);
  a.sums_only = 1;
  if (dt)
    for (int q = 0; q < 3; ++q) a.dt[q] = dt[q];
  st.resize((size_t)r->in.nframes);
  for (int f = 0; f < r->in.nframes; ++f) cf_init(st[(size_t)f], G + 12 * f, p);
  HIPCHK(hipMemcpy(r->out.dev(), st.data(), cf_bytes(r), hipMemcpyHostToDevice));
  if (dt)
    launch_camfit_reproj(a, r->in.nframes, nullptr);
  else
    launch_camfit_pass(a, r->in.nframes, nullptr);
  launch_camfit_step(a, r->in.nframes, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(st.data(), r->out.dev(), cf_bytes(r), hipMemcpyDeviceToHost));
  return ICTR_OK;
}

extern "C" int ictr_camfit_reproj(ictr_camfit *r, const double *G, const double *dt, double *mean_err, int64_t *n) {
  if (!r || !G || !mean_err) return fail(ICTR_ERR_INVALID, "camfit_reproj: NULL argument");
  if (int rc = r->in.ready("camfit_reproj", r->out, "camfit")) return rc;
  if (int rc = cf_poses_finite(G, r->in.nframes, "camfit_reproj")) return rc;
  const double zero[3] = {0.0, 0.0, 0.0};
  if (dt)
    for (int q = 0; q < 3; ++q)
      if (!cf_finite(dt[q])) return fail(ICTR_ERR_INVALID, "camfit_reproj: dt is not finite");
  std::vector<CfState> st;
  if (int rc = cf_sums_at(r, G, dt ? dt : zero, st)) return rc;
  for (int f = 0; f < r->in.nframes; ++f) {
    const double cnt = st[(size_t)f].sums[kCfCountSlot];
    mean_err[f] = cnt > 0.0 ? cf_canon(st[(size_t)f].sums[0] / cnt) : cf_nan();
    if (n) n[f] = (int64_t)cnt;
  }
  return ICTR_OK;
}

// inspection: k_camfit_pass at the poses G [nframes][12] and the ordered sum of k_camfit_step alone, on the null stream
extern "C" int ictr_debug_camfit_pass(ictr_camfit *r, const double *G, int64_t *n, double *s, double *H, double *b) {
  if (!r || !G || !n || !s || !H || !b) return fail(ICTR_ERR_INVALID, "debug_camfit_pass: NULL argument");
  if (int rc = r->in.ready("debug_camfit_pass", r->out, "camfit")) return rc;
  if (int rc = cf_poses_finite(G, r->in.nframes, "debug_camfit_pass")) return rc;
  std::vector<CfState> st;
  if (int rc = cf_sums_at(r, G, nullptr, st)) return rc;
  for (int f = 0; f < r->in.nframes; ++f) {
    const double *v = st[(size_t)f].sums;
    n[f] = (int64_t)v[kCfCountSlot];
    s[f] = v[27];
    memcpy(H + 21 * f, v, sizeof(double) * 21);
    memcpy(b + 6 * f, v + 21, sizeof(double) * 6);
  }
  return ICTR_OK;
}
