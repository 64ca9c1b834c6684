// ictr_ransac.hip -- the hypothesis stage of func_ransac_fitcameras_odom.m (:17-87) on the device.
//
// The trials run in chunks of K, all enqueued on one stream with no host wait between chunks:
//
//   k_ransac_hyp     one lane per trial: 4 distinct match indices from the counter-based stream, undistortion of their
//                    2-D points, the script's degeneracy test (f64), P3P (Lambda Twist) on the first three matches and
//                    the root that reprojects the fourth best -> R, camera centre t and a status.
//                    The solver and the body of a trial after its draws are stated once in ictr_p3p_hd.h, which the window
//                    camera RANSAC (ictr_camransac.hip) shares.
//   k_ransac_score   a workgroup holds a tile of the chunk's hypotheses in LDS; each wave sweeps one 64-match block:
//                    one ballot per hypothesis gives one 64-bit inlier word, popcounts give the counts (integers).
//   k_ransac_select  one workgroup, trial order: successes (status 1, >= 4 inliers, trial < maxtrials) ranked with
//                    ballots and scans, the first nsamples overall accepted; their trial index, draws, R, t and inlier
//                    words copied to the outputs (the log map p = se3_log([R | -R t]) is taken at the read-back, on the
//                    host: the f64 trigonometry of se3_log would put this kernel into scratch memory). Sets `done` when nsamples are held or maxtrials is reached.
//   k_ransac_colsum  after the last chunk: inl_cnt, integer column sums of the accepted rows' inlier bits.
//   k_ransac_finish  one workgroup: the post-filter's compactions (samples s < min(S, N) with inl_cnt[s] <= 4 dropped;
//                    inl_cnt without its entries <= 4), both order-preserving.
//
// Every result is decided by integers and fixed-order f64 arithmetic: the same bits on every run and for every K.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <memory>

#include "ictr_dev.h"
#include "ictr_devfn.h"
#include "ictr_draw_hd.h"
#include "ictr_launch.h"
#include "ictr_p3p_hd.h"
#include "se3_math.h"

namespace ictr {

// one trial: draws, then the hypothesis of ictr_p3p_hd.h on the drawn matches. Returns 1 and fills R, t (camera centre)
// on success; idx gets the drawn indices either way.
__device__ int ransac_trial(const RansacArgs &a, long long g, int *idx, double *Rout, double *tout) {
  if (ran_draw<4>(a.seedmix, g, a.n, idx) < 4) return 0;
  const int n = a.n;
  double P[4][3], u[4], v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = idx[q];
    P[q][0] = a.pts[2 * n + i];
    P[q][1] = a.pts[3 * n + i];
    P[q][2] = a.pts[4 * n + i];
    u[q] = a.pts[i];
    v[q] = a.pts[n + i];
  }
  return p3p_hypothesis(P, u, v, a.fx, a.fy, a.cx, a.cy, a.kc, Rout, tout);
}

__global__ void __launch_bounds__(kRanHypBlock) k_ransac_hyp(RansacArgs a) {
  const int i = blockIdx.x * kRanHypBlock + threadIdx.x;
  if (i >= a.k) return;
  a.cnt[i] = 0u;
  a.status[i] = 0;
  if (a.st->done) return;
  const long long g = a.base + i;
  if (g >= a.maxtrials) return;
  int idx[4] = {0, 0, 0, 0};
  double R[9], t[3];
  const int ok = ransac_trial(a, g, idx, R, t);
  for (int q = 0; q < 4; ++q) a.draws[(size_t)i * 4 + q] = idx[q];
  if (!ok) return;
  double *h = a.hyp + (size_t)i * 12;
  for (int k = 0; k < 9; ++k) h[k] = R[k];
  for (int k = 0; k < 3; ++k) h[9 + k] = t[k];
  a.status[i] = 1;
}

template <int TH>
__global__ void __launch_bounds__(kRanScoreBlock) k_ransac_score(RansacArgs a) {
  __shared__ double sH[TH][12];
  __shared__ int sOk[TH];
  __shared__ unsigned sCnt[TH];
  if (a.st->done) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h0 = blockIdx.x * TH;
  if (tid < TH) {
    sOk[tid] = h0 + tid < a.k ? a.status[h0 + tid] : 0;
    sCnt[tid] = 0u;
  }
  for (int q = tid; q < TH * 12; q += kRanScoreBlock) {
    const int h = q / 12;
    sH[h][q - h * 12] = h0 + h < a.k ? a.hyp[(size_t)(h0 + h) * 12 + (q - h * 12)] : 0.0;
  }
  __syncthreads();
  const int j = blockIdx.y * (kRanScoreBlock / 64) + wave;  // the wave's 64-match block
  if (j < a.nwords) {
    const int n = a.n, m = j * 64 + lane;
    const bool in = m < n;
    const int mm = in ? m : n - 1;
    const double u = a.pts[mm], v = a.pts[n + mm], X = a.pts[2 * n + mm], Y = a.pts[3 * n + mm],
                 Z = a.pts[4 * n + mm];
    const double fx = a.fx, fy = a.fy, cx = a.cx, cy = a.cy, kc = a.kc, thr = a.thr;
    for (int h = 0; h < TH; ++h) {
      if (!sOk[h]) continue;
      const double *G = sH[h];
      const double dX = X - G[9], dY = Y - G[10], dZ = Z - G[11];
      const double xc = G[0] * dX + G[1] * dY + G[2] * dZ;
      const double yc = G[3] * dX + G[4] * dY + G[5] * dZ;
      const double zc = G[6] * dX + G[7] * dY + G[8] * dZ;
      const double iz = 1.0 / zc;
      const double xn = xc * iz, yn = yc * iz;
      const double f = 1.0 + kc * (xn * xn + yn * yn);
      const double du = fx * (xn * f) + cx - u, dv = fy * (yn * f) + cy - v;
      const bool inl = in && sqrt(du * du + dv * dv) <= thr;
      const unsigned long long bits = __ballot(inl);
      if (lane == 0) {
        a.words[(size_t)(h0 + h) * a.nwords + j] = bits;
        atomicAdd(&sCnt[h], (unsigned)__popcll(bits));
      }
    }
  }
  __syncthreads();
  if (tid < TH && sOk[tid] && sCnt[tid]) atomicAdd(&a.cnt[h0 + tid], sCnt[tid]);
}

// exclusive offsets of the waves' ballots (one value per wave in sW) and their total; every thread gets both
__device__ __forceinline__ void ran_wave_scan(unsigned long long m, unsigned *sW, unsigned *off, unsigned *total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (lane == 0) sW[wave] = (unsigned)__popcll(m);
  __syncthreads();
  unsigned o = 0, t = 0;
  for (int w = 0; w < kRanSelBlock / 64; ++w) {
    const unsigned c = sW[w];
    if (w < wave) o += c;
    t += c;
  }
  *off = o + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
  *total = t;
  __syncthreads();
}

__global__ void __launch_bounds__(kRanSelBlock) k_ransac_select(RansacArgs a) {
  __shared__ unsigned sW[kRanSelBlock / 64];
  __shared__ int sLoc[kRanSelBlock];
  __shared__ int sLast;
  RansacState &st = *a.st;
  if (st.done) return;
  const int tid = threadIdx.x;
  long long held = st.held;
  bool done = false;
  for (int r0 = 0; r0 < a.k && !done; r0 += kRanSelBlock) {
    const int i = r0 + tid;
    const long long g = a.base + i;
    const bool succ = i < a.k && g < a.maxtrials && a.status[i] == 1 && a.cnt[i] >= 4u;
    unsigned off, total;
    ran_wave_scan(__ballot(succ), sW, &off, &total);
    const long long rank = held + off;
    const bool acc = succ && rank < a.nsamples;
    if (acc) {
      const double *h = a.hyp + (size_t)i * 12;
      a.o_trial[rank] = g;
      for (int q = 0; q < 4; ++q) a.o_draws[rank * 4 + q] = a.draws[(size_t)i * 4 + q];
      for (int k = 0; k < 9; ++k) a.o_R[rank * 9 + k] = h[k];
      for (int k = 0; k < 3; ++k) a.o_t[rank * 3 + k] = h[9 + k];
      sLoc[off] = i;
      if (rank == a.nsamples - 1) sLast = i;  // the trial that completes the set
    }
    __syncthreads();
    // the accepted rows' inlier words, copied by the whole workgroup
    const long long nacc = min((long long)total, a.nsamples - held);
    for (long long q = 0; q < nacc; ++q) {
      const unsigned long long *src = a.words + (size_t)sLoc[q] * a.nwords;
      unsigned long long *dst = a.o_words + (size_t)(held + q) * a.nwords;
      for (int w = tid; w < a.nwords; w += kRanSelBlock) dst[w] = src[w];
    }
    held += nacc;
    done = held >= a.nsamples;
    __syncthreads();
  }
  if (tid == 0) {
    st.held = held;
    const long long end = min(a.base + a.k, a.maxtrials);
    if (done) {
      st.trials_used = a.base + sLast + 1;
      st.done = 1;
    } else {
      st.trials_used = end;
      if (end >= a.maxtrials) st.done = 1;
    }
  }
}

__global__ void __launch_bounds__(kRanScoreBlock) k_ransac_colsum(RansacArgs a) {
  const int lane = threadIdx.x & 63, j = blockIdx.x * (kRanScoreBlock / 64) + (threadIdx.x >> 6);
  if (j >= a.nwords) return;
  const int m = j * 64 + lane;
  const long long S = a.st->held;
  int c = 0;
  for (long long s = 0; s < S; ++s) c += (int)((a.o_words[(size_t)s * a.nwords + j] >> lane) & 1ull);
  if (m < a.n) a.o_cnt[m] = c;
}

__global__ void __launch_bounds__(kRanSelBlock) k_ransac_finish(RansacArgs a) {
  __shared__ unsigned sW[kRanSelBlock / 64];
  RansacState &st = *a.st;
  const int tid = threadIdx.x;
  const long long S = st.held;
  long long kept = 0;
  for (long long s0 = 0; s0 < S; s0 += kRanSelBlock) {  // R(idxdel) = [] with idxdel = inl_cnt <= 4 (length N)
    const long long s = s0 + tid;
    const bool keep = s < S && !(s < a.n && a.o_cnt[s] <= 4);
    unsigned off, total;
    ran_wave_scan(__ballot(keep), sW, &off, &total);
    if (keep) a.o_keep[kept + off] = (int)s;
    kept += total;
  }
  long long nic = 0;
  for (int m0 = 0; m0 < a.n; m0 += kRanSelBlock) {  // inl_cnt(idxdel) = []
    const int m = m0 + tid;
    const int c = m < a.n ? a.o_cnt[m] : 0;
    const bool keep = m < a.n && c > 4;
    unsigned off, total;
    ran_wave_scan(__ballot(keep), sW, &off, &total);
    if (keep) a.o_cntf[nic + off] = c;
    nic += total;
  }
  if (tid == 0) {
    st.kept = kept;
    st.n_ic = nic;
  }
}

// the hypotheses and scores of one chunk: the launch geometry of k_ransac_hyp and k_ransac_score<tile>, stated once for
// the run (launch_ransac_chunk) and the inspection entry (ictr_debug_ransac_trials)
void launch_ransac_hyp_score(const RansacArgs &a, int tile, hipStream_t s) {
  hipLaunchKernelGGL(k_ransac_hyp, dim3((a.k + kRanHypBlock - 1) / kRanHypBlock), dim3(kRanHypBlock), 0, s, a);
  const int segs = ran_segs(a.nwords, kRanScoreBlock);
  if (tile == 16)
    hipLaunchKernelGGL(k_ransac_score<16>, dim3((a.k + 15) / 16, segs), dim3(kRanScoreBlock), 0, s, a);
  else if (tile == 64)
    hipLaunchKernelGGL(k_ransac_score<64>, dim3((a.k + 63) / 64, segs), dim3(kRanScoreBlock), 0, s, a);
  else
    hipLaunchKernelGGL(k_ransac_score<32>, dim3((a.k + 31) / 32, segs), dim3(kRanScoreBlock), 0, s, a);
}

void launch_ransac_chunk(const RansacArgs &a, int tile, hipStream_t s) {
  launch_ransac_hyp_score(a, tile, s);
  hipLaunchKernelGGL(k_ransac_select, dim3(1), dim3(kRanSelBlock), 0, s, a);
}

void launch_ransac_finish(const RansacArgs &a, hipStream_t s) {
  const int segs = ran_segs(a.nwords, kRanScoreBlock);
  hipLaunchKernelGGL(k_ransac_colsum, dim3(segs), dim3(kRanScoreBlock), 0, s, a);
  hipLaunchKernelGGL(k_ransac_finish, dim3(1), dim3(kRanSelBlock), 0, s, a);
}

}  // namespace ictr

using namespace ictr;

// ---------------------------------------------------------------- host side (func_ransac_fitcameras_odom.m:17-87)
// The trials run in chunks of K on one stream (ictr_ransac.hip): hypotheses, scoring, ordered selection per chunk, then
// the post-filter once. Chunks are enqueued in groups; between two groups the run reads the 4-byte `done` flag, so a
// run whose samples are found early does not enqueue the rest. One read-back at the end.
static constexpr int kRanGroup = 64;  // chunks enqueued between two reads of `done`

struct ictr_ransac {
  int n = 0, nwords = 0;
  int64_t smax = 0;
  int chunk = 0, tile = 32;
  hipStream_t stream = nullptr;
  DevBuf<double> d_pts, d_hyp;
  DevBuf<int> d_draws, d_status;
  DevBuf<unsigned> d_cnt;
  DevBuf<unsigned long long> d_words;
  bool points_set = false;
  Readback out;  // (ran_layout) declared last, so destroyed first: a run in flight ends before a buffer goes
};

// RansacState | trial [smax] i64 | draws [smax][4] i32 | R [smax][9] | t [smax][3] | words [smax][nwords] | cnt [n] |
// keep [smax] | cntf [n], each on a 16-byte boundary
struct RanLayout {
  Part trial, draws, R, t, words, cnt, keep, cntf, end;  // end: empty, at the block's size
};
static RanLayout ran_layout(const ictr_ransac *r) {
  Carve c;
  const size_t S = (size_t)r->smax, n = (size_t)r->n;
  c.take(sizeof(RansacState), 16);  // at the front
  return {c.take(8 * S, 16), c.take(16 * S, 16), c.take(72 * S, 16), c.take(24 * S, 16), c.take(8 * S * r->nwords, 16),
          c.take(4 * n, 16), c.take(4 * S, 16), c.take(4 * n, 16), c.take(0, 16)};  // braces: evaluated in this order
}

// trials per chunk: enough that one chunk's scoring (K x N lane tests) fills the device; ICTR_RANSAC_CHUNK overrides.
// Constants from tools/ransac_bench.py --sweep (profiles/ransac_sweep.json).
static int ransac_chunk(int n) {
  const int env = env_int("ICTR_RANSAC_CHUNK", 0);
  if (env > 0) return env;
  long long k = (1ll << 23) / n;
  k = std::max(256ll, std::min(16384ll, k));
  return (int)((k + 255) / 256 * 256);
}

extern "C" int ictr_ransac_create(ictr_ransac **out, int64_t n, int64_t max_samples) {
  if (!out) return fail(ICTR_ERR_INVALID, "ransac_create: NULL argument");
  if (n < 4 || n > ((int64_t)1 << 24))
    return fail(ICTR_ERR_INVALID, "ransac_create: %lld matches (4 .. 2^24)", (long long)n);
  if (max_samples < 1 || max_samples > ((int64_t)1 << 24))
    return fail(ICTR_ERR_INVALID, "ransac_create: max_samples %lld (1 .. 2^24)", (long long)max_samples);
  if (int rc = need_device()) return rc;
  auto r = std::make_unique<ictr_ransac>();
  r->n = (int)n;
  r->nwords = (int)((n + 63) / 64);
  r->smax = max_samples;
  r->chunk = ransac_chunk(r->n);
  r->tile = ran_tile_env("ICTR_RANSAC_TILE");
  const size_t K = (size_t)r->chunk;
  if (int rc = r->d_pts.alloc(sizeof(double) * 5 * n, true)) return rc;
  if (int rc = r->d_hyp.alloc(sizeof(double) * 12 * K, true)) return rc;
  if (int rc = r->d_draws.alloc(sizeof(int) * 4 * K, true)) return rc;
  if (int rc = r->d_status.alloc(sizeof(int) * K, true)) return rc;
  if (int rc = r->d_cnt.alloc(sizeof(unsigned) * K, true)) return rc;
  if (int rc = r->d_words.alloc(sizeof(unsigned long long) * K * r->nwords, true)) return rc;
  if (int rc = r->out.reserve(ran_layout(r.get()).end.at, true)) return rc;
  *out = r.release();
  return ICTR_OK;
}

extern "C" void ictr_ransac_destroy(ictr_ransac *r) { delete r; }

extern "C" int ictr_ransac_set_points(ictr_ransac *r, const double *pt2d, const double *pt3d) {
  if (!r || !pt2d || !pt3d) return fail(ICTR_ERR_INVALID, "ransac_set_points: NULL argument");
  if (int rc = r->out.refuse("ransac_set_points", "ransac")) return rc;
  const size_t n = (size_t)r->n;
  HIPCHK(hipMemcpy(r->d_pts.get(), pt2d, sizeof(double) * 2 * n, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(r->d_pts.get() + 2 * n, pt3d, sizeof(double) * 3 * n, hipMemcpyHostToDevice));
  r->points_set = true;
  return ICTR_OK;
}

extern "C" int ictr_ransac_chunk_size(const ictr_ransac *r) { return r ? r->chunk : 0; }

// the camera checked, and every field of the kernels' argument block that does not depend on the trial range
static int ran_fill_args(const ictr_ransac *r, const char *what, const double *fc, const double *cc, double kc,
                         double inlthresh, uint64_t seed, RansacArgs &a) {
  if (!std::isfinite(inlthresh)) return fail(ICTR_ERR_INVALID, "%s: inlthresh is not finite", what);
  if (!std::isfinite(kc) || !std::isfinite(fc[0]) || !std::isfinite(fc[1]) || fc[0] == 0.0 || fc[1] == 0.0 ||
      !std::isfinite(cc[0]) || !std::isfinite(cc[1]))
    return fail(ICTR_ERR_INVALID, "%s: the camera (fc, cc, kc) must be finite, fc non-zero", what);
  const RanLayout L = ran_layout(r);
  memset(&a, 0, sizeof(a));
  a.pts = r->d_pts.get();
  a.n = r->n;
  a.nwords = r->nwords;
  a.fx = fc[0];
  a.fy = fc[1];
  a.cx = cc[0];
  a.cy = cc[1];
  a.kc = kc;
  a.thr = inlthresh;
  a.seedmix = ran_seed(seed);
  a.hyp = r->d_hyp.get();
  a.draws = r->d_draws.get();
  a.status = r->d_status.get();
  a.cnt = r->d_cnt.get();
  a.words = r->d_words.get();
  a.st = reinterpret_cast<RansacState *>(r->out.dev());
  a.o_trial = reinterpret_cast<long long *>(r->out.dev() + L.trial.at);
  a.o_draws = reinterpret_cast<int *>(r->out.dev() + L.draws.at);
  a.o_R = reinterpret_cast<double *>(r->out.dev() + L.R.at);
  a.o_t = reinterpret_cast<double *>(r->out.dev() + L.t.at);
  a.o_words = reinterpret_cast<unsigned long long *>(r->out.dev() + L.words.at);
  a.o_cnt = reinterpret_cast<int *>(r->out.dev() + L.cnt.at);
  a.o_keep = reinterpret_cast<int *>(r->out.dev() + L.keep.at);
  a.o_cntf = reinterpret_cast<int *>(r->out.dev() + L.cntf.at);
  return ICTR_OK;
}

extern "C" int ictr_ransac_run(ictr_ransac *r, const double *fc, const double *cc, double kc, int64_t nsamples,
                               int64_t maxtrials, double inlthresh, uint64_t seed, void *hip_stream) {
  if (!r || !fc || !cc) return fail(ICTR_ERR_INVALID, "ransac_run: NULL argument");
  if (int rc = r->out.refuse("ransac_run", "ransac")) return rc;
  if (!r->points_set) return fail(ICTR_ERR_STATE, "ransac_run: ictr_ransac_set_points has not been called");
  if (nsamples < 1 || nsamples > r->smax)
    return fail(ICTR_ERR_INVALID, "ransac_run: nsamples %lld (1 .. %lld, the size given at creation)",
                (long long)nsamples, (long long)r->smax);
  if (maxtrials < 1 || maxtrials > ((int64_t)1 << 40))
    return fail(ICTR_ERR_INVALID, "ransac_run: maxtrials %lld (1 .. 2^40)", (long long)maxtrials);
  RansacArgs a;
  if (int rc = ran_fill_args(r, "ransac_run", fc, cc, kc, inlthresh, seed, a)) return rc;
  r->stream = (hipStream_t)hip_stream;
  a.nsamples = nsamples;
  a.maxtrials = maxtrials;
  HIPCHK(hipMemsetAsync(a.st, 0, sizeof(RansacState), r->stream));
  const int64_t K = r->chunk;
  const int64_t nchunks = (maxtrials + K - 1) / K;
  for (int64_t c = 0; c < nchunks; ++c) {
    if (c > 0 && c % kRanGroup == 0) {  // a long run: stop enqueueing once the samples are found
      RansacState *hs = reinterpret_cast<RansacState *>(r->out.host());
      HIPCHK(hipMemcpyAsync(&hs->done, &a.st->done, sizeof(int), hipMemcpyDeviceToHost, r->stream));
      HIPCHK(hipStreamSynchronize(r->stream));
      if (*(volatile int *)&hs->done) break;
    }
    a.base = c * K;
    a.k = (int)std::min<int64_t>(K, maxtrials - a.base);
    launch_ransac_chunk(a, r->tile, r->stream);
    HIPCHK(hipGetLastError());
  }
  launch_ransac_finish(a, r->stream);
  HIPCHK(hipGetLastError());
  return r->out.post(ran_layout(r).end.at, r->stream);
}

extern "C" int ictr_ransac_wait(ictr_ransac *r, int64_t *counts, double *R, double *t, double *p, uint64_t *inl_words,
                                int32_t *inl_cnt) {
  if (!r) return fail(ICTR_ERR_INVALID, "ransac is NULL");
  if (!r->out.pending()) return fail(ICTR_ERR_STATE, "ransac_wait: nothing has been run");
  if (int rc = r->out.wait()) return rc;
  const RanLayout L = ran_layout(r);
  const RansacState &st = *reinterpret_cast<const RansacState *>(r->out.host());
  const int *keep = reinterpret_cast<const int *>(r->out.host() + L.keep.at);
  const double *hR = reinterpret_cast<const double *>(r->out.host() + L.R.at);
  const double *ht = reinterpret_cast<const double *>(r->out.host() + L.t.at);
  const uint64_t *hw = reinterpret_cast<const uint64_t *>(r->out.host() + L.words.at);
  if (counts) {
    counts[0] = st.kept;
    counts[1] = st.held;
    counts[2] = st.trials_used;
    counts[3] = st.n_ic;
  }
  for (long long q = 0; q < st.kept; ++q) {
    const size_t s = (size_t)keep[q];
    if (R) memcpy(R + 9 * q, hR + 9 * s, 9 * sizeof(double));
    if (t) memcpy(t + 3 * q, ht + 3 * s, 3 * sizeof(double));
    if (p) {  // p = se3_log([R | -R t]) (ictr_ransac.hip: on the host, at the read-back)
      const double *Rs = hR + 9 * s, *ts = ht + 3 * s;
      double G[12];
      for (int i = 0; i < 3; ++i) {
        for (int c = 0; c < 3; ++c) G[i * 4 + c] = Rs[i * 3 + c];
        G[i * 4 + 3] = -Rs[i * 3 + 0] * ts[0] - Rs[i * 3 + 1] * ts[1] - Rs[i * 3 + 2] * ts[2];
      }
      se3_log<double>(p + 6 * q, G);
    }
    if (inl_words) memcpy(inl_words + (size_t)r->nwords * q, hw + (size_t)r->nwords * s, 8 * (size_t)r->nwords);
  }
  if (inl_cnt) memcpy(inl_cnt, r->out.host() + L.cntf.at, sizeof(int32_t) * (size_t)st.n_ic);
  return ICTR_OK;
}

extern "C" int ictr_ransac_samples(const ictr_ransac *r, int64_t *trial, int32_t *draws) {
  if (!r) return fail(ICTR_ERR_INVALID, "ransac is NULL");
  if (r->out.pending() || !r->out.ran()) return fail(ICTR_ERR_STATE, "ransac_samples: no completed run");
  const RanLayout L = ran_layout(r);
  const RansacState &st = *reinterpret_cast<const RansacState *>(r->out.host());
  const int *keep = reinterpret_cast<const int *>(r->out.host() + L.keep.at);
  const long long *ht = reinterpret_cast<const long long *>(r->out.host() + L.trial.at);
  const int *hd = reinterpret_cast<const int *>(r->out.host() + L.draws.at);
  for (long long q = 0; q < st.kept; ++q) {
    if (trial) trial[q] = ht[keep[q]];
    if (draws) memcpy(draws + 4 * q, hd + 4 * (size_t)keep[q], 4 * sizeof(int32_t));
  }
  return ICTR_OK;
}

// inspection: hypotheses and scores of trials [first_trial, first_trial + count), in the object's own chunks and tile,
// on the null stream. No select runs and `done` stays clear, so every trial of the range is computed.
extern "C" int ictr_debug_ransac_trials(ictr_ransac *r, const double *fc, const double *cc, double kc, double inlthresh,
                                        uint64_t seed, int64_t first_trial, int64_t count, int32_t *status,
                                        int32_t *draws, double *hyp, uint32_t *cnt, uint64_t *words) {
  if (!r || !fc || !cc || !status || !draws || !hyp || !cnt || !words)
    return fail(ICTR_ERR_INVALID, "debug_ransac_trials: NULL argument");
  if (int rc = r->out.refuse("debug_ransac_trials", "ransac")) return rc;
  if (!r->points_set) return fail(ICTR_ERR_STATE, "debug_ransac_trials: ictr_ransac_set_points has not been called");
  if (count < 1 || count > ((int64_t)1 << 20) || first_trial < 0 || first_trial > ((int64_t)1 << 40) - count)
    return fail(ICTR_ERR_INVALID, "debug_ransac_trials: trials %lld + %lld (1 .. 2^20 trials below 2^40)",
                (long long)first_trial, (long long)count);
  RansacArgs a;
  if (int rc = ran_fill_args(r, "debug_ransac_trials", fc, cc, kc, inlthresh, seed, a)) return rc;
  a.nsamples = 1;
  a.maxtrials = first_trial + count;
  HIPCHK(hipMemsetAsync(a.st, 0, sizeof(RansacState), nullptr));
  const int64_t K = r->chunk;
  const size_t W = (size_t)r->nwords;
  for (int64_t done = 0; done < count; done += K) {
    a.base = first_trial + done;
    a.k = (int)std::min<int64_t>(K, count - done);
    const size_t k = (size_t)a.k, o = (size_t)done;
    launch_ransac_hyp_score(a, r->tile, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(status + o, r->d_status.get(), sizeof(int32_t) * k, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(draws + 4 * o, r->d_draws.get(), sizeof(int32_t) * 4 * k, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hyp + 12 * o, r->d_hyp.get(), sizeof(double) * 12 * k, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cnt + o, r->d_cnt.get(), sizeof(uint32_t) * k, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(words + W * o, r->d_words.get(), sizeof(uint64_t) * W * k, hipMemcpyDeviceToHost));
  }
  return ICTR_OK;
}
