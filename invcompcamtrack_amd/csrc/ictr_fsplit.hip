// ictr_fsplit.hip -- "Divide points in static and dynamic using the fundamental matrix" (misc_src/run_test_OF_track.py:
// 309-343) on the device: RANSAC over 8-point fundamental matrices of P view pairs of the same N points.
//
// The trials run in chunks of K, all enqueued on one stream with no host wait in between:
//
//   k_fsplit_fit     one lane per (trial, pair): the trial's 8 distinct point indices from the counter-based stream
//                    (every lane of a trial draws the same), the pair's 8 correspondences, fs_fit8 -> F [9] and a
//                    per-pair status; nine NaN where the fit failed, so a failed trial scores nothing by arithmetic alone.
//   k_fsplit_score   a workgroup holds a tile of T trials x 320 / T pairs of matrices in LDS, one lane per point: per pair
//                    the point's four coordinates are read once and serve all T trials, a running maximum per trial stays
//                    in registers; after the last pair tile one ballot per trial, popcounts summed in LDS, one integer
//                    atomic per trial and workgroup. No inlier words are written.
//   k_fsplit_select  one workgroup: the chunk's largest count (lowest trial on ties) against the best of the chunks before
//                    (strictly greater wins); the winner's matrices and draws are copied next to the state.
//   k_fsplit_mask    after the last chunk, for the winner only: distances and inlier words, with the device functions
//                    of the score kernel (the same bits by construction).
//
// Every result is decided by integers and fixed-order f64 arithmetic (ictr_fsplit_hd.h): the same bits on every run,
// for every K and every T.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "ictr_dev.h"
#include "ictr_devfn.h"
#include "ictr_draw_hd.h"
#include "ictr_fsplit_hd.h"
#include "ictr_launch.h"

namespace ictr {

__global__ void __launch_bounds__(kFsFitBlock) k_fsplit_fit(FsplitArgs a) {
  const long long g = (long long)blockIdx.x * kFsFitBlock + threadIdx.x;
  if (g >= (long long)a.k * a.np) return;
  const int i = (int)(g / a.np), p = (int)(g - (long long)i * a.np);
  int idx[8];
  const int nd = ran_draw<8>(a.seedmix, a.base + i, a.n, idx);
  if (p == 0) {
    a.cnt[i] = 0u;
#pragma unroll
    for (int q = 0; q < 8; ++q) a.draws[(size_t)i * 8 + q] = idx[q];
  }
  double F[9];
  bool ok = false;
  if (nd == 8) {
    const double *b = a.xy + (size_t)p * 4 * a.n;
    double xa[8], ya[8], xb[8], yb[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      xa[q] = b[idx[q]];
      ya[q] = b[(size_t)a.n + idx[q]];
      xb[q] = b[2 * (size_t)a.n + idx[q]];
      yb[q] = b[3 * (size_t)a.n + idx[q]];
    }
    ok = fs_fit8(xa, ya, xb, yb, F);
  } else {
#pragma unroll
    for (int q = 0; q < 9; ++q) F[q] = fs_nan();
  }
  double *o = a.F + (size_t)g * 9;
#pragma unroll
  for (int q = 0; q < 9; ++q) o[q] = F[q];
  a.pst[g] = ok ? 1 : 0;
}

template <int TH>
__global__ void __launch_bounds__(kFsScoreBlock) k_fsplit_score(FsplitArgs a) {
  constexpr int PT = kFsTileMats / TH;  // pairs per LDS tile
  __shared__ double sF[TH * PT * 9];
  __shared__ int sOk[TH];
  __shared__ unsigned sCnt[TH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h0 = blockIdx.x * TH, np = a.np, n = a.n;
  if (tid < TH) {
    int ok = h0 + tid < a.k ? 1 : 0;
    if (ok)
      for (int p = 0; p < np; ++p) ok &= a.pst[(size_t)(h0 + tid) * np + p];
    sOk[tid] = ok;
    sCnt[tid] = 0u;
  }
  const int j = blockIdx.y * (kFsScoreBlock / 64) + wave;  // the wave's 64-point block
  const bool live = j < a.nwords;
  const int m = j * 64 + lane;
  const bool in = live && m < n;
  const int mm = in ? m : n - 1;
  double mx[TH];
#pragma unroll
  for (int h = 0; h < TH; ++h) mx[h] = -1.0;
  for (int p0 = 0; p0 < np; p0 += PT) {
    const int pt = min(PT, np - p0);
    __syncthreads();  // the tile before has been used (first pass: sOk is complete)
    for (int q = tid; q < TH * pt * 9; q += kFsScoreBlock) {
      const int h = q / (pt * 9), r = q - h * (pt * 9);
      sF[h * (PT * 9) + r] = h0 + h < a.k ? a.F[((size_t)(h0 + h) * np + p0) * 9 + r] : 0.0;
    }
    __syncthreads();
    if (live) {
      for (int pp = 0; pp < pt; ++pp) {
        const double *b = a.xy + (size_t)(p0 + pp) * 4 * n;
        const double xa = b[mm], ya = b[(size_t)n + mm], xb = b[2 * (size_t)n + mm], yb = b[3 * (size_t)n + mm];
#pragma unroll
        for (int h = 0; h < TH; ++h) {
          if (!sOk[h]) continue;
          mx[h] = fs_max(mx[h], fs_dist(&sF[(h * PT + pp) * 9], xa, ya, xb, yb));
        }
      }
    }
  }
  if (live) {
    const double thr = a.thr;
#pragma unroll
    for (int h = 0; h < TH; ++h) {
      if (!sOk[h]) continue;
      const unsigned long long bits = __ballot(in && mx[h] < thr);
      if (lane == 0 && bits) atomicAdd(&sCnt[h], (unsigned)__popcll(bits));
    }
  }
  __syncthreads();
  if (tid < TH && sOk[tid] && sCnt[tid]) atomicAdd(&a.cnt[h0 + tid], sCnt[tid]);
}

__global__ void __launch_bounds__(kFsSelBlock) k_fsplit_select(FsplitArgs a) {
  __shared__ unsigned long long sKey[kFsSelBlock / 64];
  __shared__ int sWin;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // key: count in the high word, ~index in the low one: the largest key is the largest count at the lowest index
  unsigned long long key = 0ull;
  for (int i = tid; i < a.k; i += kFsSelBlock) {
    const unsigned long long c = ((unsigned long long)a.cnt[i] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
    key = c > key ? c : key;
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const unsigned long long o = __shfl_xor(key, s, 64);
    key = o > key ? o : key;
  }
  if (lane == 0) sKey[wave] = key;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kFsSelBlock / 64; ++w) key = sKey[w] > key ? sKey[w] : key;
    const int idx = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
    const long long c = (long long)(key >> 32);
    const bool take = a.base == 0 || c > a.st->best_count;  // strictly more: the earlier trial keeps a tie
    if (take) {
      a.st->best_trial = a.base + idx;
      a.st->best_count = c;
    }
    sWin = take ? idx : -1;
  }
  __syncthreads();
  const int win = sWin;
  if (win < 0) return;
  for (int q = tid; q < a.np * 9; q += kFsSelBlock) a.o_F[q] = a.F[(size_t)win * a.np * 9 + q];
  if (tid < 8) a.st->draws[tid] = a.draws[(size_t)win * 8 + tid];
}

__global__ void __launch_bounds__(kFsScoreBlock) k_fsplit_mask(FsplitArgs a) {
  __shared__ double sF[kFsMaxPairs * 9];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int np = a.np, n = a.n;
  for (int q = tid; q < np * 9; q += kFsScoreBlock) sF[q] = a.o_F[q];
  __syncthreads();
  const int j = blockIdx.x * (kFsScoreBlock / 64) + wave;
  if (j >= a.nwords) return;
  const int m = j * 64 + lane;
  const bool in = m < n;
  const int mm = in ? m : n - 1;
  double mx = -1.0;
  for (int p = 0; p < np; ++p) {
    const double *b = a.xy + (size_t)p * 4 * n;
    mx = fs_max(mx, fs_dist(&sF[p * 9], b[mm], b[(size_t)n + mm], b[2 * (size_t)n + mm], b[3 * (size_t)n + mm]));
  }
  if (in) a.o_dd[m] = mx;
  const unsigned long long bits = __ballot(in && mx < a.thr);
  if (lane == 0) a.o_words[j] = bits;
}

// the fits and scores of one chunk: the launch geometry of k_fsplit_fit and k_fsplit_score<tile>, stated once for the
// run and the inspection entry (ictr_debug_fsplit_trials). after_fit (optional, timing runs): recorded between the two.
void launch_fsplit_fit_score(const FsplitArgs &a, int tile, hipStream_t s, hipEvent_t after_fit) {
  const long long fits = (long long)a.k * a.np;
  hipLaunchKernelGGL(k_fsplit_fit, dim3((unsigned)((fits + kFsFitBlock - 1) / kFsFitBlock)), dim3(kFsFitBlock), 0, s, a);
  if (after_fit) (void)hipEventRecord(after_fit, s);
  const int segs = ran_segs(a.nwords, kFsScoreBlock);
  if (tile == 16)
    hipLaunchKernelGGL(k_fsplit_score<16>, dim3((a.k + 15) / 16, segs), dim3(kFsScoreBlock), 0, s, a);
  else if (tile == 64)
    hipLaunchKernelGGL(k_fsplit_score<64>, dim3((a.k + 63) / 64, segs), dim3(kFsScoreBlock), 0, s, a);
  else
    hipLaunchKernelGGL(k_fsplit_score<32>, dim3((a.k + 31) / 32, segs), dim3(kFsScoreBlock), 0, s, a);
}

void launch_fsplit_select(const FsplitArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_fsplit_select, dim3(1), dim3(kFsSelBlock), 0, s, a);
}

void launch_fsplit_mask(const FsplitArgs &a, hipStream_t s) {
  const int segs = ran_segs(a.nwords, kFsScoreBlock);
  hipLaunchKernelGGL(k_fsplit_mask, dim3(segs), dim3(kFsScoreBlock), 0, s, a);
}

}  // namespace ictr

using namespace ictr;

// ---------------------------------------------------------------- host side
struct ictr_fsplit {
  int n = 0, nwords = 0, np = 0;
  int chunk = 0, tile = 32;
  DevBuf<double> d_xy, d_F;
  DevBuf<int> d_draws, d_pst;
  DevBuf<unsigned> d_cnt;
  bool pairs_set = false;
  bool timing = false, timed = false;  // timed: the run in flight (or last waited) carries events
  std::vector<Event> tev;              // per chunk: before fit, after fit, after score, after select; then after mask
  float ms[4] = {0, 0, 0, 0};
  // (fs_layout) declared last, so destroyed first: a run in flight ends before a buffer or a timing event goes
  Readback out;
};

struct FsLayout {  // FsplitState | F [np][9] | words [nwords] | dd [n], each on a 16-byte boundary
  Part F, words, dd, end;  // end: empty, at the block's size
};
static FsLayout fs_layout(const ictr_fsplit *r) {
  Carve c;
  c.take(sizeof(FsplitState), 16);  // at the front
  return {c.take(72 * (size_t)r->np, 16), c.take(8 * (size_t)r->nwords, 16), c.take(8 * (size_t)r->n, 16),
          c.take(0, 16)};  // braces: evaluated in this order
}

extern "C" int ictr_fsplit_create(ictr_fsplit **out, int64_t n, int64_t npairs) {
  if (!out) return fail(ICTR_ERR_INVALID, "fsplit_create: NULL argument");
  if (n < 8 || n > ((int64_t)1 << 22))
    return fail(ICTR_ERR_INVALID, "fsplit_create: %lld points (8 .. 2^22)", (long long)n);
  if (npairs < 1 || npairs > kFsMaxPairs)
    return fail(ICTR_ERR_INVALID, "fsplit_create: %lld view pairs (1 .. %d)", (long long)npairs, kFsMaxPairs);
  if (int rc = need_device()) return rc;
  auto r = std::make_unique<ictr_fsplit>();
  r->n = (int)n;
  r->nwords = (int)((n + 63) / 64);
  r->np = (int)npairs;
  // trials per chunk: the matrices of a chunk (K x P x 72 B) stay below 19 MB; ICTR_FSPLIT_CHUNK overrides
  const int chunk = env_int("ICTR_FSPLIT_CHUNK", 0);
  r->chunk = chunk > 0 ? std::min(chunk, 1 << 16) : 4096;
  r->tile = ran_tile_env("ICTR_FSPLIT_TILE");
  const size_t K = (size_t)r->chunk, P = (size_t)r->np;
  if (int rc = r->d_xy.alloc(sizeof(double) * 4 * P * (size_t)n, true)) return rc;
  if (int rc = r->d_F.alloc(sizeof(double) * 9 * K * P, true)) return rc;
  if (int rc = r->d_draws.alloc(sizeof(int) * 8 * K, true)) return rc;
  if (int rc = r->d_pst.alloc(sizeof(int) * K * P, true)) return rc;
  if (int rc = r->d_cnt.alloc(sizeof(unsigned) * K, true)) return rc;
  if (int rc = r->out.reserve(fs_layout(r.get()).end.at, true)) return rc;
  *out = r.release();
  return ICTR_OK;
}

extern "C" void ictr_fsplit_destroy(ictr_fsplit *r) { delete r; }

extern "C" int ictr_fsplit_set_pairs(ictr_fsplit *r, const double *xy) {
  if (!r || !xy) return fail(ICTR_ERR_INVALID, "fsplit_set_pairs: NULL argument");
  if (int rc = r->out.refuse("fsplit_set_pairs", "fsplit")) return rc;
  HIPCHK(hipMemcpy(r->d_xy.get(), xy, sizeof(double) * 4 * (size_t)r->np * (size_t)r->n, hipMemcpyHostToDevice));
  r->pairs_set = true;
  return ICTR_OK;
}

extern "C" int ictr_fsplit_view_(const ictr_fsplit *r, ictr_fsplit_view *v) {
  v->xy = r->d_xy.get();
  v->n = r->n;
  v->np = r->np;
  v->pending = r->out.pending();
  return ICTR_OK;
}

extern "C" int ictr_fsplit_mask_(const ictr_fsplit *r, WinMaskSrc *m) {
  *m = {reinterpret_cast<const unsigned long long *>(r->out.dev() + fs_layout(r).words.at), r->n, r->out.ran(), "split"};
  return ICTR_OK;
}

extern "C" void ictr_fsplit_pairs_filled_(ictr_fsplit *r) { r->pairs_set = true; }

extern "C" int ictr_fsplit_set_timing(ictr_fsplit *r, int on) {
  if (!r) return fail(ICTR_ERR_INVALID, "fsplit is NULL");
  if (int rc = r->out.refuse("fsplit_set_timing", "fsplit")) return rc;
  r->timing = on != 0;
  return ICTR_OK;
}

// every field of the kernels' argument block that does not depend on the trial range
static int fs_fill_args(const ictr_fsplit *r, const char *what, double thresh, uint64_t seed, FsplitArgs &a) {
  if (std::isnan(thresh)) return fail(ICTR_ERR_INVALID, "%s: thresh is NaN", what);
  const FsLayout L = fs_layout(r);
  memset(&a, 0, sizeof(a));
  a.xy = r->d_xy.get();
  a.n = r->n;
  a.nwords = r->nwords;
  a.np = r->np;
  a.thr = thresh;
  a.seedmix = ran_seed(seed);
  a.F = r->d_F.get();
  a.draws = r->d_draws.get();
  a.pst = r->d_pst.get();
  a.cnt = r->d_cnt.get();
  a.st = reinterpret_cast<FsplitState *>(r->out.dev());
  a.o_F = reinterpret_cast<double *>(r->out.dev() + L.F.at);
  a.o_words = reinterpret_cast<unsigned long long *>(r->out.dev() + L.words.at);
  a.o_dd = reinterpret_cast<double *>(r->out.dev() + L.dd.at);
  return ICTR_OK;
}

extern "C" int ictr_fsplit_run(ictr_fsplit *r, int64_t ntrials, double thresh, uint64_t seed, void *hip_stream) {
  if (!r) return fail(ICTR_ERR_INVALID, "fsplit is NULL");
  if (int rc = r->out.refuse("fsplit_run", "fsplit")) return rc;
  if (!r->pairs_set) return fail(ICTR_ERR_STATE, "fsplit_run: ictr_fsplit_set_pairs has not been called");
  if (ntrials < 1 || ntrials > ((int64_t)1 << 20))
    return fail(ICTR_ERR_INVALID, "fsplit_run: ntrials %lld (1 .. 2^20)", (long long)ntrials);
  FsplitArgs a;
  if (int rc = fs_fill_args(r, "fsplit_run", thresh, seed, a)) return rc;
  const int64_t K = r->chunk;
  const int64_t nchunks = (ntrials + K - 1) / K;
  std::vector<Event> tev;
  if (r->timing) {
    tev.resize((size_t)nchunks * 4 + 1);
    for (Event &e : tev)
      if (int rc = e.create()) return rc;
  }
  hipStream_t s = (hipStream_t)hip_stream;
  for (int64_t c = 0; c < nchunks; ++c) {
    a.base = c * K;
    a.k = (int)std::min<int64_t>(K, ntrials - a.base);
    Event *e = r->timing ? &tev[(size_t)c * 4] : nullptr;
    if (e) HIPCHK(hipEventRecord(e[0].get(), s));
    launch_fsplit_fit_score(a, r->tile, s, e ? e[1].get() : nullptr);
    if (e) HIPCHK(hipEventRecord(e[2].get(), s));
    launch_fsplit_select(a, s);
    if (e) HIPCHK(hipEventRecord(e[3].get(), s));
    HIPCHK(hipGetLastError());
  }
  launch_fsplit_mask(a, s);
  HIPCHK(hipGetLastError());
  if (r->timing) HIPCHK(hipEventRecord(tev.back().get(), s));
  if (int rc = r->out.post(fs_layout(r).end.at, s)) return rc;
  r->tev = std::move(tev);
  r->timed = r->timing;
  return ICTR_OK;
}

extern "C" int ictr_fsplit_wait(ictr_fsplit *r, int64_t *best_trial, int64_t *best_count, int32_t *draws, double *F,
                                uint64_t *inl_words, double *dd) {
  if (!r) return fail(ICTR_ERR_INVALID, "fsplit is NULL");
  if (!r->out.pending()) return fail(ICTR_ERR_STATE, "fsplit_wait: nothing has been run");
  if (int rc = r->out.wait()) return rc;
  const FsLayout L = fs_layout(r);
  const FsplitState &st = *reinterpret_cast<const FsplitState *>(r->out.host());
  if (best_trial) *best_trial = st.best_trial;
  if (best_count) *best_count = st.best_count;
  if (draws) memcpy(draws, st.draws, sizeof(st.draws));
  if (F) memcpy(F, r->out.host() + L.F.at, L.F.bytes);
  if (inl_words) memcpy(inl_words, r->out.host() + L.words.at, L.words.bytes);
  if (dd) memcpy(dd, r->out.host() + L.dd.at, L.dd.bytes);
  if (r->timed) {
    float ms[4] = {0, 0, 0, 0};
    const size_t nchunks = (r->tev.size() - 1) / 4;
    for (size_t c = 0; c < nchunks; ++c)
      for (int k = 0; k < 3; ++k) {
        float t = 0;
        HIPCHK(hipEventElapsedTime(&t, r->tev[c * 4 + k].get(), r->tev[c * 4 + k + 1].get()));
        ms[k] += t;
      }
    HIPCHK(hipEventElapsedTime(&ms[3], r->tev[r->tev.size() - 2].get(), r->tev.back().get()));
    memcpy(r->ms, ms, sizeof(ms));
    r->tev.clear();
  }
  return ICTR_OK;
}

extern "C" int ictr_fsplit_get_kernel_times(const ictr_fsplit *r, float *ms) {
  if (!r || !ms) return fail(ICTR_ERR_INVALID, "fsplit_get_kernel_times: NULL argument");
  if (r->out.pending() || !r->timed) return fail(ICTR_ERR_STATE, "fsplit_get_kernel_times: no completed timed run");
  memcpy(ms, r->ms, sizeof(r->ms));
  return ICTR_OK;
}

// inspection: fits and scores of trials [first_trial, first_trial + count), in the object's own chunks and tile, on the
// null stream. No select runs: the object's best trial is left alone.
extern "C" int ictr_debug_fsplit_trials(ictr_fsplit *r, double thresh, uint64_t seed, int64_t first_trial, int64_t count,
                                        int32_t *status, int32_t *draws, double *F, uint32_t *cnt) {
  if (!r || !status || !draws || !F || !cnt) return fail(ICTR_ERR_INVALID, "debug_fsplit_trials: NULL argument");
  if (int rc = r->out.refuse("debug_fsplit_trials", "fsplit")) return rc;
  if (!r->pairs_set) return fail(ICTR_ERR_STATE, "debug_fsplit_trials: ictr_fsplit_set_pairs has not been called");
  if (count < 1 || count > ((int64_t)1 << 20) || first_trial < 0 || first_trial > ((int64_t)1 << 20) - count)
    return fail(ICTR_ERR_INVALID, "debug_fsplit_trials: trials %lld + %lld (1 .. 2^20 trials below 2^20)",
                (long long)first_trial, (long long)count);
  FsplitArgs a;
  if (int rc = fs_fill_args(r, "debug_fsplit_trials", thresh, seed, a)) return rc;
  const int64_t K = r->chunk;
  const size_t P = (size_t)r->np;
  std::vector<int32_t> pst((size_t)std::min<int64_t>(K, count) * P);
  for (int64_t done = 0; done < count; done += K) {
    a.base = first_trial + done;
    a.k = (int)std::min<int64_t>(K, count - done);
    const size_t k = (size_t)a.k, o = (size_t)done;
    launch_fsplit_fit_score(a, r->tile, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(pst.data(), r->d_pst.get(), sizeof(int32_t) * k * P, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(draws + 8 * o, r->d_draws.get(), sizeof(int32_t) * 8 * k, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(F + 9 * P * o, r->d_F.get(), sizeof(double) * 9 * P * k, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cnt + o, r->d_cnt.get(), sizeof(uint32_t) * k, hipMemcpyDeviceToHost));
    for (size_t t = 0; t < k; ++t) {  // a trial succeeds when every pair's fit does
      int32_t ok = 1;
      for (size_t p = 0; p < P; ++p) ok &= pst[t * P + p];
      status[o + t] = ok;
    }
  }
  return ICTR_OK;
}
