// ictr_camransac.hip -- "RANSAC camera estimation ... for whole sequence, check right for consistency"
// (misc_src/run_test_OF_track.py, TODO 1) on the device: RANSAC over P3P poses of the F frames of a track window, every
// trial scored by the points that reproject within the threshold in every frame and in both cameras.
//
// k_cr_flags runs once per run; the trials then run in chunks of K, all enqueued on one stream with no host wait in
// between:
//
//   k_cr_flags   one lane per point: does it count (cr_counts); one 64-bit word per wave by ballot, stored by lane 0.
//   k_cr_hyp     one lane per (trial, frame): the trial's 4 distinct point indices from the counter-based stream (every
//                lane of a trial draws the same), the counts test of the drawn points, the frame's hypothesis
//                (p3p_hypothesis on the left observations) -> G [12] and a per-frame status; twelve NaN where there is
//                none, so a failed trial scores nothing by arithmetic alone.
//   k_cr_score   a workgroup holds a tile of T trials x 240 / T frames of poses in LDS, one lane per point: X is read
//                once, per frame the 2 S observation coordinates are read once and serve all T trials, a running maximum
//                of rx^2 + ry^2 per trial stays in registers; after the last frame tile one root and one ballot per trial,
//                popcounts summed in LDS, one integer atomic per trial and workgroup. No inlier words are written.
//   k_cr_select  one workgroup: the chunk's largest count among the successful trials (lowest trial on ties) against the
//                best of the chunks before (strictly greater wins); the winner's poses and draws are copied next to the
//                state.
//   k_cr_mask    after the last chunk, for the winner only: distances and inlier words, with the device functions of the
//                score kernel (the same bits by construction). Without a winner the poses are NaN and so is every distance.
//
// Every result is decided by integers and fixed-order f64 arithmetic (ictr_camransac_hd.h): the same bits on every run,
// for every K and every T.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "ictr_camransac_hd.h"
#include "ictr_dev.h"
#include "ictr_launch.h"
#include "ictr_wininputs.h"

namespace ictr {

struct CrArgs {
  const double *X;                    // [3][n]
  const double *xy;                   // [S][F][2][n]
  const unsigned long long *mask;     // [nwords] or NULL: every point
  unsigned long long *cw;             // [nwords] the counts words
  int n, nwords, nframes, nsides;
  CfCam cam;
  double off[3];                      // o_1
  double thr;
  unsigned long long seedmix;
  long long base;                     // first trial of the chunk
  int k, init;                        // trials in the chunk; k_cr_flags: reset the state
  double *G;                          // [K][F][12]
  int *draws, *fst, *status;          // [K][4], [K][F], [K]
  unsigned *cnt;                      // [K]
  CrState *st;                        // the best trial so far ...
  double *o_G;                        // ... its poses [F][12]
  unsigned long long *o_words;        // [nwords] its inlier bits
  double *o_dd;                       // [n] its distances
};

__global__ void __launch_bounds__(kCrScoreBlock) k_cr_flags(CrArgs a) {
  const size_t n = (size_t)a.n, m = (size_t)blockIdx.x * kCrScoreBlock + threadIdx.x;
  const bool in = m < n;
  const size_t mm = in ? m : n - 1;
  const bool bit = a.mask ? cr_bit(a.mask, (long long)mm) : true;
  const bool ok = in && cr_counts(bit, a.X, a.xy, (long long)n, a.nframes, a.nsides, (long long)mm);
  const unsigned long long w = __ballot(ok);
  if ((threadIdx.x & 63) == 0 && in) a.cw[m >> 6] = w;
  if (a.init && m == 0) {
    a.st->best_trial = -1;
    a.st->best_count = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) a.st->draws[q] = -1;
    a.st->found = 0;
    a.st->pad_ = 0;
  }
}

__global__ void __launch_bounds__(kCrHypBlock) k_cr_hyp(CrArgs a) {
  const long long g = (long long)blockIdx.x * kCrHypBlock + threadIdx.x;
  if (g >= (long long)a.k * a.nframes) return;
  const int i = (int)(g / a.nframes), f = (int)(g - (long long)i * a.nframes);
  int idx[4];
  const bool drawn = cr_draw(a.seedmix, a.base + i, a.n, a.cw, idx);
  if (f == 0) {
    a.cnt[i] = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) a.draws[(size_t)i * 4 + q] = idx[q];
  }
  double G[12];
  bool ok = false;
  if (drawn) {
    ok = cr_hyp(idx, a.X, a.xy + (size_t)f * 2 * (size_t)a.n, (long long)a.n, a.cam, G);
  } else {
#pragma unroll
    for (int q = 0; q < 12; ++q) G[q] = cf_nan();
  }
  double *o = a.G + (size_t)g * 12;
#pragma unroll
  for (int q = 0; q < 12; ++q) o[q] = G[q];
  a.fst[g] = ok ? 1 : 0;
}

template <int TH>
__global__ void __launch_bounds__(kCrScoreBlock) k_cr_score(CrArgs a) {
  constexpr int FT = kCrTilePoses / TH;  // frames per LDS tile
  __shared__ double sG[TH * FT * 12];
  __shared__ int sOk[TH];
  __shared__ unsigned sCnt[TH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h0 = blockIdx.x * TH, F = a.nframes, n = a.n;
  if (tid < TH) {
    int ok = h0 + tid < a.k ? 1 : 0;
    if (ok)
      for (int f = 0; f < F; ++f) ok &= a.fst[(size_t)(h0 + tid) * F + f];
    sOk[tid] = ok;
    sCnt[tid] = 0u;
    if (blockIdx.y == 0 && h0 + tid < a.k) a.status[h0 + tid] = ok;
  }
  const int j = blockIdx.y * (kCrScoreBlock / 64) + wave;  // the wave's 64-point block
  const bool live = j < a.nwords;
  const int m = j * 64 + lane;
  const bool in = live && m < n;
  const size_t mm = (size_t)(in ? m : n - 1), N = (size_t)n;
  const double X = a.X[mm], Y = a.X[N + mm], Z = a.X[2 * N + mm];
  const bool two = a.nsides == 2;
  const double o0[3] = {0.0, 0.0, 0.0}, o1[3] = {a.off[0], a.off[1], a.off[2]};
  const CfCam cam = a.cam;
  double mx[TH];
#pragma unroll
  for (int h = 0; h < TH; ++h) mx[h] = -1.0;
  for (int f0 = 0; f0 < F; f0 += FT) {
    const int ft = min(FT, F - f0);
    __syncthreads();  // the tile before has been used (first pass: sOk is complete)
    for (int q = tid; q < TH * ft * 12; q += kCrScoreBlock) {
      const int h = q / (ft * 12), r = q - h * (ft * 12);
      sG[h * (FT * 12) + r] = h0 + h < a.k ? a.G[((size_t)(h0 + h) * F + f0) * 12 + r] : 0.0;
    }
    __syncthreads();
    if (live) {
      for (int ff = 0; ff < ft; ++ff) {
        const double *b0 = a.xy + (size_t)(f0 + ff) * 2 * N;
        const double *b1 = a.xy + (size_t)((two ? F : 0) + f0 + ff) * 2 * N;
        const double xl = b0[mm], yl = b0[N + mm], xr = b1[mm], yr = b1[N + mm];
#pragma unroll
        for (int h = 0; h < TH; ++h) {
          if (!sOk[h]) continue;
          const double *G = &sG[(h * FT + ff) * 12];
          mx[h] = cr_max(mx[h], cr_sq(G, o0, cam, X, Y, Z, xl, yl));
          if (two) mx[h] = cr_max(mx[h], cr_sq(G, o1, cam, X, Y, Z, xr, yr));
        }
      }
    }
  }
  if (live) {
    const double thr = a.thr;
    const bool cb = in && ((a.cw[j] >> lane) & 1ull) != 0;
#pragma unroll
    for (int h = 0; h < TH; ++h) {
      if (!sOk[h]) continue;
      const unsigned long long bits = __ballot(cb && cr_dist(mx[h]) < thr);
      if (lane == 0 && bits) atomicAdd(&sCnt[h], (unsigned)__popcll(bits));
    }
  }
  __syncthreads();
  if (tid < TH && sOk[tid] && sCnt[tid]) atomicAdd(&a.cnt[h0 + tid], sCnt[tid]);
}

__global__ void __launch_bounds__(kCrSelBlock) k_cr_select(CrArgs a) {
  __shared__ unsigned long long sKey[kCrSelBlock / 64];
  __shared__ int sWin;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // key of a successful trial: count + 1 in the high word, ~index in the low one: the largest key is the largest count at
  // the lowest index; 0: no trial of the chunk succeeded
  unsigned long long key = 0ull;
  for (int i = tid; i < a.k; i += kCrSelBlock) {
    if (!a.status[i]) continue;
    const unsigned long long c =
        (((unsigned long long)a.cnt[i] + 1ull) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
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
    for (int w = 1; w < kCrSelBlock / 64; ++w) key = sKey[w] > key ? sKey[w] : key;
    int win = -1;
    if (key != 0ull) {
      const int idx = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
      const long long c = (long long)(key >> 32) - 1;
      if (!a.st->found || c > a.st->best_count) {  // strictly more: the earlier trial keeps a tie
        a.st->best_trial = a.base + idx;
        a.st->best_count = c;
        a.st->found = 1;
        win = idx;
      }
    }
    sWin = win;
  }
  __syncthreads();
  const int win = sWin;
  if (win < 0) return;
  for (int q = tid; q < a.nframes * 12; q += kCrSelBlock) a.o_G[q] = a.G[(size_t)win * a.nframes * 12 + q];
  if (tid < 4) a.st->draws[tid] = a.draws[(size_t)win * 4 + tid];
}

__global__ void __launch_bounds__(kCrScoreBlock) k_cr_mask(CrArgs a) {
  __shared__ double sG[kCrMaxFrames * 12];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int F = a.nframes, n = a.n;
  const bool won = a.st->found != 0;
  for (int q = tid; q < F * 12; q += kCrScoreBlock) {
    sG[q] = won ? a.o_G[q] : cf_nan();
    if (!won && blockIdx.x == 0) a.o_G[q] = cf_nan();
  }
  __syncthreads();
  const int j = blockIdx.x * (kCrScoreBlock / 64) + wave;
  if (j >= a.nwords) return;
  const int m = j * 64 + lane;
  const bool in = m < n;
  const size_t mm = (size_t)(in ? m : n - 1), N = (size_t)n;
  const double X = a.X[mm], Y = a.X[N + mm], Z = a.X[2 * N + mm];
  const double o0[3] = {0.0, 0.0, 0.0}, o1[3] = {a.off[0], a.off[1], a.off[2]};
  double mx = -1.0;
  for (int f = 0; f < F; ++f) {
    const double *b0 = a.xy + (size_t)f * 2 * N;
    mx = cr_max(mx, cr_sq(&sG[f * 12], o0, a.cam, X, Y, Z, b0[mm], b0[N + mm]));
    if (a.nsides == 2) {
      const double *b1 = a.xy + (size_t)(F + f) * 2 * N;
      mx = cr_max(mx, cr_sq(&sG[f * 12], o1, a.cam, X, Y, Z, b1[mm], b1[N + mm]));
    }
  }
  const double d = cr_dist(mx);
  if (in) a.o_dd[m] = d;
  const bool cb = in && ((a.cw[j] >> lane) & 1ull) != 0;
  const unsigned long long bits = __ballot(cb && d < a.thr);
  if (lane == 0) a.o_words[j] = bits;
}

// the counts words (and, with a.init, the state before the first chunk)
static void launch_cr_flags(const CrArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_cr_flags, dim3((unsigned)((a.n + kCrScoreBlock - 1) / kCrScoreBlock)), dim3(kCrScoreBlock), 0, s, a);
}

// the hypotheses and scores of one chunk: the launch geometry of k_cr_hyp and k_cr_score<tile>, stated once for the run
// and the inspection entry (ictr_debug_camransac_trials). after_hyp (optional, timing runs): recorded between the two.
static void launch_cr_hyp_score(const CrArgs &a, int tile, hipStream_t s, hipEvent_t after_hyp = nullptr) {
  const long long fits = (long long)a.k * a.nframes;
  hipLaunchKernelGGL(k_cr_hyp, dim3((unsigned)((fits + kCrHypBlock - 1) / kCrHypBlock)), dim3(kCrHypBlock), 0, s, a);
  if (after_hyp) (void)hipEventRecord(after_hyp, s);
  const int segs = ran_segs(a.nwords, kCrScoreBlock);
  if (tile == 16)
    hipLaunchKernelGGL(k_cr_score<16>, dim3((a.k + 15) / 16, segs), dim3(kCrScoreBlock), 0, s, a);
  else if (tile == 64)
    hipLaunchKernelGGL(k_cr_score<64>, dim3((a.k + 63) / 64, segs), dim3(kCrScoreBlock), 0, s, a);
  else
    hipLaunchKernelGGL(k_cr_score<32>, dim3((a.k + 31) / 32, segs), dim3(kCrScoreBlock), 0, s, a);
}

static void launch_cr_select(const CrArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_cr_select, dim3(1), dim3(kCrSelBlock), 0, s, a);
}

static void launch_cr_mask(const CrArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_cr_mask, dim3(ran_segs(a.nwords, kCrScoreBlock)), dim3(kCrScoreBlock), 0, s, a);
}

}  // namespace ictr

using namespace ictr;

// ---------------------------------------------------------------- host side
struct ictr_camransac {
  WinInputs in;  // in.words: the mask words as set
  int chunk = 0, tile = 32;
  DevBuf<double> d_G;
  DevBuf<unsigned long long> d_cw;
  DevBuf<int> d_draws, d_fst, d_status;
  DevBuf<unsigned> d_cnt;
  bool timing = false, timed = false;  // timed: the run in flight (or last waited) carries events
  std::vector<Event> tev;              // before flags, after flags, per chunk after hyp / score / select, after mask
  float ms[4] = {0, 0, 0, 0};
  // (cr_layout) declared last, so destroyed first: a run in flight ends before a buffer or a timing event goes
  Readback out;
};

struct CrLayout {  // CrState | G [F][12] | words [nwords] | dd [n], each on a 16-byte boundary
  Part G, words, dd, end;  // end: empty, at the block's size
};
static CrLayout cr_layout(const ictr_camransac *r) {
  Carve c;
  c.take(sizeof(CrState), 16);  // at the front
  return {c.take(96 * (size_t)r->in.nframes, 16), c.take(8 * (size_t)r->in.nwords, 16), c.take(8 * (size_t)r->in.n, 16),
          c.take(0, 16)};  // braces: evaluated in this order
}

extern "C" int ictr_camransac_create(ictr_camransac **out, int64_t n, int64_t nframes, int64_t nsides) {
  if (!out) return fail(ICTR_ERR_INVALID, "camransac_create: NULL argument");
  if (n < 4 || n > ((int64_t)1 << 22))
    return fail(ICTR_ERR_INVALID, "camransac_create: %lld points (4 .. 2^22)", (long long)n);
  if (nframes < 1 || nframes > kCrMaxFrames)
    return fail(ICTR_ERR_INVALID, "camransac_create: %lld frames (1 .. %d)", (long long)nframes, kCrMaxFrames);
  if (nsides < 1 || nsides > 2) return fail(ICTR_ERR_INVALID, "camransac_create: %lld sides (1 or 2)", (long long)nsides);
  if (int rc = need_device()) return rc;
  auto r = std::make_unique<ictr_camransac>();
  if (int rc = r->in.alloc((int)n, (int)nframes, (int)nsides)) return rc;
  // trials per chunk: at the default the poses of a chunk (K x F x 96 B) stay below 26 MB; ICTR_CAMRANSAC_CHUNK
  // overrides (tests and sweeps; up to 65536, whose poses are allocated as asked: 400 MB at F = 64)
  const int chunk = env_int("ICTR_CAMRANSAC_CHUNK", 0);
  r->chunk = chunk > 0 ? std::min(chunk, 1 << 16) : 4096;
  r->tile = ran_tile_env("ICTR_CAMRANSAC_TILE");
  const size_t K = (size_t)r->chunk, F = (size_t)nframes;
  if (int rc = r->d_G.alloc(sizeof(double) * 12 * K * F, true)) return rc;
  if (int rc = r->d_cw.alloc(sizeof(unsigned long long) * (size_t)r->in.nwords, true)) return rc;
  if (int rc = r->d_draws.alloc(sizeof(int) * 4 * K, true)) return rc;
  if (int rc = r->d_fst.alloc(sizeof(int) * K * F, true)) return rc;
  if (int rc = r->d_status.alloc(sizeof(int) * K, true)) return rc;
  if (int rc = r->d_cnt.alloc(sizeof(unsigned) * K, true)) return rc;
  if (int rc = r->out.reserve(cr_layout(r.get()).end.at, true)) return rc;
  *out = r.release();
  return ICTR_OK;
}

extern "C" void ictr_camransac_destroy(ictr_camransac *r) { delete r; }

extern "C" int ictr_camransac_chunk_size(const ictr_camransac *r) { return r ? r->chunk : 0; }

extern "C" int ictr_camransac_set_points(ictr_camransac *r, const double *X) {
  return r ? r->in.set_points("camransac_set_points", "camransac", r->out, X) : null_object("camransac_set_points");
}
extern "C" int ictr_camransac_set_observations(ictr_camransac *r, const double *xy) {
  return r ? r->in.set_observations("camransac_set_observations", "camransac", r->out, xy)
           : null_object("camransac_set_observations");
}
extern "C" int ictr_camransac_set_mask(ictr_camransac *r, const uint64_t *words) {
  return r ? r->in.set_mask("camransac_set_mask", "camransac", r->out, words) : fail(ICTR_ERR_INVALID, "camransac is NULL");
}
extern "C" int ictr_camransac_set_camera(ictr_camransac *r, const double *fc, const double *cc) {
  return r ? r->in.set_camera("camransac_set_camera", "camransac", r->out, fc, cc) : null_object("camransac_set_camera");
}
extern "C" int ictr_camransac_set_offset(ictr_camransac *r, const double *offset) {
  return r ? r->in.set_offset("camransac_set_offset", "camransac", r->out, offset) : null_object("camransac_set_offset");
}

extern "C" int ictr_camransac_inputs_(ictr_camransac *r, WinDest *d) {
  *d = {&r->in, &r->out, "camransac", "RANSAC"};
  return ICTR_OK;
}

// the winner's inlier bits of the last run, in the result block on the device
extern "C" int ictr_camransac_mask_(const ictr_camransac *r, WinMaskSrc *m) {
  *m = {reinterpret_cast<const unsigned long long *>(r->out.dev() + cr_layout(r).words.at), r->in.n, r->out.ran(), "RANSAC"};
  return ICTR_OK;
}

extern "C" int ictr_camransac_set_timing(ictr_camransac *r, int on) {
  if (!r) return fail(ICTR_ERR_INVALID, "camransac is NULL");
  if (int rc = r->out.refuse("camransac_set_timing", "camransac")) return rc;
  r->timing = on != 0;
  return ICTR_OK;
}

// what every entry that launches needs first, and every field of the kernels' argument block that does not depend on the
// trial range
static int cr_fill_args(const ictr_camransac *r, const char *what, double thresh, uint64_t seed, CrArgs &a) {
  if (int rc = r->in.ready(what, r->out, "camransac")) return rc;
  if (std::isnan(thresh)) return fail(ICTR_ERR_INVALID, "%s: thresh is NaN", what);
  const CrLayout L = cr_layout(r);
  memset(&a, 0, sizeof(a));
  a.X = r->in.X.get();
  a.xy = r->in.xy.get();
  a.mask = r->in.mask_or_null();
  a.cw = r->d_cw.get();
  a.n = r->in.n;
  a.nwords = r->in.nwords;
  a.nframes = r->in.nframes;
  a.nsides = r->in.nsides;
  a.cam = r->in.cam;
  for (int q = 0; q < 3; ++q) a.off[q] = r->in.nsides == 2 ? r->in.off[q] : 0.0;
  a.thr = thresh;
  a.seedmix = ran_seed(seed);
  a.G = r->d_G.get();
  a.draws = r->d_draws.get();
  a.fst = r->d_fst.get();
  a.status = r->d_status.get();
  a.cnt = r->d_cnt.get();
  a.st = reinterpret_cast<CrState *>(r->out.dev());
  a.o_G = reinterpret_cast<double *>(r->out.dev() + L.G.at);
  a.o_words = reinterpret_cast<unsigned long long *>(r->out.dev() + L.words.at);
  a.o_dd = reinterpret_cast<double *>(r->out.dev() + L.dd.at);
  return ICTR_OK;
}

extern "C" int ictr_camransac_run(ictr_camransac *r, int64_t ntrials, double thresh, uint64_t seed, void *hip_stream) {
  if (!r) return fail(ICTR_ERR_INVALID, "camransac is NULL");
  if (ntrials < 1 || ntrials > ((int64_t)1 << 20))
    return fail(ICTR_ERR_INVALID, "camransac_run: ntrials %lld (1 .. 2^20)", (long long)ntrials);
  CrArgs a;
  if (int rc = cr_fill_args(r, "camransac_run", thresh, seed, a)) return rc;
  const int64_t K = r->chunk;
  const int64_t nchunks = (ntrials + K - 1) / K;
  std::vector<Event> tev;
  if (r->timing) {
    tev.resize((size_t)nchunks * 3 + 3);
    for (Event &e : tev)
      if (int rc = e.create()) return rc;
  }
  hipStream_t s = (hipStream_t)hip_stream;
  size_t e = 0;
  if (r->timing) HIPCHK(hipEventRecord(tev[e++].get(), s));
  a.init = 1;
  launch_cr_flags(a, s);
  a.init = 0;
  if (r->timing) HIPCHK(hipEventRecord(tev[e++].get(), s));
  for (int64_t c = 0; c < nchunks; ++c) {
    a.base = c * K;
    a.k = (int)std::min<int64_t>(K, ntrials - a.base);
    launch_cr_hyp_score(a, r->tile, s, r->timing ? tev[e++].get() : nullptr);
    if (r->timing) HIPCHK(hipEventRecord(tev[e++].get(), s));
    launch_cr_select(a, s);
    if (r->timing) HIPCHK(hipEventRecord(tev[e++].get(), s));
    HIPCHK(hipGetLastError());
  }
  launch_cr_mask(a, s);
  HIPCHK(hipGetLastError());
  if (r->timing) HIPCHK(hipEventRecord(tev[e++].get(), s));
  if (int rc = r->out.post(cr_layout(r).end.at, s)) return rc;
  r->tev = std::move(tev);
  r->timed = r->timing;
  return ICTR_OK;
}

extern "C" int ictr_camransac_wait(ictr_camransac *r, int64_t *best_trial, int64_t *best_count, int32_t *draws, double *G,
                                   double *p, uint64_t *inl_words, double *dd) {
  if (!r) return fail(ICTR_ERR_INVALID, "camransac is NULL");
  if (!r->out.pending()) return fail(ICTR_ERR_STATE, "camransac_wait: nothing has been run");
  if (int rc = r->out.wait()) return rc;
  const CrLayout L = cr_layout(r);
  const CrState &st = *reinterpret_cast<const CrState *>(r->out.host());
  const double *hG = reinterpret_cast<const double *>(r->out.host() + L.G.at);
  if (best_trial) *best_trial = st.best_trial;
  if (best_count) *best_count = st.best_count;
  if (draws) memcpy(draws, st.draws, sizeof(st.draws));
  if (G) memcpy(G, hG, L.G.bytes);
  if (p)  // p = se3_log(G), on the host at the read-back (as ictr_ransac_wait); NaN without a winner
    for (int f = 0; f < r->in.nframes; ++f) {
      if (st.found) {
        se3_log<double>(p + 6 * f, hG + 12 * f);
      } else {
        for (int q = 0; q < 6; ++q) p[6 * f + q] = cf_nan();
      }
    }
  if (inl_words) memcpy(inl_words, r->out.host() + L.words.at, L.words.bytes);
  if (dd) memcpy(dd, r->out.host() + L.dd.at, L.dd.bytes);
  if (r->timed) {
    float ms[4] = {0, 0, 0, 0};
    for (size_t k = 0; k + 1 < r->tev.size(); ++k) {
      float t = 0;
      HIPCHK(hipEventElapsedTime(&t, r->tev[k].get(), r->tev[k + 1].get()));
      ms[(k == 0 || k + 2 == r->tev.size()) ? 3 : (k - 1) % 3] += t;
    }
    memcpy(r->ms, ms, sizeof(ms));
    r->tev.clear();
  }
  return ICTR_OK;
}

extern "C" int ictr_camransac_get_kernel_times(const ictr_camransac *r, float *ms) {
  if (!r || !ms) return fail(ICTR_ERR_INVALID, "camransac_get_kernel_times: NULL argument");
  if (r->out.pending() || !r->timed) return fail(ICTR_ERR_STATE, "camransac_get_kernel_times: no completed timed run");
  memcpy(ms, r->ms, sizeof(r->ms));
  return ICTR_OK;
}

// inspection: hypotheses and scores of trials [first_trial, first_trial + count), in the object's own chunks and tile, on
// the null stream. No select runs: the object's best trial is left alone.
extern "C" int ictr_debug_camransac_trials(ictr_camransac *r, double thresh, uint64_t seed, int64_t first_trial,
                                           int64_t count, int32_t *status, int32_t *draws, double *G, uint32_t *cnt) {
  if (!r || !status || !draws || !G || !cnt) return fail(ICTR_ERR_INVALID, "debug_camransac_trials: NULL argument");
  if (count < 1 || count > ((int64_t)1 << 20) || first_trial < 0 || first_trial > ((int64_t)1 << 20) - count)
    return fail(ICTR_ERR_INVALID, "debug_camransac_trials: trials %lld + %lld (1 .. 2^20 trials below 2^20)",
                (long long)first_trial, (long long)count);
  CrArgs a;
  if (int rc = cr_fill_args(r, "debug_camransac_trials", thresh, seed, a)) return rc;
  launch_cr_flags(a, nullptr);
  const int64_t K = r->chunk;
  const size_t F = (size_t)r->in.nframes;
  for (int64_t done = 0; done < count; done += K) {
    a.base = first_trial + done;
    a.k = (int)std::min<int64_t>(K, count - done);
    const size_t k = (size_t)a.k, o = (size_t)done;
    launch_cr_hyp_score(a, r->tile, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(status + o, r->d_status.get(), sizeof(int32_t) * k, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(draws + 4 * o, r->d_draws.get(), sizeof(int32_t) * 4 * k, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(G + 12 * F * o, r->d_G.get(), sizeof(double) * 12 * F * k, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cnt + o, r->d_cnt.get(), sizeof(uint32_t) * k, hipMemcpyDeviceToHost));
  }
  return ICTR_OK;
}
