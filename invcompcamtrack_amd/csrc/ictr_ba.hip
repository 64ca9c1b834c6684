// ictr_ba.hip -- "BA Adjust cameras and static points" (item 3 of the list that ends misc_src/run_test_OF_track.py) on the
// device: the poses of frames 1 .. F - 1 and the adjusted points of a track window moved together by Levenberg-Marquardt
// through the Schur complement of the points.
//
// A run is 2 + 7 (noiter + 1) launches on one stream with no host wait in between: k_ba_flags, then noiter + 1 rounds of
// point, frames, decide, schur, gather, solve, back, then k_ba_final. The points live in two sets (X, V, gp): the accepted
// one and the trial one; accepting a step swaps their roles in BaState.
//
//   k_ba_flags   one lane per point: is it adjusted (one 64-bit word per wave by ballot), and the point as set into the
//                first trial set.
//   k_ba_point   one lane per point of the trial set over all frames and sides: V (6) and gp (3) into planes.
//   k_ba_frames  grid (chunks of kCfChunk points, frames) at the trial set: the 28 terms of ba_add_cam summed with
//                k_camfit_pass's reduction; partials per chunk and frame.
//   k_ba_decide  one workgroup: the chunk partials in chunk order, then one lane runs ba_decide (cost, accept test, stops).
//   k_ba_schur   grid (chunks, block pairs f <= g) at the accepted set: per point the 3 x 3 factors from the V plane, W_f
//                and W_g recomputed from pose, point and observations, the 42 terms of ba_pair_terms, same reduction.
//   k_ba_gather  one wave per block pair: the chunk partials in chunk order.
//   k_ba_solve   one workgroup: assembles the reduced system's upper triangle, factors it column by column (one lane per
//                entry of the column; in LDS up to kBaLdsDim unknowns, in device memory above), one lane substitutes and
//                runs ba_solved (trial poses, or the damping raised).
//   k_ba_back    one lane per point: the trial set's points from the accepted set's and the step.
//   k_ba_final   the accepted points into the buffer that ictr_ba_wait reads.
//
// A round whose run has stopped returns at once. Every result is fixed-order f64 arithmetic (ictr_ba_hd.h): the same bits
// on every run and every device.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <memory>
#include <vector>

#include "ictr_ba_hd.h"
#include "ictr_dev.h"
#include "ictr_launch.h"
#include "ictr_wininputs.h"

namespace ictr {

constexpr int kBaBlock = 256;
constexpr int kBaKinds = 7;
constexpr int kBaMaxIter = 1000;
constexpr int kBaLdsTri = kBaLdsDim * (kBaLdsDim + 1) / 2;

struct BaArgs {
  const double *xy;                 // [S][F][2][n]
  const unsigned long long *words;  // [ceil(n / 64)] inlier bits, or NULL: every point
  unsigned long long *adjw;         // [ceil(n / 64)] adjusted bits
  const double *Xin;                // [3][n] the points as set
  double *X[2], *V[2], *gp[2];      // the two point sets: [3][n], [6][n], [3][n]
  double *Xout;                     // [3][n]
  int n, nwords, nchunks, nframes, nsides, npairs, debug;
  CfCam cam;
  CfParams prm;
  double off[2][3];
  double *fpart;  // [F][nchunks][kCfSlots]
  double *ppart;  // [npairs][nchunks][kBaPairSlots]
  double *fsums;  // [F][kCfSlots]
  double *T;      // [npairs][kBaPairSlots]
  double *A;      // the packed upper triangle as assembled, factored in place above kBaLdsDim unknowns
  double *rhs;    // [6 (F - 1)]
  BaState *st;
};

// one of the two sets by a run-time index, without indexing the kernel arguments
template <class T>
__device__ __forceinline__ T *ba_set(T *const (&p)[2], int e) {
  return e ? p[1] : p[0];
}
__device__ __forceinline__ bool ba_bit(const unsigned long long *w, size_t m) { return ((w[m >> 6] >> (m & 63)) & 1ull) != 0; }

// one observation of point m: frame f, side s at the poses G
__device__ __forceinline__ void ba_obs_at(const BaArgs &a, const double *G, int f, int s, double X, double Y, double Z,
                                          size_t m, BaObs &b) {
  const size_t n = (size_t)a.n;
  const double *o = a.xy + ((size_t)s * a.nframes + f) * 2 * n;
  const double off[3] = {s ? a.off[1][0] : 0.0, s ? a.off[1][1] : 0.0, s ? a.off[1][2] : 0.0};
  ba_obs(G + 12 * f, off, a.cam, X, Y, Z, o[m], o[n + m], b);
}

__device__ __forceinline__ void ba_w_at(const BaArgs &a, const double *G, int f, double X, double Y, double Z, size_t m,
                                        double *W) {
#pragma unroll
  for (int q = 0; q < 18; ++q) W[q] = 0.0;
  for (int s = 0; s < a.nsides; ++s) {
    BaObs b;
    ba_obs_at(a, G, f, s, X, Y, Z, m, b);
    ba_add_w(b, W);
  }
}

__global__ void __launch_bounds__(kBaBlock) k_ba_flags(BaArgs a) {
  const size_t n = (size_t)a.n, m = (size_t)blockIdx.x * kBaBlock + threadIdx.x;
  const bool in = m < n;
  const size_t mm = in ? m : n - 1;
  const bool bit = a.words ? ba_bit(a.words, mm) : true;
  const bool ok = in && ba_adjusted(bit, a.Xin, a.xy, (long long)n, a.nframes, a.nsides, (long long)mm);
  const unsigned long long w = __ballot(ok);
  if ((threadIdx.x & 63) == 0 && in) a.adjw[m >> 6] = w;
  if (in) {  // the run starts from the points as set, whatever an earlier run left in the sets
    double *X = ba_set(a.X, a.st->tset);
#pragma unroll
    for (int q = 0; q < 3; ++q) X[(size_t)q * n + m] = a.Xin[(size_t)q * n + m];
  }
}

__global__ void __launch_bounds__(kBaBlock) k_ba_point(BaArgs a) {
  const BaState *st = a.st;
  if (!a.debug && (st->status != kCfRunning || st->phase == kBaRetry)) return;
  const size_t n = (size_t)a.n, m = (size_t)blockIdx.x * kBaBlock + threadIdx.x;
  if (m >= n) return;
  const int e = st->tset;
  const double *Xe = ba_set(a.X, e);
  double *Ve = ba_set(a.V, e), *ge = ba_set(a.gp, e);
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
  if (ba_bit(a.adjw, m)) {
    const double X = Xe[m], Y = Xe[n + m], Z = Xe[2 * n + m];
    for (int f = 0; f < a.nframes; ++f)
      for (int s = 0; s < a.nsides; ++s) {
        BaObs b;
        ba_obs_at(a, st->Gt, f, s, X, Y, Z, m, b);
        ba_add_point(b, v, g);
      }
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) Ve[(size_t)q * n + m] = v[q];
#pragma unroll
  for (int q = 0; q < 3; ++q) ge[(size_t)q * n + m] = g[q];
}

// the lane values of NT terms through the pairwise tree: xor shuffles inside a wave, LDS across the four waves; the
// first NS lanes store the chunk's partial (slot `cslot`: cnt)
template <int NT, int NS>
__device__ __forceinline__ void ba_reduce_store(double *acc, int cnt, int cslot, double *out) {
  __shared__ double sW[kBaBlock / 64][NT];
  __shared__ int sC[kBaBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
  if (tid < NS) {
    double v = 0.0;
    if (tid < NT) v = (sW[0][tid] + sW[1][tid]) + (sW[2][tid] + sW[3][tid]);
    if (tid == cslot) v = (double)((sC[0] + sC[1]) + (sC[2] + sC[3]));
    out[tid] = v;
  }
}

__global__ void __launch_bounds__(kCfBlock) k_ba_frames(BaArgs a) {
  const BaState *st = a.st;
  if (!a.debug && (st->status != kCfRunning || st->phase == kBaRetry)) return;
  const int f = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x, e = st->tset;
  const size_t n = (size_t)a.n;
  const double *Xe = ba_set(a.X, e);
  double acc[kCfTerms];
#pragma unroll
  for (int q = 0; q < kCfTerms; ++q) acc[q] = 0.0;
  int cnt = 0;
#pragma unroll 1
  for (int r = 0; r < kCfPerLane; ++r) {
    const size_t m = (size_t)ch * kCfChunk + (size_t)r * kCfBlock + tid;
    if (m >= n || !ba_bit(a.adjw, m)) continue;  // exact zeros
    cnt += 1;
    const double X = Xe[m], Y = Xe[n + m], Z = Xe[2 * n + m];
    double t[kCfTerms];
#pragma unroll
    for (int q = 0; q < kCfTerms; ++q) t[q] = 0.0;
    for (int s = 0; s < a.nsides; ++s) {
      BaObs b;
      ba_obs_at(a, st->Gt, f, s, X, Y, Z, m, b);
      ba_add_cam(b, t);
    }
#pragma unroll
    for (int q = 0; q < kCfTerms; ++q) acc[q] = acc[q] + t[q];
  }
  ba_reduce_store<kCfTerms, kCfSlots>(acc, cnt, kCfCountSlot, a.fpart + ((size_t)f * a.nchunks + ch) * kCfSlots);
}

__global__ void __launch_bounds__(kBaBlock) k_ba_decide(BaArgs a) {
  __shared__ double sS[kBaMaxFrames * kCfSlots];
  BaState *st = a.st;
  if (!a.debug && (st->status != kCfRunning || st->phase == kBaRetry)) return;
  for (int i = threadIdx.x; i < a.nframes * kCfSlots; i += kBaBlock) {
    const int f = i / kCfSlots, t = i % kCfSlots;
    const double *p = a.fpart + (size_t)f * a.nchunks * kCfSlots + t;
    double acc = 0.0;
    for (int c = 0; c < a.nchunks; ++c) acc = acc + p[(size_t)c * kCfSlots];
    sS[i] = t < kCfTerms ? cf_canon(acc) : acc;
  }
  __syncthreads();
  if (a.debug) {  // the sums, n and the cost alone
    for (int i = threadIdx.x; i < a.nframes * kCfSlots; i += kBaBlock) {
      const int f = i / kCfSlots, t = i % kCfSlots;
      a.fsums[i] = sS[i];
      if (t < 21) st->U[21 * f + t] = sS[i];
      if (t >= 21 && t < 27) st->gc[6 * f + (t - 21)] = sS[i];
    }
    if (threadIdx.x == 0) {
      st->n = (long long)sS[kCfCountSlot];
      st->c = ba_cost(sS, a.nframes, a.nsides);
    }
    return;
  }
  if (threadIdx.x == 0) ba_decide(*st, sS, a.nframes, a.nsides, a.prm);
}

__global__ void __launch_bounds__(kCfBlock) k_ba_schur(BaArgs a) {
  const BaState *st = a.st;
  if (!a.debug && st->status != kCfRunning) return;
  const int ch = blockIdx.x, p = blockIdx.y, tid = threadIdx.x, e = a.debug ? st->tset : st->cur;
  const size_t n = (size_t)a.n;
  const double damp = st->damp;
  const double *Xe = ba_set(a.X, e), *Ve = ba_set(a.V, e), *ge = ba_set(a.gp, e);
  int f, g;
  ba_pair(a.nframes, p, f, g);
  double acc[kBaPairTerms];
#pragma unroll
  for (int q = 0; q < kBaPairTerms; ++q) acc[q] = 0.0;
  int fails = 0;
#pragma unroll 1
  for (int r = 0; r < kCfPerLane; ++r) {
    const size_t m = (size_t)ch * kCfChunk + (size_t)r * kCfBlock + tid;
    if (m >= n || !ba_bit(a.adjw, m)) continue;  // exact zeros
    const double X = Xe[m], Y = Xe[n + m], Z = Xe[2 * n + m];
    double v[6], gq[3], L[3], D[3], Wf[18], Wg[18], t[kBaPairTerms];
#pragma unroll
    for (int q = 0; q < 6; ++q) v[q] = Ve[(size_t)q * n + m];
#pragma unroll
    for (int q = 0; q < 3; ++q) gq[q] = ge[(size_t)q * n + m];
    fails += ba_factor3(v, damp, L, D) ? 0 : 1;
    ba_w_at(a, st->G, f, X, Y, Z, m, Wf);
    if (g != f) {
      ba_w_at(a, st->G, g, X, Y, Z, m, Wg);
    } else {
#pragma unroll
      for (int q = 0; q < 18; ++q) Wg[q] = Wf[q];
    }
    ba_pair_terms(Wf, Wg, L, D, gq, t);
#pragma unroll
    for (int q = 0; q < kBaPairTerms; ++q) acc[q] = acc[q] + t[q];
  }
  ba_reduce_store<kBaPairTerms, kBaPairSlots>(acc, fails, kBaFailSlot,
                                              a.ppart + ((size_t)p * a.nchunks + ch) * kBaPairSlots);
}

__global__ void __launch_bounds__(64) k_ba_gather(BaArgs a) {
  if (!a.debug && a.st->status != kCfRunning) return;
  const int p = blockIdx.x, t = threadIdx.x;
  if (t >= kBaPairSlots) return;
  const double *q = a.ppart + (size_t)p * a.nchunks * kBaPairSlots + t;
  double acc = 0.0;
  for (int c = 0; c < a.nchunks; ++c) acc = acc + q[(size_t)c * kBaPairSlots];
  a.T[(size_t)p * kBaPairSlots + t] = t < kBaPairTerms ? cf_canon(acc) : acc;
}

__global__ void __launch_bounds__(kBaBlock) k_ba_solve(BaArgs a) {
  __shared__ double sA[kBaLdsTri];
  __shared__ double sCol[kBaMaxDim], sX[kBaMaxDim];
  BaState *st = a.st;
  if (!a.debug && st->status != kCfRunning) return;
  const int tid = threadIdx.x, dim = 6 * (a.nframes - 1);
  double *A = (!a.debug && dim <= kBaLdsDim) ? sA : a.A;
  const double damp = st->damp;
  for (int I = 0; I < dim; ++I)
    for (int J = I + tid; J < dim; J += kBaBlock) A[ba_ridx(dim, I, J)] = ba_reduced_entry(st->U, a.T, a.nframes, damp, I, J);
  if (tid < dim) {
    const double b = ba_reduced_rhs(st->gc, a.T, a.nframes, tid);
    sX[tid] = b;
    if (a.debug) a.rhs[tid] = b;
  }
  if (a.debug) return;
  __syncthreads();
  bool ok = a.T[kBaFailSlot] == 0.0;
  const int i0 = tid;  // lane i0 owns row j + i0 of column j
  for (int j = 0; j < dim && ok; ++j) {
    const int i = j + i0;
    if (i < dim) sCol[i] = ba_ldl_sum(A, dim, j, i);
    __syncthreads();
    const double d = sCol[j];
    if (!ba_pivot_ok(d)) ok = false;  // the same d in every lane
    if (ok && i < dim) A[ba_ridx(dim, j, i)] = i == j ? d : sCol[i] / d;
    __syncthreads();
  }
  if (tid == 0) {
    if (ok) ba_ldl_solve(A, dim, sX, sX);
    ba_solved(*st, ok, sX, a.nframes, a.prm);
  }
}

__global__ void __launch_bounds__(kBaBlock) k_ba_back(BaArgs a) {
  const BaState *st = a.st;
  if (st->status != kCfRunning || st->phase != kBaTrial) return;
  const size_t n = (size_t)a.n, m = (size_t)blockIdx.x * kBaBlock + threadIdx.x;
  if (m >= n) return;
  const double *Xf = ba_set(a.X, st->cur), *Vf = ba_set(a.V, st->cur), *gf = ba_set(a.gp, st->cur);
  double *Xt = ba_set(a.X, st->tset);
  double x[3] = {Xf[m], Xf[n + m], Xf[2 * n + m]};
  if (ba_bit(a.adjw, m)) {
    double v[6], b[3], L[3], D[3], d[3];
#pragma unroll
    for (int q = 0; q < 6; ++q) v[q] = Vf[(size_t)q * n + m];
#pragma unroll
    for (int q = 0; q < 3; ++q) b[q] = gf[(size_t)q * n + m];
    ba_factor3(v, st->damp, L, D);
    for (int f = 1; f < a.nframes; ++f) {
      double W[18];
      ba_w_at(a, st->G, f, x[0], x[1], x[2], m, W);
      ba_back_rhs(W, st->dc + 6 * (f - 1), b);
    }
    ba_solve3(L, D, b, d);
#pragma unroll
    for (int q = 0; q < 3; ++q) x[q] = x[q] + d[q];
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) Xt[(size_t)q * n + m] = x[q];
}

__global__ void __launch_bounds__(kBaBlock) k_ba_final(BaArgs a) {
  const size_t i = (size_t)blockIdx.x * kBaBlock + threadIdx.x;
  if (i < 3 * (size_t)a.n) a.Xout[i] = ba_set(a.X, a.st->cur)[i];
}

static unsigned ba_grid(size_t items) { return (unsigned)((items + kBaBlock - 1) / kBaBlock); }

// kind 0 .. 6 of a round
static void launch_ba_kind(const BaArgs &a, int kind, hipStream_t s) {
  switch (kind) {
    case 0: hipLaunchKernelGGL(k_ba_point, dim3(ba_grid((size_t)a.n)), dim3(kBaBlock), 0, s, a); break;
    case 1: hipLaunchKernelGGL(k_ba_frames, dim3(a.nchunks, a.nframes), dim3(kCfBlock), 0, s, a); break;
    case 2: hipLaunchKernelGGL(k_ba_decide, dim3(1), dim3(kBaBlock), 0, s, a); break;
    case 3: hipLaunchKernelGGL(k_ba_schur, dim3(a.nchunks, a.npairs), dim3(kCfBlock), 0, s, a); break;
    case 4: hipLaunchKernelGGL(k_ba_gather, dim3(a.npairs), dim3(64), 0, s, a); break;
    case 5: hipLaunchKernelGGL(k_ba_solve, dim3(1), dim3(kBaBlock), 0, s, a); break;
    default: hipLaunchKernelGGL(k_ba_back, dim3(ba_grid((size_t)a.n)), dim3(kBaBlock), 0, s, a); break;
  }
}

}  // namespace ictr

using namespace ictr;

// ---------------------------------------------------------------- host side
struct ictr_ba {
  WinInputs in;  // in.X: the points as set
  int nchunks = 0, npairs = 0, dim = 0;
  DevBuf<double> d_X[2], d_V[2], d_gp[2], d_Xout, d_fpart, d_ppart, d_fsums, d_T, d_A, d_rhs;
  DevBuf<unsigned long long> d_adjw;
  PinBuf<char> up;  // the initial state of a run, uploaded on its stream
  bool timing = false, timed = false;  // timed: the run in flight (or last waited) carries events
  std::vector<Event> tev;              // one before every launch of a round and one after the last
  float ms[kBaKinds] = {0, 0, 0, 0, 0, 0, 0};
  // declared last, so destroyed first: a run in flight ends before a buffer or a timing event goes
  Readback out;  // BaState
};

extern "C" int ictr_ba_create(ictr_ba **out, int64_t n, int64_t nframes, int64_t nsides) {
  if (!out) return fail(ICTR_ERR_INVALID, "ba_create: NULL argument");
  if (n < 8 || n > ((int64_t)1 << 22)) return fail(ICTR_ERR_INVALID, "ba_create: %lld points (8 .. 2^22)", (long long)n);
  if (nframes < 2 || nframes > kBaMaxFrames)
    return fail(ICTR_ERR_INVALID, "ba_create: %lld frames (2 .. %d)", (long long)nframes, kBaMaxFrames);
  if (nsides < 1 || nsides > 2) return fail(ICTR_ERR_INVALID, "ba_create: %lld sides (1 or 2)", (long long)nsides);
  if (int rc = need_device()) return rc;
  auto r = std::make_unique<ictr_ba>();
  r->nchunks = (int)((n + kCfChunk - 1) / kCfChunk);
  r->npairs = ba_npairs((int)nframes);
  r->dim = 6 * ((int)nframes - 1);
  const size_t N = (size_t)n, F = (size_t)nframes, D = sizeof(double);
  if (int rc = r->in.alloc((int)n, (int)nframes, (int)nsides)) return rc;
  for (int e = 0; e < 2; ++e) {
    if (int rc = r->d_X[e].alloc(D * 3 * N, true)) return rc;
    if (int rc = r->d_V[e].alloc(D * 6 * N, true)) return rc;
    if (int rc = r->d_gp[e].alloc(D * 3 * N, true)) return rc;
  }
  if (int rc = r->d_Xout.alloc(D * 3 * N, true)) return rc;
  if (int rc = r->d_fpart.alloc(D * kCfSlots * F * (size_t)r->nchunks, true)) return rc;
  if (int rc = r->d_ppart.alloc(D * kBaPairSlots * (size_t)r->npairs * (size_t)r->nchunks, true)) return rc;
  if (int rc = r->d_fsums.alloc(D * kCfSlots * F, true)) return rc;
  if (int rc = r->d_T.alloc(D * kBaPairSlots * (size_t)r->npairs, true)) return rc;
  if (int rc = r->d_A.alloc(D * (size_t)(r->dim * (r->dim + 1) / 2), true)) return rc;
  if (int rc = r->d_rhs.alloc(D * (size_t)r->dim, true)) return rc;
  if (int rc = r->d_adjw.alloc(sizeof(unsigned long long) * (size_t)r->in.nwords, true)) return rc;
  if (int rc = r->up.alloc(sizeof(BaState))) return rc;
  if (int rc = r->out.reserve(sizeof(BaState), true)) return rc;
  *out = r.release();
  return ICTR_OK;
}

extern "C" void ictr_ba_destroy(ictr_ba *r) { delete r; }

extern "C" int ictr_ba_set_points(ictr_ba *r, const double *X) {
  return r ? r->in.set_points("ba_set_points", "ba", r->out, X) : null_object("ba_set_points");
}
extern "C" int ictr_ba_set_observations(ictr_ba *r, const double *xy) {
  return r ? r->in.set_observations("ba_set_observations", "ba", r->out, xy) : null_object("ba_set_observations");
}
extern "C" int ictr_ba_set_mask(ictr_ba *r, const uint64_t *words) {
  return r ? r->in.set_mask("ba_set_mask", "ba", r->out, words) : fail(ICTR_ERR_INVALID, "ba is NULL");
}
extern "C" int ictr_ba_set_camera(ictr_ba *r, const double *fc, const double *cc) {
  return r ? r->in.set_camera("ba_set_camera", "ba", r->out, fc, cc) : null_object("ba_set_camera");
}
extern "C" int ictr_ba_set_offset(ictr_ba *r, const double *offset) {
  return r ? r->in.set_offset("ba_set_offset", "ba", r->out, offset) : null_object("ba_set_offset");
}

extern "C" int ictr_ba_inputs_(ictr_ba *r, WinDest *d) {
  *d = {&r->in, &r->out, "ba", "adjuster"};
  return ICTR_OK;
}

extern "C" int ictr_ba_set_timing(ictr_ba *r, int on) {
  if (!r) return fail(ICTR_ERR_INVALID, "ba is NULL");
  if (int rc = r->out.refuse("ba_set_timing", "ba")) return rc;
  r->timing = on != 0;
  return ICTR_OK;
}

static void ba_fill_args(const ictr_ba *r, const CfParams &p, BaArgs &a) {
  memset(&a, 0, sizeof(a));
  a.xy = r->in.xy.get();
  a.words = r->in.mask_or_null();
  a.adjw = r->d_adjw.get();
  a.Xin = r->in.X.get();
  for (int e = 0; e < 2; ++e) {
    a.X[e] = r->d_X[e].get();
    a.V[e] = r->d_V[e].get();
    a.gp[e] = r->d_gp[e].get();
  }
  a.Xout = r->d_Xout.get();
  a.n = r->in.n;
  a.nwords = r->in.nwords;
  a.nchunks = r->nchunks;
  a.nframes = r->in.nframes;
  a.nsides = r->in.nsides;
  a.npairs = r->npairs;
  a.cam = r->in.cam;
  a.prm = p;
  for (int q = 0; q < 3; ++q) a.off[1][q] = r->in.off[q];
  a.fpart = r->d_fpart.get();
  a.ppart = r->d_ppart.get();
  a.fsums = r->d_fsums.get();
  a.T = r->d_T.get();
  a.A = r->d_A.get();
  a.rhs = r->d_rhs.get();
  a.st = reinterpret_cast<BaState *>(r->out.dev());
}

static int ba_poses_finite(const double *G, int nframes, const char *what) {
  for (int q = 0; q < 12 * nframes; ++q)
    if (!cf_finite(G[q])) return fail(ICTR_ERR_INVALID, "%s: a pose entry is not finite", what);
  return ICTR_OK;
}

extern "C" int ictr_ba_run(ictr_ba *r, const double *G0, int32_t noiter, double damp_init, double damp_fct, double minres,
                           double maxdamp, void *hip_stream) {
  if (!r || !G0) return fail(ICTR_ERR_INVALID, "ba_run: NULL argument");
  if (int rc = r->in.ready("ba_run", r->out, "ba")) return rc;
  if (noiter < 0 || noiter > kBaMaxIter) return fail(ICTR_ERR_INVALID, "ba_run: noiter %d (0 .. %d)", noiter, kBaMaxIter);
  if (!(damp_init > 0.0) || !cf_finite(damp_init) || !(damp_fct > 1.0) || !cf_finite(damp_fct) || !(minres >= 0.0) ||
      !cf_finite(minres) || !(maxdamp > 0.0))
    return fail(ICTR_ERR_INVALID, "ba_run: needs damp_init > 0, damp_fct > 1, minres >= 0 (all finite), maxdamp > 0");
  if (int rc = ba_poses_finite(G0, r->in.nframes, "ba_run")) return rc;
  const CfParams p = {noiter, damp_init, damp_fct, minres, maxdamp};
  BaArgs a;
  ba_fill_args(r, p, a);
  std::vector<Event> tev;
  if (r->timing) {
    tev.resize(1 + (size_t)kBaKinds * ((size_t)noiter + 1));
    for (Event &e : tev)
      if (int rc = e.create()) return rc;
  }
  ba_init(*reinterpret_cast<BaState *>(r->up.get()), G0, r->in.nframes, p);
  hipStream_t s = (hipStream_t)hip_stream;
  HIPCHK(hipMemcpyAsync(r->out.dev(), r->up.get(), sizeof(BaState), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_ba_flags, dim3(ba_grid((size_t)r->in.n)), dim3(kBaBlock), 0, s, a);
  size_t e = 0;
  for (int it = 0; it <= noiter; ++it) {
    for (int kind = 0; kind < kBaKinds; ++kind) {
      if (r->timing) HIPCHK(hipEventRecord(tev[e++].get(), s));
      launch_ba_kind(a, kind, s);
    }
    HIPCHK(hipGetLastError());
  }
  if (r->timing) HIPCHK(hipEventRecord(tev[e++].get(), s));
  hipLaunchKernelGGL(k_ba_final, dim3(ba_grid(3 * (size_t)r->in.n)), dim3(kBaBlock), 0, s, a);
  HIPCHK(hipGetLastError());
  if (int rc = r->out.post(sizeof(BaState), s)) return rc;
  r->tev = std::move(tev);
  r->timed = r->timing;
  return ICTR_OK;
}

extern "C" int ictr_ba_wait(ictr_ba *r, double *G, double *X, double *cost, double *damp, int32_t *iters, int32_t *status,
                            int64_t *n) {
  if (!r) return fail(ICTR_ERR_INVALID, "ba is NULL");
  if (!r->out.pending()) return fail(ICTR_ERR_STATE, "ba_wait: nothing has been run");
  if (int rc = r->out.wait()) return rc;
  const BaState *st = reinterpret_cast<const BaState *>(r->out.host());
  if (G) memcpy(G, st->G, sizeof(double) * 12 * (size_t)r->in.nframes);
  if (cost) *cost = st->c;
  if (damp) *damp = st->damp;
  if (iters) *iters = st->it;
  if (status) *status = st->status;
  if (n) *n = st->n;
  if (r->timed) {
    float ms[kBaKinds] = {0, 0, 0, 0, 0, 0, 0};
    for (size_t k = 0; k + 1 < r->tev.size(); ++k) {
      float t = 0;
      HIPCHK(hipEventElapsedTime(&t, r->tev[k].get(), r->tev[k + 1].get()));
      ms[k % kBaKinds] += t;
    }
    memcpy(r->ms, ms, sizeof(ms));
    r->tev.clear();
  }
  if (X) HIPCHK(hipMemcpy(X, r->d_Xout.get(), sizeof(double) * 3 * (size_t)r->in.n, hipMemcpyDeviceToHost));
  return ICTR_OK;
}

extern "C" int ictr_ba_get_kernel_times(const ictr_ba *r, float *ms) {
  if (!r || !ms) return fail(ICTR_ERR_INVALID, "ba_get_kernel_times: NULL argument");
  if (r->out.pending() || !r->timed) return fail(ICTR_ERR_STATE, "ba_get_kernel_times: no completed timed run");
  memcpy(ms, r->ms, sizeof(r->ms));
  return ICTR_OK;
}

extern "C" int ictr_debug_ba_system(ictr_ba *r, const double *G, const double *X, double damp, int64_t *n, double *cost,
                                    double *A, double *rhs, double *V, double *gp, int64_t *nfail) {
  if (!r || !G || !n || !cost || !A || !rhs || !V || !gp || !nfail)
    return fail(ICTR_ERR_INVALID, "debug_ba_system: NULL argument");
  if (int rc = r->in.ready("debug_ba_system", r->out, "ba")) return rc;
  if (int rc = ba_poses_finite(G, r->in.nframes, "debug_ba_system")) return rc;
  if (!(damp >= 0.0) || !cf_finite(damp)) return fail(ICTR_ERR_INVALID, "debug_ba_system: damp must be finite and >= 0");
  const CfParams p = {0, damp > 0.0 ? damp : 1.0, 2.0, 0.0, 1.0};
  BaArgs a;
  ba_fill_args(r, p, a);
  a.debug = 1;
  const int e = X ? 1 : 0;
  const size_t N = (size_t)r->in.n, D = sizeof(double);
  if (X) {  // the given points go through the second set
    HIPCHK(hipMemcpy(r->d_X[1].get(), X, D * 3 * N, hipMemcpyHostToDevice));
    a.Xin = r->d_X[1].get();
  }
  auto st = std::make_unique<BaState>();
  ba_init(*st, G, r->in.nframes, p);
  st->damp = damp;
  st->cur = st->tset = e;
  HIPCHK(hipMemcpy(r->out.dev(), st.get(), sizeof(BaState), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_ba_flags, dim3(ba_grid(N)), dim3(kBaBlock), 0, nullptr, a);
  for (int kind = 0; kind < kBaKinds - 1; ++kind) launch_ba_kind(a, kind, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(st.get(), r->out.dev(), sizeof(BaState), hipMemcpyDeviceToHost));
  *n = st->n;
  *cost = st->c;
  double fails = 0.0;
  HIPCHK(hipMemcpy(&fails, r->d_T.get() + kBaFailSlot, D, hipMemcpyDeviceToHost));
  *nfail = (int64_t)fails;
  HIPCHK(hipMemcpy(A, r->d_A.get(), D * (size_t)(r->dim * (r->dim + 1) / 2), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(rhs, r->d_rhs.get(), D * (size_t)r->dim, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(V, r->d_V[e].get(), D * 6 * N, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(gp, r->d_gp[e].get(), D * 3 * N, hipMemcpyDeviceToHost));
  return ICTR_OK;
}
