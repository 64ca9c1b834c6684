// ictr_sequence.hip -- the step BETWEEN two frame pairs of a video (run_odometer_test.m:172-250) on the device.
//
// A sequence tracks frame t -> t+1 from the pose it has just found for frame t. Between two trackings the script culls
// the world points against frame t's view, keeps every s-th survivor and hands them to a fresh Set3Dpoints + SetPose;
// here that step is three launches on the tracking's stream, so the host never waits between pairs (one more than the
// "one or two" first planned: the one-workgroup finish keeps the f64 normalisation sums in one fixed order without a
// grid-wide last-workgroup hand-off):
//
//   k_seq_select_count    every workgroup: p_t from the previous pair's final record (the getpose arithmetic,
//                         ictr_pose_hd.h; p_0 from the arguments; the previous pose again when the previous pair was
//                         lost), G(p_t) in f64, the cull of its kSeqChunk world points in f64 -> one 64-bit ballot per
//                         wave and step, survivors per workgroup. Workgroup 0 also writes p_t and the previous pair's
//                         iteration count to the outputs. With `tail` set only that bookkeeping runs (the last pose).
//   k_seq_select_scatter  every workgroup: its first survivor's rank (sum of the counts in front of it), ranks inside it
//                         from the masks (popcounts across waves and steps, mbcnt inside a wave), the ranks 0, s, 2s, ...
//                         below s * cap -> sel[rank / s] = world index (world order); patch / coefficient state zeroed
//                         over [0, npts).
//   k_seq_select_finish   one workgroup: meanshift / varval of the selected points in f64 in a fixed order (per-thread
//                         strided sums, then a fixed tree), the normalised f32 points into the engine's pt3d, the initial
//                         record as ictr_batch_begin's host part writes it (p and G from the setpose arithmetic, npts,
//                         normdp).
//
// Every value is decided by integer counts and fixed-order sums: no float atomics, the same bits on every run.
#include "ictr_dev.h"
#include "ictr_launch.h"
#include "ictr_pose_hd.h"
#include "se3_math.h"

namespace ictr {

// p_t of pair a.t (thread-local; called by one thread per workgroup)
__device__ void seq_pose(const SeqArgs &a, double *p) {
  if (a.t == 0) {
    for (int k = 0; k < 6; ++k) p[k] = a.p0[k];
    return;
  }
  const SeqState &ss = *a.ss;
  if (ss.npts == 0) {  // the previous pair selected no point: its pose is carried
    for (int k = 0; k < 6; ++k) p[k] = a.poses[(size_t)(a.t - 1) * 6 + k];
    return;
  }
  const ProbState &st = *a.st;
  float pf[6], Gf[12];
  for (int k = 0; k < 6; ++k) pf[k] = st.p[k];
  for (int k = 0; k < 12; ++k) Gf[k] = st.G[k];
  host_getpose(a.donorm != 0, pf, Gf, ss.ms, ss.varval, p);
}

__global__ void __launch_bounds__(kSeqBlock) k_seq_select_count(SeqArgs a) {
  __shared__ double sG[12];
  __shared__ unsigned sWave[kSeqBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) {
    double p[6], G[12];
    seq_pose(a, p);
    se3_exp<double>(G, p);
    for (int k = 0; k < 12; ++k) sG[k] = G[k];
    if (blockIdx.x == 0) {
      for (int k = 0; k < 6; ++k) a.poses[(size_t)a.t * 6 + k] = a.ss->pose[k] = p[k];
      if (a.t > 0) a.iters_out[a.t - 1] = a.ss->npts == 0 ? 0 : a.st->total_iters;
    }
  }
  if (a.tail) return;
  __syncthreads();
  double G[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) G[k] = sG[k];
  const long long base = (long long)blockIdx.x * kSeqChunk;
  const long long nw = a.nw;
  unsigned count = 0;
  for (int k = 0; k < kSeqPPT; ++k) {
    const long long i = base + (long long)k * kSeqBlock + tid;
    bool keep = false;
    if (i < nw) {
      const double X = a.X[i], Y = a.X[i + nw], Z = a.X[i + 2 * nw];
      const double xc = G[0] * X + G[1] * Y + G[2] * Z + G[3];
      const double yc = G[4] * X + G[5] * Y + G[6] * Z + G[7];
      const double zc = G[8] * X + G[9] * Y + G[10] * Z + G[11];
      const double u = a.fx * xc / zc + a.cx;
      const double v = a.fy * yc / zc + a.cy;
      keep = u >= 1.0 && u <= a.w && v >= 1.0 && v <= a.h;  // the script's bounds, literally; no depth test
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) a.mask[(size_t)blockIdx.x * (kSeqChunk / 64) + k * (kSeqBlock / 64) + wave] = m;
    count += (unsigned)__popcll(m);
  }
  if (lane == 0) sWave[wave] = count;
  __syncthreads();
  if (tid == 0) {
    unsigned c = 0;
    for (int w = 0; w < kSeqBlock / 64; ++w) c += sWave[w];
    a.cnt[blockIdx.x] = c;
  }
}

// survivors in front of workgroup `blk` and in total (every thread of the workgroup gets both)
__device__ void seq_prefix(const SeqArgs &a, int blk, unsigned *before, unsigned *total, unsigned *sRed, int nthr) {
  const int tid = threadIdx.x;
  unsigned pre = 0, tot = 0;
  for (int j = tid; j < a.nblk; j += nthr) {
    const unsigned c = a.cnt[j];
    tot += c;
    if (j < blk) pre += c;
  }
  sRed[tid] = pre;
  sRed[nthr + tid] = tot;
  __syncthreads();
  for (int h = nthr / 2; h > 0; h >>= 1) {
    if (tid < h) {
      sRed[tid] += sRed[tid + h];
      sRed[nthr + tid] += sRed[nthr + tid + h];
    }
    __syncthreads();
  }
  *before = sRed[0];
  *total = sRed[nthr];
  __syncthreads();
}

__device__ __forceinline__ int seq_npts(const SeqArgs &a, unsigned total) {
  const unsigned long long sel = ((unsigned long long)total + a.stride - 1) / a.stride;
  return (int)min(sel, (unsigned long long)a.cap);
}

__global__ void __launch_bounds__(kSeqBlock) k_seq_select_scatter(SeqArgs a) {
  __shared__ unsigned sRed[2 * kSeqBlock];
  __shared__ unsigned sOff[kSeqChunk / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned before, total;
  seq_prefix(a, blockIdx.x, &before, &total, sRed, kSeqBlock);
  const int npts = seq_npts(a, total);
  const unsigned long long *mk = a.mask + (size_t)blockIdx.x * (kSeqChunk / 64);
  if (tid < kSeqChunk / 64) sOff[tid] = (unsigned)__popcll(mk[tid]);
  __syncthreads();
  if (tid == 0) {  // exclusive scan of the 64 per-(step, wave) counts: step-major, wave-minor = world order
    unsigned run = before;
    for (int j = 0; j < kSeqChunk / 64; ++j) {
      const unsigned c = sOff[j];
      sOff[j] = run;
      run += c;
    }
  }
  __syncthreads();
  const unsigned s = (unsigned)a.stride;
  const unsigned long long lim = (unsigned long long)a.cap * s;
  for (int k = 0; k < kSeqPPT; ++k) {
    const int j = k * (kSeqBlock / 64) + wave;
    const unsigned long long m = mk[j];
    if ((m >> lane) & 1ull) {
      const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
      const unsigned r = sOff[j] + below;
      if (r % s == 0 && (unsigned long long)r < lim)
        a.sel[r / s] = (int)((long long)blockIdx.x * kSeqChunk + (long long)k * kSeqBlock + tid);
    }
  }
  // ResetOdometer (odometer.cpp:580-609) over the points the tracking will read
  const size_t gtid = (size_t)blockIdx.x * kSeqBlock + tid, gstride = (size_t)a.nblk * kSeqBlock;
  const size_t nT = (size_t)npts * a.n, nC = (size_t)npts * kCoefStride;
  for (size_t q = gtid; q < nT; q += gstride) {
    a.T[q] = 0.0f;
    a.Gx[q] = 0.0f;
    a.Gy[q] = 0.0f;
  }
  for (size_t q = gtid; q < nC; q += gstride) a.coef[q] = 0.0f;
}

__device__ __forceinline__ unsigned long long seq_mix(unsigned long long z) {  // splitmix64 finaliser
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// fixed-order tree over kSeqFinish doubles in LDS (every thread calls it; the result is in s[0])
__device__ void seq_tree(double *s) {
  const int tid = threadIdx.x;
  __syncthreads();
  for (int h = kSeqFinish / 2; h > 0; h >>= 1) {
    if (tid < h) s[tid] += s[tid + h];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kSeqFinish) k_seq_select_finish(SeqArgs a) {
  __shared__ unsigned sRed[2 * kSeqFinish];
  __shared__ double sD[3][kSeqFinish];
  __shared__ unsigned long long sH[kSeqFinish];
  __shared__ ProbState sSt;
  const int tid = threadIdx.x;
  unsigned before, total;
  seq_prefix(a, 0, &before, &total, sRed, kSeqFinish);
  const int npts = seq_npts(a, total);
  const long long nw = a.nw;
  const int M = a.M;
  // odometer.cpp:198-214 on the selected points: meanshift, then the mean squared radius (no sqrt)
  double ms[3] = {0.0, 0.0, 0.0}, varval = 1.0;
  if (a.donorm && npts > 0) {
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int i = tid; i < npts; i += kSeqFinish) {
      const long long w = a.sel[i];
      sx += a.X[w];
      sy += a.X[w + nw];
      sz += a.X[w + 2 * nw];
    }
    sD[0][tid] = sx;
    sD[1][tid] = sy;
    sD[2][tid] = sz;
    __syncthreads();
    for (int h = kSeqFinish / 2; h > 0; h >>= 1) {
      if (tid < h)
        for (int c = 0; c < 3; ++c) sD[c][tid] += sD[c][tid + h];
      __syncthreads();
    }
    const double nd = (double)npts;
    ms[0] = sD[0][0] / nd;
    ms[1] = sD[1][0] / nd;
    ms[2] = sD[2][0] / nd;
    __syncthreads();
    double vv = 0.0;
    for (int i = tid; i < npts; i += kSeqFinish) {
      const long long w = a.sel[i];
      const double p1 = a.X[w] - ms[0], p2 = a.X[w + nw] - ms[1], p3 = a.X[w + 2 * nw] - ms[2];
      vv += p1 * p1 + p2 * p2 + p3 * p3;
    }
    sD[0][tid] = vv;
    seq_tree(sD[0]);
    varval = sD[0][0] / nd;
  }
  // the normalised f32 points (f64 -> f32 SoA, zeros behind npts like the host's staging buffer)
  for (int i = tid; i < M; i += kSeqFinish) {
    float x = 0.0f, y = 0.0f, z = 0.0f;
    if (i < npts) {
      const long long w = a.sel[i];
      if (a.donorm) {
        x = (float)((a.X[w] - ms[0]) / varval);
        y = (float)((a.X[w + nw] - ms[1]) / varval);
        z = (float)((a.X[w + 2 * nw] - ms[2]) / varval);
      } else {
        x = (float)a.X[w];
        y = (float)a.X[w + nw];
        z = (float)a.X[w + 2 * nw];
      }
    }
    a.pt3d[i] = x;
    a.pt3d[i + M] = y;
    a.pt3d[i + 2 * M] = z;
  }
  // order-aware hash of the selection (integer sum: the same whatever the reduction order)
  unsigned long long h = 0;
  for (int i = tid; i < npts; i += kSeqFinish)
    h += seq_mix(((unsigned long long)(unsigned)i << 32) | (unsigned)a.sel[i]);
  sH[tid] = h;
  __syncthreads();
  for (int hh = kSeqFinish / 2; hh > 0; hh >>= 1) {
    if (tid < hh) sH[tid] += sH[tid + hh];
    __syncthreads();
  }
  // the initial record, as begin_prepare writes it from SetPose (built in LDS, stored by all threads)
  unsigned *sw = reinterpret_cast<unsigned *>(&sSt);
  for (int i = tid; i < (int)(sizeof(ProbState) / 4); i += kSeqFinish) sw[i] = 0u;
  __syncthreads();
  if (tid == 0) {
    host_setpose(a.donorm != 0, a.ss->pose, ms, varval, sSt.p, sSt.G);
    sSt.npts = npts;
    sSt.normdp = sSt.normdp_init = 1e-10f;
    for (int c = 0; c < 3; ++c) a.ss->ms[c] = ms[c];
    a.ss->varval = varval;
    a.ss->npts = npts;
    a.npts_out[a.t] = npts;
    a.hash[a.t] = sH[0];
  }
  __syncthreads();
  unsigned *dst = reinterpret_cast<unsigned *>(a.st);
  for (int i = tid; i < (int)(sizeof(ProbState) / 4); i += kSeqFinish) dst[i] = sw[i];
}

// the between-pairs step (three launches), or with a.tail the last frame's bookkeeping (one)
void launch_seq_select(const SeqArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(k_seq_select_count, dim3(a.tail ? 1 : a.nblk), dim3(kSeqBlock), 0, s, a);
  if (a.tail) return;
  hipLaunchKernelGGL(k_seq_select_scatter, dim3(a.nblk), dim3(kSeqBlock), 0, s, a);
  hipLaunchKernelGGL(k_seq_select_finish, dim3(1), dim3(kSeqFinish), 0, s, a);
}

}  // namespace ictr
