// ictr_resident.hip -- all Gauss-Newton iterations of a pyramid level with the templates RESIDENT on the chip
// (gfx950 / CDNA4; 8x8 patches, large problems: thousands to tens of thousands of points per frame pair).
//
// The per-iteration kernel k_iter8 streams T, Gx, Gy of every patch from HBM in every iteration: 12 of its 16 bytes
// per pixel, ten times per level, and it runs at the HBM roofline doing so. But a frame pair's templates are only 25 MB
// per level -- the chip has 128 MB of vector registers and 40 MB of LDS. Here a frame pair is shared by `parts` worker
// workgroups that load their templates ONCE per level and keep them for all iterations of odometer.cpp:344-418; an
// iteration then reads only the current frame's windows (cache-resident) and exchanges six numbers per workgroup.
//
// r03 form (what bounds this kernel is the number of frame pairs in flight -- an iteration is a latency chain of two
// hops through memory -- so the design maximises the templates a CU holds):
//   * a worker workgroup = 4 waves, a wave keeps THIRTY-TWO patches: Gx and Gy of a patch are two registers of the wave
//     (lane = pixel; 64 of its 128 registers), T sits in LDS (32 KB per workgroup); four workgroups per CU = 512 points
//     = 384 KB of templates per CU, FOUR 1080p frame pairs in flight on the chip (r02: two);
//   * J is constant over a patch (odometer.cpp:313-326), so b_k = sum_px sd_k r = sum_patches [cx_k A + cy_k B] with the
//     two per-patch sums A = sum Gx r, B = sum Gy r: per pixel the loop does the bilinear blend, the residual and two
//     products; the 64 per-lane values (A, B of 32 patches) are summed over the 64 lanes by a TRANSPOSING reduction
//     (each merge halves the registers and doubles the lanes summed: two instructions per value) that leaves lane l
//     with the complete sum of one (patch, A|B); the lane then applies ITS point's six coefficients -- no per-patch
//     coefficient broadcast, no per-pixel multiply-adds into six sums;
//   * the workgroup's six partial sums travel as six float granules (the precision of the streaming form's float
//     partials); the pair's SOLVER workgroup polls them in one round trip (256 lanes x 8 granules), adds in a fixed
//     order in f64, one wave runs the solver turn (WaveSolver, ictr_devfn.h: substitution with the level's LU factors,
//     pose update, exp map, loop condition; odometer.cpp:407-418, 509-515) and broadcasts cpos_G + the loop flag.
//   * current-frame windows (r05, ICTR_RES_WIN = 1): a lane loads only the row pair (a, b) of its own pixel row; (c, d) is
//     the (a, b) of the lane eight below and arrives by two ds_bpermute when the patch is blended; the window's top row
//     (nine texels, which no lane holds) comes for four patches in one one-register load and one more ds_bpermute. Two
//     registers per window in flight instead of four and 40 instead of 64 load instructions per wave and iteration;
//     kResD windows in flight (ICTR_RES_D). The blend's operands and order are those of the full-window form
//     (ICTR_RES_WIN = 0, kept as the A/B reference), so b and the poses keep their bits.
// The mailbox protocol and this form's mailbox layout: ictr_xchg.h.
// H partials come from the level's setup launch (k_ref8: three sums per patch) and are reduced + factored by the pair's
// solver workgroup at the start of the pair (what k_level_tail does in the other launch forms); templates and (possibly
// stale) coefficients come from the buffers that launch wrote: patches, coefficients and projections are bit-identical
// to the other launch forms, b differs by summation order only.
#include <string.h>

#include <type_traits>

#include "ictr_dev.h"
#include "ictr_launch.h"
#include "ictr_devfn.h"
#include "se3_math.h"

namespace ictr {

constexpr int kResWaves = 4;                // waves per workgroup
constexpr int kResThreads = 64 * kResWaves;
// patches (points) per wave: template parameter NP of the kernel, 32 (large batches: four pairs in flight) or 16 (one
// or two pairs: twice the workgroups, half the patch loop); points per workgroup = kResWaves * NP
#ifndef ICTR_RES_AUX
#define ICTR_RES_AUX 2  // template loads of the pair prologue: slc (streamed)
#endif
// window form: 1 = half windows (a lane loads its own row pair; the pair of the row above comes from the lane eight below,
// the window's top row for four patches in one load: two registers per window in flight), 0 = full windows (four registers)
#ifndef ICTR_RES_WIN
#define ICTR_RES_WIN 1
#endif
#ifndef ICTR_RES_D
#define ICTR_RES_D (ICTR_RES_WIN ? 8 : 4)
#endif
constexpr int kResD = ICTR_RES_D;           // current-frame windows in flight per wave
static_assert(kResD >= 1 && kResD <= 16, "windows in flight: at most the patches of a wave");

struct ResArgs {
  LevelCam lc;
  int level;
  int parts, slots;          // worker workgroups per frame pair; pairs in flight (grid = slots * (parts + 1))
  int nblk;                  // workgroups per problem of the level's setup launch (their H partials: e.partH)
  int prof_slot;             // ICTR_RES_PROF builds: the slot whose worker 0 / solver report their cycle counters
  ResXchg x;                 // x.world > 1: the solver workgroups sum H and b over the ranks (one-hop mailbox exchange)
  Exchange ex;               // the launch's exchange; the mailbox in the resident layout (ictr_xchg.h)
};

// poll up to eight granules per lane until every tag matches; lanes / entries without a granule pass nullptr
// (entries written out one by one: everything stays in registers). TWO sets of requests are kept in flight, half a
// round trip apart: a granule is seen at most half a memory round trip after it became visible (one set: a whole one).
#define RES_EACH8(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
__device__ __forceinline__ void res_poll(XchgPoll &pc, const unsigned long long *(&src)[8], unsigned long long (&g)[8],
                                         unsigned tag, int lane) {
  const unsigned long long empty = xchg_empty(tag);
#define RES_LOAD(u) g[u] = src[u] ? __hip_atomic_load(src[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : empty;
  RES_EACH8(RES_LOAD)
  if (pc.dead) return;
  unsigned long long h[8];
  __builtin_amdgcn_s_sleep(4);
#define RES_LOADH(u) h[u] = src[u] ? __hip_atomic_load(src[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : empty;
  RES_EACH8(RES_LOADH)
  bool started = false;
  unsigned long long t0 = 0;
  for (;;) {
    bool miss = false;
#define RES_MISS(u) miss |= xchg_miss(g[u], tag);
    RES_EACH8(RES_MISS)
    if (__builtin_amdgcn_ballot_w64(miss) == 0) break;  // wave-uniform
    XCHG_TIMEOUT_STEP(pc, started, t0, lane)
    // the older set's answers replace what is still missing; that set is requested again for what is missing then
#define RES_ROTATE(u)                                                                                         \
  if (xchg_miss(g[u], tag)) {                                                                                 \
    g[u] = h[u];                                                                                              \
    h[u] = __hip_atomic_load(src[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                             \
  }
    RES_EACH8(RES_ROTATE)
  }
}
// one granule per lane (the workers' wait for the broadcast): three requests in flight
__device__ __forceinline__ unsigned long long res_poll1(XchgPoll &pc, const unsigned long long *src, unsigned tag, int lane) {
  const unsigned long long empty = xchg_empty(tag);
  unsigned long long g = src ? __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : empty;
  if (pc.dead) return g;
  __builtin_amdgcn_s_sleep(3);
  unsigned long long h1 = src ? __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : empty;
  __builtin_amdgcn_s_sleep(3);
  unsigned long long h2 = src ? __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : empty;
  bool started = false;
  unsigned long long t0 = 0;
  while (__builtin_amdgcn_ballot_w64(xchg_miss(g, tag)) != 0) {
    XCHG_TIMEOUT_STEP(pc, started, t0, lane)
    if (xchg_miss(g, tag)) {
      g = h1;
      h1 = h2;
      h2 = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  return g;
}

// (the transposing wave reduction -- tr_merge_*, TrAcc, tr_for_each_patch -- lives in ictr_devfn.h: k_ref8 uses it too)
// inspection (tests/test_gpu_parity.py): the reduction alone on caller data, vals[lane][2 patch + kind]
template <int NP>
__global__ __launch_bounds__(64) void k_debug_transpose_reduce(const float *__restrict__ vals, float *__restrict__ out,
                                                               int *__restrict__ patch_of_lane, int *__restrict__ kind_of_lane) {
  const int lane = threadIdx.x;
  TrAcc<NP> acc;
  tr_for_each_patch<NP, 0>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    acc.template push<j>(vals[lane * 64 + 2 * j], vals[lane * 64 + 2 * j + 1], lane);
  });
  out[lane] = acc.F;
  patch_of_lane[lane] = tr_patch_of_lane<NP>(lane);
  kind_of_lane[lane] = tr_kind_of_lane(lane);
}
hipError_t launch_debug_transpose_reduce(const float *vals, float *out, int *pl, int *kl, int np, hipStream_t s) {
  if (np == 16)
    hipLaunchKernelGGL(k_debug_transpose_reduce<16>, dim3(1), dim3(64), 0, s, vals, out, pl, kl);
  else
    hipLaunchKernelGGL(k_debug_transpose_reduce<32>, dim3(1), dim3(64), 0, s, vals, out, pl, kl);
  return hipGetLastError();
}

// inspection (tests/test_gpu_resident_windows.py): the half-window fetch path alone, one wave, eight windows of a caller
// plane: top_left[g] = texel index of window g's top-left texel -> out[g][lane] = {a, b, c, d}. The resource is bounded by
// the plane, so a window that leaves it reads zeros.
__global__ __launch_bounds__(64) void k_debug_half_window(const float *__restrict__ plane, int ntexels, int sw,
                                                          const int *__restrict__ top_left, float4 *__restrict__ out) {
  const int lane = threadIdx.x;
  const HalfWinLane hwl = hw_lane(lane);
  const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(plane), 0, ntexels * 4, 0x00020000);
  const int off_ab = ((lane >> 3) * sw + (lane & 7) + sw) * 4;
  const int base_v = top_left[lane & 7] * 4;
  const float row[2] = {hw_load_row(rp, hw_row_voff(base_v, 0, lane)), hw_load_row(rp, hw_row_voff(base_v, 1, lane))};
  tr_for_each_patch<8, 0>([&](auto gc) {
    constexpr int g = decltype(gc)::value;
    const f32x2_a4 ab = hw_load(rp, off_ab, rlane(base_v, g));
    int q[3];
    hw_cd_issue<g % 4>(ab, row[g / 4], hwl, q);
    const f32x2_a4 cd = hw_cd_take(q);
    out[g * 64 + lane] = make_float4(ab.y, ab.x, cd.y, cd.x);
  });
}
hipError_t launch_debug_half_window(const float *plane, int ntexels, int sw, const int *top_left, float *out, hipStream_t s) {
  hipLaunchKernelGGL(k_debug_half_window, dim3(1), dim3(64), 0, s, plane, ntexels, sw, top_left, reinterpret_cast<float4 *>(out));
  return hipGetLastError();
}

// Sharded resident form: lanes [0, n) of the solver's wave 0 each hold one local value; it goes as one granule into
// [pair * kXchgPerPair + off + lane] of this rank's slot of EVERY rank's mailbox (system-scope stores over the
// point-to-point links), then the lane polls its own mailbox for the same granule of every rank and adds them in rank
// order in f64 (ictr_xchg.h's protocol with rank tags, inside the launch: no kernel boundary, no host, no communicator).
__device__ __forceinline__ double res_xchg_sum(const ResXchg &x, XchgPoll &pc, int pair, unsigned xs, int off, int n, float v,
                                               int lane) {
  const unsigned tag = xchg_rank_tag(xs);
  const size_t par = rank_mail_slot(xs, x.world);
  const size_t idx = (size_t)pair * kXchgPerPair + off + lane;
  if (lane < n) {
    const unsigned long long g = xchg_pack(tag, v);
    for (int r = 0; r < x.world; ++r)
      __hip_atomic_store(x.peer[r] + rank_mail_index(par + x.rank, x.cap, idx), g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  // the peers' granules: eight ranks' requests in flight at a time (one fabric round trip for a node of eight), re-polled
  // until every tag matches; added in rank order
  double sum = 0.0;
  bool started = false;
  unsigned long long t0 = 0;
  const unsigned long long empty = xchg_empty(tag);
  for (int r0 = 0; r0 < x.world; r0 += 8) {
    unsigned long long g[8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      g[u] = (lane < n && r0 + u < x.world)
                 ? __hip_atomic_load(x.local + rank_mail_index(par + r0 + u, x.cap, idx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                 : empty;
    while (!pc.dead) {
      bool miss = false;
#pragma unroll
      for (int u = 0; u < 8; ++u) miss |= xchg_miss(g[u], tag);
      if (__builtin_amdgcn_ballot_w64(miss) == 0) break;  // wave-uniform
      XCHG_TIMEOUT_STEP(pc, started, t0, lane)
      __builtin_amdgcn_s_sleep(1);
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (xchg_miss(g[u], tag))
          g[u] = __hip_atomic_load(x.local + rank_mail_index(par + r0 + u, x.cap, idx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) sum += (double)xchg_value(g[u]);
  }
  return sum;
}

// sum of a double over aligned groups of eight lanes (every lane of the group gets it)
__device__ __forceinline__ double res_sum8(double v) {
#define RES_DPP64(ctrl)                                                                              \
  {                                                                                                  \
    const int lo = dpp_mov<ctrl>(__double2loint(v)), hi = dpp_mov<ctrl>(__double2hiint(v));          \
    v += __hiloint2double(hi, lo);                                                                   \
  }
  RES_DPP64(0xB1)   // quad_perm [1,0,3,2]
  RES_DPP64(0x4E)   // quad_perm [2,3,0,1]
  RES_DPP64(0x141)  // row_half_mirror: the other quad of the group (its lanes all hold that quad's sum)
  return v;
}

typedef float f32x2_t __attribute__((ext_vector_type(2)));
#ifdef ICTR_RES_PROF  // diagnostic builds only: per-phase cycle counters of one wave (tools/resprof.py)
#define RES_MARK(k)                        \
  {                                        \
    t1_ = __builtin_readcyclecounter();    \
    tp_[k] += t1_ - t0_;                   \
    t0_ = t1_;                             \
  }
// time line (tools/restrace.py): 100 MHz wall-clock stamps of wave 0 of the workers that share CU `blockIdx % 256 == 0`
// (rows 0..7: one per slot) and of every slot's solver workgroup (rows 8..15), four stamps per iteration
constexpr int kTrIters = 128;
__device__ unsigned long long g_res_trace[16][kTrIters][4];
#define RES_STAMP(row, it, k) \
  if ((row) >= 0 && (it) < kTrIters && tid == 0) g_res_trace[row][it][k] = wall_clock64();
#else
#define RES_MARK(k)
#define RES_STAMP(row, it, k)
#endif
struct ResWin {
  f32x2_a4 ab, cd;  // (x-1,y),(x,y) and (x-1,y-1),(x,y-1)
};

__device__ __forceinline__ void res_setprio(int p) {  // wave-uniform p in 0..3 (the instruction takes an immediate)
  if (p == 0) __builtin_amdgcn_s_setprio(0);
  else if (p == 1) __builtin_amdgcn_s_setprio(1);
  else if (p == 2) __builtin_amdgcn_s_setprio(2);
  else __builtin_amdgcn_s_setprio(3);
}

// Register budget: 128 per wave = four 4-wave workgroups per CU (launch bounds), 64 of them Gx / Gy of the wave's patches.
template <int NP>
__global__ __launch_bounds__(kResThreads, 4) void k_level_resident(EngineDev e, ResArgs a) {
  constexpr int kResPPW = NP, kResQ = kResWaves * NP;
  __shared__ __attribute__((aligned(16))) float4 sRecW[kResWaves][kResPPW];  // per point: bilinear weights [w1 w0 w3 w2]
  __shared__ float sT[kResWaves][kResPPW * 64];  // T of the wave's patches (lane = pixel)
  __shared__ float sPart[kResWaves][8];
  __shared__ double sRed[kResWaves][8];
  __shared__ float sG[16];   // cpos_G of the current iteration, [12] = loop flag (bits)
  __shared__ ProbState sSt;  // solver workgroup: the problem's state between the solver's turns

  const int parts = a.parts;
  const int group = parts + 1;  // a pair's workgroups: `parts` workers (128 points each) + ONE solver workgroup (index parts)
  const int slot = (int)blockIdx.x / group;
  const int part = (int)blockIdx.x - slot * group;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int M = e.M;
  unsigned long long *gbox = a.ex.mail + res_gather_box(slot, parts);
  unsigned long long *bbox = gbox + res_bcast_box(parts);
  XchgPoll pc{a.ex.limit, a.ex.err, 0};
  unsigned seq = 0;
#ifdef ICTR_RES_PROF
  const int tr_row = part == parts ? (slot < 8 ? 8 + slot : -1) : ((part == 0 && slot < 8) ? slot : -1);
  int tr_it = 0;
  unsigned long long tp_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t0_ = __builtin_readcyclecounter(), t1_ = 0;
#endif

  if (part == parts) {
    __builtin_amdgcn_s_setprio(3);
    // ================================================================ the pair's solver workgroup
    SolveOpts sopt = solve_opts(e);
    sopt.robust = 0;
    __shared__ double sRedH[kResThreads / 32][32];
    __shared__ float sH[32];
    for (int b = slot, round = 0; b < e.B; b += a.slots, ++round) {
      const ProbState &gst = e.st[b];
      // loop condition of odometer.cpp:341-346 at the start of a level: normdp / normdp_init = 1 (every workgroup of the
      // pair evaluates it for itself; maxiter >= 1 is the host's condition for this form)
      int active = ((0 < e.maxiter) & (1.0f > e.ratio)) ? 1 : 0;
      {
        const unsigned *src = reinterpret_cast<const unsigned *>(&gst);
        unsigned *dst = reinterpret_cast<unsigned *>(&sSt);
        for (int i = tid; i < (int)(sizeof(ProbState) / 4); i += kResThreads) dst[i] = src[i];
      }
      // ---- what k_level_tail does in the other launch forms: fixed-order f64 sum of the H partials, full-pivot LU once
      // per level, loop state reset: the setup launch's partials (e.partH), while the pair's workers load their templates
      reduce_partH<kResThreads>(e, b, a.nblk, sRedH, sH);
      unsigned xs = 0;  // (sharded resident form) this pair's exchange count, wave 0 only
      if (wave == 0) {
        float hl = lane < kHUnique ? sH[lane] : 0.0f;
        if (a.x.world > 1) {  // H of the level = the sum over the ranks' point shards
          xs = a.x.xseq[b] + 1u;
          hl = (float)res_xchg_sum(a.x, pc, b, xs, 12, kHUnique, hl, lane);
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (every lane has read its sH entry)
          __builtin_amdgcn_wave_barrier();
          if (lane < kHUnique) sH[lane] = hl;
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        WaveSolver S;
        ws_factor(S, sH[h_unique_index(lane)], lane);
        ws_store_factor(S, sSt, lane);
        if (lane == 0) level_reset(sSt, e);
      }
      __syncthreads();
      while (active) {
        seq += 1;
        const unsigned tag = xchg_tag(a.ex.tag0, seq);
        const unsigned long long *gslot = gbox + res_gather_slot(seq, parts);
        unsigned long long *bslot = bbox + res_bcast_slot(seq);
        // lane (k, rr) = 8 k + rr (k < 6) reads value k of the workers ((8 wave + u) 8 + rr), u = 0..7: eight granule
        // loads in flight per lane, 256 workers per round trip; sums in a fixed order: u, rounds, rr, waves
        RES_MARK(0)  // solver: loop overhead / barrier behind the previous broadcast
        RES_STAMP(tr_row, tr_it, 0)
        const int k = lane >> 3, rr = lane & 7;
        double accd = 0.0;
        for (int r0 = 0; r0 < parts; r0 += 64 * kResWaves) {
          const unsigned long long *src[8];
          unsigned long long g[8];
#define RES_SRC(u)                                                                   \
  {                                                                                  \
    const int r = r0 + (wave * 8 + u) * 8 + rr;                                      \
    src[u] = (k < 6 && r < parts) ? gslot + res_gather_row(r) + k : nullptr;        \
  }
          RES_EACH8(RES_SRC)
          res_poll(pc, src, g, tag, lane);
#define RES_ACC(u) accd += (double)xchg_value(g[u]);
          RES_EACH8(RES_ACC)
        }
        const double tot = res_sum8(accd);
        RES_MARK(1)  // solver: waiting for / summing the workers' granules
        RES_STAMP(tr_row, tr_it, 1)
        if (rr == 0 && k < 6) sRed[wave][k] = tot;
        __syncthreads();
        RES_MARK(2)  // solver: barrier
        RES_STAMP(tr_row, tr_it, 2)
        if (wave == 0) {
          double bsum = 0.0;
          if (lane < 6)
            for (int w = 0; w < kResWaves; ++w) bsum += sRed[w][lane];
          if (a.x.world > 1) {
            // b is a sum of signed terms: a shard's partial can be much larger than the total, so it travels as a (hi, lo)
            // pair of floats (lanes 0-5 / 6-11) and the ranks' total is rounded once (as the team form does)
            xs += 1u;
            const float hi = (float)bsum;
            const float lo = (float)(bsum - (double)hi);
            const float pv = lane < 6 ? hi : lane_gather(lo, lane - 6);
            const double t = res_xchg_sum(a.x, pc, b, xs, 0, 12, pv, lane);
            const int l6 = lane + 6;
            bsum = t + __hiloint2double(lane_gather(__double2hiint(t), l6), lane_gather(__double2loint(t), l6));
          }
          WaveSolver S;
          float G[12];
          ws_load_state(S, sSt, lane, G);
          ws_load_factor(S, sSt, lane);
          ws_iterate(S, (float)bsum, sopt, a.level, b, lane, G);
          ws_store_state(S, sSt, lane, G);
          float gv = 0.0f;
#pragma unroll
          for (int q = 0; q < 12; ++q) gv = lane == q ? G[q] : gv;
          const int act = pc.dead ? 0 : S.active;  // a time-out ends the pair (the host reports the failure)
          if (lane == 12) gv = __builtin_bit_cast(float, act);
          if (lane < 13)
            __hip_atomic_store(bslot + lane, xchg_pack(tag, gv), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (lane == 0) sG[12] = __builtin_bit_cast(float, act);
          RES_MARK(3)  // solver: solve + broadcast
          RES_STAMP(tr_row, tr_it, 3)
        }
#ifdef ICTR_RES_PROF
        tr_it += 1;
#endif
        __syncthreads();
        active = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, sG[12]));
      }
      if (wave == 0) {  // final state of the level (H, factors, pose, loop state) back to the problem's record
        if (a.x.world > 1 && lane == 0) a.x.xseq[b] = xs;
        const unsigned *src = reinterpret_cast<const unsigned *>(&sSt);
        unsigned *dst = reinterpret_cast<unsigned *>(e.st + b);
        for (int i = lane; i < (int)(sizeof(ProbState) / 4); i += 64) dst[i] = src[i];
      }
      __syncthreads();
    }
#ifdef ICTR_RES_PROF
    if (slot == a.prof_slot && tid == 0)
      for (int k = 0; k < 8; ++k) e.partH[8 + k] = (float)tp_[k];
#endif
    return;
  }

  // ================================================================ a worker workgroup: 128 points of the pair
  const LevelCam lc = a.lc;
  const int sw = lc.sw;
  const unsigned off_cd = (unsigned)((lane >> 3) * sw + (lane & 7)) * 4u;  // bytes from the window's top-left texel
  const unsigned off_ab = off_cd + (unsigned)sw * 4u;
  const HalfWinLane hwl = hw_lane(lane);
  float4 *const recs = sRecW[wave];
  float *const tw = sT[wave] + lane;
  const int my_patch = tr_patch_of_lane<NP>(lane);  // the (patch, A|B) whose complete sum this lane holds after stage 2
  const int my_kind = tr_kind_of_lane(lane);
  for (int b = slot, round = 0; b < e.B; b += a.slots, ++round) {
    res_setprio((slot + round) & 3);  // rotating wave priorities: 4.29 -> 4.03 ms per 32 pairs (r03 notes)
    const ProbState &gst = e.st[b];
    const int npts = gst.npts;
    int active = ((0 < e.maxiter) & (1.0f > e.ratio)) ? 1 : 0;  // as the solver workgroup evaluates it (odometer.cpp:341-346)
    if (!active) continue;
    const int i0 = part * kResQ + wave * kResPPW;
    const int cnt = min(kResPPW, max(0, npts - i0));  // this wave's points (wave-uniform)
    // (the plane pointer is wave-uniform, but it comes out of a table in memory: say so, or every buffer load below is
    // wrapped in a waterfall loop over its descriptor)
    const float *cur_plane;
    {
      const unsigned long long pc64 = reinterpret_cast<unsigned long long>(e.planes[b * e.nlev + a.level].cur);
      const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)pc64), hi = __builtin_amdgcn_readfirstlane((unsigned)(pc64 >> 32));
      cur_plane = reinterpret_cast<const float *>(((unsigned long long)hi << 32) | lo);
    }
    const __amdgpu_buffer_rsrc_t rcur =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(cur_plane), 0, 0x7fffffff, 0x00020000);
    f32x2_t Gxy[kResPPW];  // {Gx, Gy} of the lane's pixel, patch by patch: one register pair, one packed multiply by r
    const float *gT = e.T + ((size_t)b * M + i0) * 64 + lane;
    const float *gGx = e.Gx + ((size_t)b * M + i0) * 64 + lane;
    const float *gGy = e.Gy + ((size_t)b * M + i0) * 64 + lane;
    const bool pv = lane < cnt;
    float c6[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    // ---- templates of this wave's patches (written by the level's setup launch; stale ones included): Gx, Gy into
    // registers, T into LDS. Buffer loads bounded by the wave's point count (patches beyond it read as zeros: no
    // branches), Gx / Gy of all patches requested at once straight into the registers they stay in (one memory round
    // trip for the whole wave), T eight patches at a time (it only passes through)
    const int nbytes = __builtin_amdgcn_readfirstlane(cnt * 256);
    auto bounded = [&](const float *q) {
      const unsigned long long v = reinterpret_cast<unsigned long long>(q - lane);
      const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
      return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<float *>(((unsigned long long)hi << 32) | lo), 0, nbytes,
                                               0x00020000);
    };
    const __amdgpu_buffer_rsrc_t rT = bounded(gT), rGx = bounded(gGx), rGy = bounded(gGy);
    const int loff = lane * 4;
#pragma unroll
    for (int j = 0; j < kResPPW; ++j) {
      Gxy[j].x = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rGx, loff, j * 256, ICTR_RES_AUX));  // slc: streamed
      Gxy[j].y = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rGy, loff, j * 256, ICTR_RES_AUX));
    }
#pragma unroll
    for (int j0 = 0; j0 < kResPPW; j0 += 8) {
      float t8[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t8[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rT, loff, (j0 + u) * 256, ICTR_RES_AUX));
#pragma unroll
      for (int u = 0; u < 8; ++u) tw[(j0 + u) * 64] = t8[u];
    }
    // every lane: the six coefficients of ITS (patch, A|B): cx_k of point my_patch for an A lane, cy_k for a B lane
    // (odometer.cpp:313-326; zeros beyond the wave's points)
    if (my_patch < cnt && tr_primary_lane<NP>(lane)) {
      const float *cl = e.coef + ((size_t)b * M + i0 + my_patch) * kCoefStride + (my_kind ? 6 : 0);
#pragma unroll
      for (int k = 0; k < 6; ++k) c6[k] = cl[k];
    }
    // ---- lane l < NP: point i0 + l (X, Y, Z stay in registers)
    float X = 0.0f, Y = 0.0f, Z = 1.0f;
    if (pv) {
      const float *p3 = e.pt3d + (size_t)b * 3 * M;
      X = p3[i0 + lane], Y = p3[i0 + lane + M], Z = p3[i0 + lane + 2 * M];
    }
    if (tid < 12) sG[tid] = gst.G[tid];
    __syncthreads();

    while (active) {  // uniform over the pair's workgroups: every one of them follows the same broadcast
      RES_MARK(0)  // worker: barrier behind the broadcast
      RES_STAMP(tr_row, tr_it, 0)
      // ---- stage 1 (pose.cpp:384-391, odometer.cpp:369-377): lane l < 32 <-> point i0 + l
      int base_v;
      float vis_f;
      {
        float Gc[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) Gc[k] = sG[k];
        const IterPoint pt = iter_point(Gc, X, Y, Z, lc, pv, 4);
        const Taps &tp = pt.tp;
        base_v = ((tp.row0 - 1) * sw + tp.col0 - 1) * 4;  // bytes: the buffer load's scalar offset
        vis_f = pt.vis ? 1.0f : 0.0f;
        if (lane < kResPPW) recs[lane] = make_float4(tp.w1, tp.w0, tp.w3, tp.w2);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      RES_MARK(1)  // worker: stage 1
      // ---- stage 2: thirty-two patches from registers, kResD windows in flight. Per pixel: blend (utilities.cpp:107,
      // reference operand order, not contracted), residual (odometer.cpp:381), Gx r and Gy r; the per-patch sums by the
      // transposing reduction: a patch's (A, B) pair merges on lane bit 2, then a binary counter of pending registers
#if ICTR_RES_WIN
      // half windows (ictr_devfn.h): W holds the lanes' own row pairs, Rw the windows' top rows of two groups of four
      // patches (group k + 2 is requested into group k's register behind that group's last lane move); a patch's lane
      // moves are requested one patch ahead, like its weights and T
      constexpr int kRowK = kResPPW / 4;
      f32x2_a4 W[kResD];
      float Rw[2];
      auto issue = [&](int j) {
#if defined(ICTR_RES_ABL) && ICTR_RES_ABL == 2  // timing ablations (diagnostic builds, wrong results): no window loads in the loop
        if (j >= kResD) return;
#endif
#if defined(ICTR_RES_ABL) && ICTR_RES_ABL == 1  // ... every window = the plane's first (cache-resident)
        const int soff = 0;
#else
        const int soff = rlane(base_v, j);
#endif
        W[j % kResD] = hw_load(rcur, (int)off_ab, soff);
      };
      Rw[0] = hw_load_row(rcur, hw_row_voff(base_v, 0, lane));
#pragma unroll
      for (int j = 0; j < kResD; ++j) issue(j);
      TrAcc<NP> acc;
      float4 wv_n = recs[0];  // the next patch's weights, T and lane moves: one patch ahead of the arithmetic
      float t_n = tw[0];
      int q_n[3], vrow_n = 0;
      hw_cd_issue<0>(W[0], Rw[0], hwl, q_n);
      tr_for_each_patch<NP, 0>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        const float4 wv = wv_n;
        const float t = t_n;
        const f32x2_a4 cd = hw_cd_take(q_n);
        asm volatile("" ::: "memory");  // (the LDS reads of later patches stay behind this point: two patches' worth live)
        if constexpr (j + 1 < kResPPW) {
          wv_n = recs[j + 1];
          t_n = tw[(j + 1) * 64];
        }
        const f32x2_a4 ab = W[j % kResD];
        // w0 a + w1 b + w2 c + w3 d in the reference's order; the four products as two packed multiplies (each product
        // rounded on its own, like the scalar form)
        const f32x2_t pab = f32x2_t{wv.x, wv.y} * f32x2_t{ab.x, ab.y}, pcd = f32x2_t{wv.z, wv.w} * f32x2_t{cd.x, cd.y};
        const float inew = ((pab.y + pab.x) + pcd.y) + pcd.x;
        if constexpr (j + kResD < kResPPW) issue(j + kResD);
        if constexpr (j + 1 < kResPPW) hw_cd_issue<(j + 1) % 4>(W[(j + 1) % kResD], Rw[((j + 1) / 4) & 1], hwl, q_n);
        if constexpr (j == 0) Rw[1] = hw_load_row(rcur, hw_row_voff(base_v, 1, lane));  // (not with the first windows: registers)
        if constexpr (j % 4 == 1 && j / 4 + 2 < kRowK) vrow_n = hw_row_voff(base_v, j / 4 + 2, lane);
        if constexpr (j % 4 == 3 && j / 4 + 2 < kRowK) Rw[(j / 4) & 1] = hw_load_row(rcur, vrow_n);
        const float r = t - inew;  // pdiff (odometer.cpp:381); visibility is applied to the patch sums below
        const f32x2_t gr = Gxy[j] * f32x2_t{r, r};
        acc.template push<j>(gr.x, gr.y, lane);
      });
#else
      ResWin W[kResD];
      auto issue = [&](int j) {
#if defined(ICTR_RES_ABL) && ICTR_RES_ABL == 2  // timing ablations (diagnostic builds, wrong results): no window loads in the loop
        if (j >= kResD) return;
#endif
#if defined(ICTR_RES_ABL) && ICTR_RES_ABL == 1  // ... every window = the plane's first (cache-resident)
        const int soff = 0;
#else
        const int soff = rlane(base_v, j);
#endif
        W[j % kResD].cd = __builtin_bit_cast(f32x2_a4, __builtin_amdgcn_raw_buffer_load_b64(rcur, (int)off_cd, soff, 0));
        W[j % kResD].ab = __builtin_bit_cast(f32x2_a4, __builtin_amdgcn_raw_buffer_load_b64(rcur, (int)off_ab, soff, 0));
      };
#pragma unroll
      for (int j = 0; j < kResD; ++j) issue(j);
      TrAcc<NP> acc;
      float4 wv_n = recs[0];  // the next patch's weights and T: one patch ahead of the arithmetic (LDS latency hidden)
      float t_n = tw[0];
      tr_for_each_patch<NP, 0>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        const float4 wv = wv_n;
        const float t = t_n;
        asm volatile("" ::: "memory");  // (the LDS reads of later patches stay behind this point: two patches' worth live)
        if constexpr (j + 1 < kResPPW) {
          wv_n = recs[j + 1];
          t_n = tw[(j + 1) * 64];
        }
        const ResWin w = W[j % kResD];
        // w0 a + w1 b + w2 c + w3 d in the reference's order; the four products as two packed multiplies (each product
        // rounded on its own, like the scalar form)
        const f32x2_t pab = f32x2_t{wv.x, wv.y} * f32x2_t{w.ab.x, w.ab.y}, pcd = f32x2_t{wv.z, wv.w} * f32x2_t{w.cd.x, w.cd.y};
        const float inew = ((pab.y + pab.x) + pcd.y) + pcd.x;
        if constexpr (j + kResD < kResPPW) issue(j + kResD);
        const float r = t - inew;  // pdiff (odometer.cpp:381); visibility is applied to the patch sums below
        const f32x2_t gr = Gxy[j] * f32x2_t{r, r};
        acc.template push<j>(gr.x, gr.y, lane);
      });
#endif
      const float F = acc.F;
      RES_MARK(2)  // worker: stage 2
      RES_STAMP(tr_row, tr_it, 1)
      // ---- lane = (patch, A|B): its point's visibility and coefficients, then the six sums over the wave
      {
        const float val = F * lane_gather(vis_f, my_patch);  // 0 out of the new view (ind_new) and beyond the wave's points
        float o = 0.0f, v6[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) v6[k] = c6[k] * val;
        wave_sum6_dpp(v6);  // b_k = sum_patches cx_k A + cy_k B (odometer.cpp:386-404)
#pragma unroll
        for (int k = 0; k < 6; ++k) o = lane == k ? v6[k] : o;
        int lane_w = lane;  // (opaque copy: the LDS address is formed here, not kept in a register over the loop)
        asm volatile("" : "+v"(lane_w));
        if (lane < 6) sPart[wave][lane_w] = o;
      }
      __syncthreads();
      RES_MARK(3)  // worker: wave reduction + barrier
      RES_STAMP(tr_row, tr_it, 2)
      // ---- gather: the workgroup's six sums -> the pair's mailbox; then the broadcast
      seq += 1;
      const unsigned tag = xchg_tag(a.ex.tag0, seq);
      unsigned long long *gslot = gbox + res_gather_slot(seq, parts);
      const unsigned long long *bslot = bbox + res_bcast_slot(seq);
      if (wave == 0) {
        int lane_v = lane;  // (opaque copy: the two mailbox addresses are formed here, not kept in registers over the loop)
        asm volatile("" : "+v"(lane_v));
        float bs = 0.0f;
        if (lane < 6) bs = (sPart[0][lane] + sPart[1][lane]) + (sPart[2][lane] + sPart[3][lane]);
        if (lane < 6 && part + 1 != a.ex.mute)
          __hip_atomic_store(gslot + res_gather_row(part) + lane_v, xchg_pack(tag, bs), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long g = res_poll1(pc, lane < 13 ? bslot + lane_v : nullptr, tag, lane);
        // a time-out ends the pair in this workgroup (bounded time; the host reports the tracking as failed)
        if (lane < 13) sG[lane] = (lane == 12 && pc.dead) ? 0.0f : xchg_value(g);
        RES_MARK(4)  // worker (wave 0): gather store + waiting for the broadcast
        RES_STAMP(tr_row, tr_it, 3)
      }
#ifdef ICTR_RES_PROF
      tr_it += 1;
#endif
      __syncthreads();
      active = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, sG[12]));
    }
    RES_MARK(5)  // worker: pair prologue (template loads) -- charged at the next pair's end
    __syncthreads();  // sG and the records are rewritten for the next pair
  }
#ifdef ICTR_RES_PROF
  if (slot == a.prof_slot && part == 0 && tid == 0)
    for (int k = 0; k < 8; ++k) e.partH[k] = (float)tp_[k];
#endif
}

// ---------------------------------------------------------------- host side
#ifdef ICTR_RES_PROF
extern "C" int ictr_prof_res_trace(unsigned long long *out, int clear) {  // out[16][128][4]
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_res_trace), sizeof(g_res_trace)) != hipSuccess) return 1;
  if (clear) {
    static unsigned long long z[16][kTrIters][4];
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_res_trace), z, sizeof(z)) != hipSuccess) return 1;
  }
  return 0;
}
#endif
int resident_points_per_workgroup(int np) { return kResWaves * np; }
template <int NP>
static int res_occupancy() {
  int v = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, reinterpret_cast<const void *>(&k_level_resident<NP>),
                                                   kResThreads, 0) != hipSuccess) {
    (void)hipGetLastError();
    v = 0;
  }
  return v;
}
// workgroups of this kernel that one CU holds at once (0: the kernel cannot run)
int resident_blocks_per_cu(int np) {
  static const int n[2] = {res_occupancy<16>(), res_occupancy<32>()};
  return n[np == 32 ? 1 : 0];
}
hipError_t launch_level_resident(const EngineDev &e, const LevelCam &lc, int level, const ResidentGeom &g, int nblk,
                                 const Exchange &x, const ResXchg *xchg, hipStream_t s) {
  ResArgs a;
  if (xchg)
    a.x = *xchg;
  else
    memset(&a.x, 0, sizeof(a.x));
  {
    const char *ps = getenv("ICTR_RES_PROF_SLOT");
    a.prof_slot = ps ? atoi(ps) : 0;
  }
  a.nblk = nblk;
  a.lc = lc;
  a.level = level;
  a.parts = g.parts;
  a.slots = g.slots;
  a.ex = x;
  const dim3 grid((g.parts + 1) * g.slots), blk(kResThreads);
  if (g.np == 32)
    hipLaunchKernelGGL((k_level_resident<32>), grid, blk, 0, s, e, a);
  else
    hipLaunchKernelGGL((k_level_resident<16>), grid, blk, 0, s, e, a);
  return hipGetLastError();
}

}  // namespace ictr
