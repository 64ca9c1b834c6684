// ictr_stereotrack.hip -- the checked stereo track window (misc_src/run_test_OF_track.py:170-223) on the device
// (DESIGN.md §4 "Stereo track window"). The per-point arithmetic is ictr_stereotrack_hd.h; this file holds the field
// descriptor as a kernel reads it, the kernels and the C-ABI.
//
//   k_st_open       one thread per start point: frame 0 of st_open into column 0 of the history, the alive byte
//   k_st_advance    one thread per start point: a dead point returns at once; st_advance from column c-1 into column c
//   k_st_count      alive points per workgroup of kBlock start points
//   k_st_scan       one workgroup: the exclusive scan of those counts in workgroup order, and M
//   k_st_rows       start index of every survivor at offset(workgroup) + rank inside the workgroup (ballots, no atomics)
//   k_st_transpose  one thread per output element: [bsize][4][N] history -> the script's [M][4][bsize]
//
// The history is [bsize][4][N] f64, so every column read and write of a step is coalesced over the points; the order of
// the output depends on the start index alone. Everything is enqueued on the null stream.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <memory>
#include <utility>
#include <vector>

#include "ictr_dev.h"
#include "ictr_flowgrid_dev.h"
#include "ictr_launch.h"
#include "ictr_stereotrack_hd.h"

namespace ictr {

constexpr int kStScanBlock = 1024;
constexpr int kStMaxBsize = 256;
constexpr int64_t kStMaxPoints = (int64_t)1 << 24;

// a field descriptor on the device: plain memory (StMem) or a flow grid whose dense field is never formed
struct StField {
  StMem m;  // kinds plane and flow; for a grid m.w, m.h, m.x_only, m.sign are read as well
  FgDev g;
  int grid;
  __device__ __forceinline__ int width() const { return m.w; }
  __device__ __forceinline__ int height() const { return m.h; }
  __device__ __forceinline__ bool xonly() const { return grid ? m.x_only != 0 : m.xonly(); }
  __device__ __forceinline__ void taps(int x0, int y0, double *u, double *v) const {
    if (!grid) {
      m.taps(x0, y0, u, v);
      return;
    }
    float a[4], b[4];
    fg_value(g, x0 + 1, y0 + 1, &a[0], &b[0]);
    fg_value(g, x0, y0 + 1, &a[1], &b[1]);
    fg_value(g, x0 + 1, y0, &a[2], &b[2]);
    fg_value(g, x0, y0, &a[3], &b[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      u[k] = m.sign * (double)a[k];
      v[k] = m.sign * (double)b[k];
    }
  }
};

struct StArgs {
  double *hist;          // [bsize][4][n]
  unsigned char *alive;  // [n]
  const double *xy0;     // [n][2], or NULL: pixel i = (i % w, i / w)
  int n, w, col;
  double th_ratio, th_abs;
};

__global__ __launch_bounds__(kBlock) void k_st_open(StArgs a, StField lr, StField rl) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n) return;
  const double x = a.xy0 ? a.xy0[2 * (size_t)i] : (double)(i % a.w);
  const double y = a.xy0 ? a.xy0[2 * (size_t)i + 1] : (double)(i / a.w);
  double p[4];
  const bool ok = st_open(lr, rl, x, y, a.th_ratio, a.th_abs, p);
  a.alive[i] = ok ? 1 : 0;
  if (!ok) return;
  const size_t n = (size_t)a.n;
#pragma unroll
  for (int c = 0; c < 4; ++c) a.hist[c * n + i] = p[c];
}

__global__ __launch_bounds__(kBlock) void k_st_advance(StArgs a, StField l_fwd, StField l_bwd, StField r_fwd, StField r_bwd,
                                                       StField lr, StField rl) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n || !a.alive[i]) return;
  const size_t n = (size_t)a.n;
  const double *src = a.hist + (size_t)(a.col - 1) * 4 * n + i;
  double *dst = a.hist + (size_t)a.col * 4 * n + i;
  double p[4], q[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) p[c] = src[c * n];
  if (!st_advance(l_fwd, l_bwd, r_fwd, r_bwd, lr, rl, p, a.th_ratio, a.th_abs, q)) {
    a.alive[i] = 0;
    return;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) dst[c * n] = q[c];
}

// survivors of this workgroup's kBlock start points; *rank: this thread's place among them
__device__ __forceinline__ int st_block_rank(bool live, int *rank) {
  __shared__ int sW[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long b = __ballot(live);
  if (lane == 0) sW[wave] = __popcll(b);
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int k = 0; k < kWaves; ++k) {
    before += k < wave ? sW[k] : 0;
    total += sW[k];
  }
  *rank = before + __popcll(b & ((1ull << lane) - 1ull));
  return total;
}

__global__ __launch_bounds__(kBlock) void k_st_count(const unsigned char *__restrict__ alive, int n, int *__restrict__ counts) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  int rank;
  const int total = st_block_rank(i < n && alive[i], &rank);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// counts[nb] -> exclusive offsets in place, counts[nb] = M; chunks of kStScanBlock in order, a carry between them
__global__ __launch_bounds__(kStScanBlock) void k_st_scan(int *counts, int nb) {
  __shared__ int sS[kStScanBlock];
  __shared__ int sCarry;
  const int t = threadIdx.x;
  if (t == 0) sCarry = 0;
  __syncthreads();
  for (int base = 0; base < nb; base += kStScanBlock) {
    const int k = base + t;
    const int own = k < nb ? counts[k] : 0;
    sS[t] = own;
    __syncthreads();
    for (int s = 1; s < kStScanBlock; s <<= 1) {
      const int add = t >= s ? sS[t - s] : 0;
      __syncthreads();
      sS[t] += add;
      __syncthreads();
    }
    const int carry = sCarry;
    if (k < nb) counts[k] = carry + sS[t] - own;
    __syncthreads();
    if (t == kStScanBlock - 1) sCarry = carry + sS[t];
    __syncthreads();
  }
  if (t == 0) counts[nb] = sCarry;
}

__global__ __launch_bounds__(kBlock) void k_st_rows(const unsigned char *__restrict__ alive, int n,
                                                    const int *__restrict__ offsets, long long *__restrict__ rows) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < n && alive[i];
  int rank;
  st_block_rank(live, &rank);
  if (live) rows[(size_t)offsets[blockIdx.x] + rank] = i;
}

__global__ __launch_bounds__(kBlock) void k_st_transpose(const double *__restrict__ hist, const long long *__restrict__ rows,
                                                         size_t total, int n, int bsize, double *__restrict__ out) {
  const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= total) return;
  const size_t per = 4 * (size_t)bsize, m = e / per, r = e - m * per;
  const size_t c = r / (size_t)bsize, fr = r - c * (size_t)bsize;
  out[e] = hist[(fr * 4 + c) * (size_t)n + (size_t)rows[m]];
}

}  // namespace ictr

using namespace ictr;

// ---------------------------------------------------------------- host side
enum { kStIdle = 0, kStOpen = 1, kStCounted = 2 };

struct ictr_stereotrack {
  int w = 0, h = 0, bsize = 0;
  double th_ratio = 0, th_abs = 0;
  int n = 0, col = 0, state = kStIdle;
  size_t cap = 0;  // start points the window buffers hold
  int64_t m = 0;
  DevBuf<double> d_hist, d_xy0, d_out;
  DevBuf<unsigned char> d_alive;
  DevBuf<int> d_counts;  // [blocks + 1]
  DevBuf<long long> d_rows;
  DevBuf<float> stage[6];  // one step's host fields
  size_t out_cap = 0;
  PinBuf<int> h_m;
  bool timing = false;
  std::vector<std::pair<Event, Event>> tev[2];  // around the launches of the window: tracking, compaction
  float ms[2] = {0, 0};
  bool timed = false;
};

namespace {

struct StTimer {  // events around one group of launches when the object is timed
  ictr_stereotrack *t;
  int which;
  Event a, b;
  int begin() {
    if (!t->timing) return ICTR_OK;
    if (int rc = a.create()) return rc;
    if (int rc = b.create()) return rc;
    HIPCHK(hipEventRecord(a.get(), nullptr));
    return ICTR_OK;
  }
  int end() {
    if (!t->timing) return ICTR_OK;
    HIPCHK(hipEventRecord(b.get(), nullptr));
    t->tev[which].emplace_back(std::move(a), std::move(b));
    return ICTR_OK;
  }
};

int st_collect_times(ictr_stereotrack *t) {  // after a host wait
  for (int k = 0; k < 2; ++k) {
    for (auto &p : t->tev[k]) {
      float v = 0;
      HIPCHK(hipEventElapsedTime(&v, p.first.get(), p.second.get()));
      t->ms[k] += v;
    }
    t->tev[k].clear();
  }
  return ICTR_OK;
}

// descriptor -> kernel argument; a host field is copied to stage[slot] before this returns (the copy waits for the step
// that read the slot last)
int st_field(ictr_stereotrack *t, const ictr_field *f, int slot, bool want_xonly, const char *what, StField *out) {
  if (!f || !f->data) return fail(ICTR_ERR_INVALID, "%s: a field (or its data) is NULL", what);
  if (f->sign != 1 && f->sign != -1) return fail(ICTR_ERR_INVALID, "%s: a field's sign is %d (+1 or -1)", what, f->sign);
  memset(out, 0, sizeof(*out));
  out->m.w = t->w;
  out->m.h = t->h;
  out->m.sign = (double)f->sign;
  out->m.x_only = f->x_only != 0;
  if (f->kind == ICTR_FIELD_GRID) {
    if (int rc = ictr_flowgrid_view_(static_cast<const ictr_flowgrid *>(f->data), &out->g)) return rc;
    if (out->g.w != t->w || out->g.h != t->h)
      return fail(ICTR_ERR_INVALID, "%s: the flow grid is %d x %d, the window %d x %d", what, out->g.w, out->g.h, t->w, t->h);
    out->grid = 1;
    out->m.comps = 2;
  } else if (f->kind == ICTR_FIELD_PLANE || f->kind == ICTR_FIELD_FLOW) {
    out->m.comps = f->kind == ICTR_FIELD_PLANE ? 1 : 2;
    const size_t bytes = sizeof(float) * (size_t)out->m.comps * (size_t)t->w * (size_t)t->h;
    if (f->on_device) {
      out->m.p = static_cast<const float *>(f->data);
    } else {
      if (!t->stage[slot])
        if (int rc = t->stage[slot].alloc(sizeof(float) * 2 * (size_t)t->w * (size_t)t->h)) return rc;
      HIPCHK(hipMemcpy(t->stage[slot].get(), f->data, bytes, hipMemcpyHostToDevice));
      out->m.p = t->stage[slot].get();
    }
  } else {
    return fail(ICTR_ERR_INVALID, "%s: field kind %d (ICTR_FIELD_PLANE, _FLOW or _GRID)", what, f->kind);
  }
  const bool xonly = out->grid ? out->m.x_only != 0 : out->m.xonly();
  if (xonly != want_xonly)
    return fail(ICTR_ERR_INVALID, want_xonly ? "%s: the stereo fields move x only (a plane, or x_only set)"
                                             : "%s: the temporal flows have two components (a flow or a grid, x_only clear)",
                what);
  return ICTR_OK;
}

StArgs st_args(const ictr_stereotrack *t) {
  StArgs a;
  memset(&a, 0, sizeof(a));
  a.hist = t->d_hist.get();
  a.alive = t->d_alive.get();
  a.n = t->n;
  a.w = t->w;
  a.col = t->col;
  a.th_ratio = t->th_ratio;
  a.th_abs = t->th_abs;
  return a;
}

int st_blocks(const ictr_stereotrack *t) { return (t->n + kBlock - 1) / kBlock; }

}  // namespace

extern "C" int ictr_stereotrack_create(ictr_stereotrack **out, int w, int h, int bsize, double th_ratio, double th_abs) {
  if (!out) return fail(ICTR_ERR_INVALID, "stereotrack_create: NULL argument");
  if (w < 2 || h < 2 || w > 32768 || h > 32768) return fail(ICTR_ERR_INVALID, "stereotrack_create: %d x %d (2 .. 32768)", w, h);
  if (bsize < 1 || bsize > kStMaxBsize) return fail(ICTR_ERR_INVALID, "stereotrack_create: bsize %d (1 .. %d)", bsize, kStMaxBsize);
  if (int rc = need_device()) return rc;
  auto t = std::make_unique<ictr_stereotrack>();
  t->w = w;
  t->h = h;
  t->bsize = bsize;
  t->th_ratio = th_ratio;
  t->th_abs = th_abs;
  if (int rc = t->h_m.alloc(sizeof(int))) return rc;
  *out = t.release();
  return ICTR_OK;
}

extern "C" void ictr_stereotrack_destroy(ictr_stereotrack *t) {
  if (t) (void)hipStreamSynchronize(nullptr);  // nothing in flight reads what goes now
  delete t;
}

extern "C" int ictr_stereotrack_open(ictr_stereotrack *t, const double *xy0, int64_t n, const ictr_field *lr,
                                     const ictr_field *rl) {
  if (!t) return fail(ICTR_ERR_INVALID, "stereotrack is NULL");
  const int64_t npix = (int64_t)t->w * t->h;
  if (!xy0 && n == 0) n = npix;
  if (!xy0 && n != npix) return fail(ICTR_ERR_INVALID, "stereotrack_open: every pixel is %lld points, not %lld", (long long)npix, (long long)n);
  if (n < 1 || n > kStMaxPoints) return fail(ICTR_ERR_INVALID, "stereotrack_open: %lld points (1 .. 2^24)", (long long)n);
  t->state = kStIdle;
  StField flr, frl;
  if (int rc = st_field(t, lr, 0, true, "stereotrack_open", &flr)) return rc;
  if (int rc = st_field(t, rl, 1, true, "stereotrack_open", &frl)) return rc;
  if ((size_t)n > t->cap) {
    t->cap = 0;
    HIPCHK(hipStreamSynchronize(nullptr));  // the previous window's kernels are done with what goes now
    const size_t N = (size_t)n, nb = (N + kBlock - 1) / kBlock;
    if (int rc = t->d_hist.alloc(sizeof(double) * 4 * (size_t)t->bsize * N)) return rc;
    if (int rc = t->d_alive.alloc(N)) return rc;
    if (int rc = t->d_counts.alloc(sizeof(int) * (nb + 1))) return rc;
    if (int rc = t->d_rows.alloc(sizeof(long long) * N)) return rc;
    if (int rc = t->d_xy0.alloc(sizeof(double) * 2 * N)) return rc;
    t->cap = N;
  }
  t->n = (int)n;
  t->col = 0;
  t->ms[0] = t->ms[1] = 0;
  t->tev[0].clear();
  t->tev[1].clear();
  t->timed = t->timing;
  StArgs a = st_args(t);
  if (xy0) {
    HIPCHK(hipMemcpy(t->d_xy0.get(), xy0, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice));
    a.xy0 = t->d_xy0.get();
  }
  StTimer tm{t, 0};
  if (int rc = tm.begin()) return rc;
  hipLaunchKernelGGL(k_st_open, dim3(st_blocks(t)), dim3(kBlock), 0, nullptr, a, flr, frl);
  HIPCHK(hipGetLastError());
  if (int rc = tm.end()) return rc;
  t->state = kStOpen;
  return ICTR_OK;
}

extern "C" int ictr_stereotrack_advance(ictr_stereotrack *t, const ictr_field *l_fwd, const ictr_field *l_bwd,
                                        const ictr_field *r_fwd, const ictr_field *r_bwd, const ictr_field *lr_next,
                                        const ictr_field *rl_next) {
  if (!t) return fail(ICTR_ERR_INVALID, "stereotrack is NULL");
  if (t->state != kStOpen) return fail(ICTR_ERR_STATE, "stereotrack_advance: open comes first");
  if (t->col + 1 >= t->bsize)
    return fail(ICTR_ERR_STATE, "stereotrack_advance: the window of %d frames is full", t->bsize);
  const ictr_field *in[6] = {l_fwd, l_bwd, r_fwd, r_bwd, lr_next, rl_next};
  StField f[6];
  for (int k = 0; k < 6; ++k)
    if (int rc = st_field(t, in[k], k, k >= 4, "stereotrack_advance", &f[k])) return rc;
  t->col += 1;
  const StArgs a = st_args(t);
  StTimer tm{t, 0};
  if (int rc = tm.begin()) return rc;
  hipLaunchKernelGGL(k_st_advance, dim3(st_blocks(t)), dim3(kBlock), 0, nullptr, a, f[0], f[1], f[2], f[3], f[4], f[5]);
  HIPCHK(hipGetLastError());
  return tm.end();
}

extern "C" int ictr_stereotrack_count(ictr_stereotrack *t, int64_t *m) {
  if (!t || !m) return fail(ICTR_ERR_INVALID, "stereotrack_count: NULL argument");
  if (t->state != kStOpen || t->col + 1 != t->bsize)
    return fail(ICTR_ERR_STATE, "stereotrack_count: open and %d advances come first", t->bsize - 1);
  const int nb = st_blocks(t);
  StTimer tm{t, 1};
  if (int rc = tm.begin()) return rc;
  hipLaunchKernelGGL(k_st_count, dim3(nb), dim3(kBlock), 0, nullptr, t->d_alive.get(), t->n, t->d_counts.get());
  hipLaunchKernelGGL(k_st_scan, dim3(1), dim3(kStScanBlock), 0, nullptr, t->d_counts.get(), nb);
  hipLaunchKernelGGL(k_st_rows, dim3(nb), dim3(kBlock), 0, nullptr, t->d_alive.get(), t->n, t->d_counts.get(),
                     t->d_rows.get());
  HIPCHK(hipGetLastError());
  if (int rc = tm.end()) return rc;
  HIPCHK(hipMemcpyAsync(t->h_m.get(), t->d_counts.get() + nb, sizeof(int), hipMemcpyDeviceToHost, nullptr));
  HIPCHK(hipStreamSynchronize(nullptr));
  if (int rc = st_collect_times(t)) return rc;
  t->m = *t->h_m.get();
  if (t->m < 0 || t->m > t->n) return fail(ICTR_ERR_HIP, "stereotrack_count: the device counted %lld of %d points", (long long)t->m, t->n);
  *m = t->m;
  t->state = kStCounted;
  return ICTR_OK;
}

extern "C" int ictr_stereotrack_read(ictr_stereotrack *t, double *xy_t, int64_t *rows) {
  if (!t) return fail(ICTR_ERR_INVALID, "stereotrack is NULL");
  if (t->state != kStCounted) return fail(ICTR_ERR_STATE, "stereotrack_read: count comes first");
  const size_t M = (size_t)t->m, total = M * 4 * (size_t)t->bsize;
  if (M > 0 && xy_t) {
    if (total > t->out_cap) {
      t->out_cap = 0;
      if (int rc = t->d_out.alloc(sizeof(double) * total)) return rc;
      t->out_cap = total;
    }
    StTimer tm{t, 1};
    if (int rc = tm.begin()) return rc;
    hipLaunchKernelGGL(k_st_transpose, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr,
                       t->d_hist.get(), t->d_rows.get(), total, t->n, t->bsize, t->d_out.get());
    HIPCHK(hipGetLastError());
    if (int rc = tm.end()) return rc;
    HIPCHK(hipMemcpy(xy_t, t->d_out.get(), sizeof(double) * total, hipMemcpyDeviceToHost));
    if (int rc = st_collect_times(t)) return rc;
  }
  if (M > 0 && rows) HIPCHK(hipMemcpy(rows, t->d_rows.get(), sizeof(int64_t) * M, hipMemcpyDeviceToHost));
  return ICTR_OK;
}

extern "C" int ictr_stereotrack_view_(const ictr_stereotrack *t, ictr_stereotrack_view *v) {
  v->hist = t->d_hist.get();
  v->rows = t->d_rows.get();
  v->n = t->n;
  v->bsize = t->bsize;
  v->counted = t->state == kStCounted;
  v->m = t->m;
  return ICTR_OK;
}

extern "C" int ictr_stereotrack_set_timing(ictr_stereotrack *t, int on) {
  if (!t) return fail(ICTR_ERR_INVALID, "stereotrack is NULL");
  if (t->state == kStOpen) return fail(ICTR_ERR_STATE, "stereotrack_set_timing: a window is open; count and read it first");
  t->timing = on != 0;
  return ICTR_OK;
}

extern "C" int ictr_stereotrack_get_kernel_times(const ictr_stereotrack *t, float *ms) {
  if (!t || !ms) return fail(ICTR_ERR_INVALID, "stereotrack_get_kernel_times: NULL argument");
  if (t->state != kStCounted || !t->timed) return fail(ICTR_ERR_STATE, "stereotrack_get_kernel_times: no completed timed window");
  memcpy(ms, t->ms, sizeof(t->ms));
  return ICTR_OK;
}
