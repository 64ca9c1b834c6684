// ictr_frontend.hip -- the point-track front end on the device: corners, flow grid, track window (DESIGN.md §4 "Point-track
// front end"). Everything here restates host code of the package bit for bit:
//   patchflow.good_features            -> k_gf_response / k_gf_cells / k_gf_select / k_gf_compact / k_gf_rank
//   patchflow.dense_flow's fill + bilinear up-sampling -> k_fg_nodes / k_fg_diff / k_fg_rowfill / k_fg_colfill, fg_value()
//   classoftrack.func_get_transf_position on that field -> fg_gather() (the field is never formed), k_fg_gather, k_fg_dense
//   classoftrack.oftrack.addframe      -> k_pt_open / k_pt_advance on a ring of block slots
// All float64 arithmetic is written in the host code's operation order; the library is built with -ffp-contract=off, and /
// and sqrt on doubles are the correctly rounded sequences, so the results carry NumPy's bits.
//
// The host decides no launch from device data: corner counts stay in device memory and the kernels read them there.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "ictr_dev.h"
#include "ictr_flowgrid_dev.h"
#include "ictr_launch.h"

namespace ictr {

// ---------------------------------------------------------------- corner picker
constexpr int kGfTW = 32, kGfTH = 16;  // response tile (outputs) of one workgroup
constexpr int kGfSelBlock = 1024;
constexpr size_t kGfMaxLds = 64 * 1024;

struct GfCtl {
  unsigned long long maxbits;  // bits of max(lam) (lam >= 0 there: the border is 0)
  unsigned long long thr;      // key of the maxcorners-th strongest cell winner (0: every winner survives)
  int nsurv;                   // survivors in the list (key >= thr)
  int pad;
};

static size_t gf_lds_bytes(int win) {
  const size_t ph = kGfTH + 2 * win, pw = kGfTW + 2 * win;
  return sizeof(double) * 3 * (ph * pw + ph * kGfTW);
}

// lam = smaller eigenvalue of the (2 win + 1)^2 zero-padded window sums of [gx^2 gx gy; gx gy gy^2], float64, central
// differences (0 in the first / last column / row); window sums separable: rows (dx ascending) first, then columns (dy
// ascending). lam = 0 in the outer `mindist` rows and columns. The block maximum goes to ctl->maxbits by an unsigned max.
__global__ __launch_bounds__(kBlock) void k_gf_response(const float *__restrict__ img, int stride, int W, int H, int win,
                                                        int mindist, double *__restrict__ lam, GfCtl *ctl) {
  extern __shared__ __attribute__((aligned(16))) char gf_smem[];
  const int PH = kGfTH + 2 * win, PW = kGfTW + 2 * win;
  double *P = reinterpret_cast<double *>(gf_smem);  // [3][PH][PW] products
  double *R = P + 3 * PH * PW;                      // [3][PH][TW] row sums
  const int x0 = blockIdx.x * kGfTW, y0 = blockIdx.y * kGfTH;
  const int tid = threadIdx.x;
  for (int e = tid; e < PH * PW; e += kBlock) {
    const int ly = e / PW, lx = e - ly * PW;
    const int X = x0 - win + lx, Y = y0 - win + ly;
    double gx = 0.0, gy = 0.0;
    if (X >= 0 && X < W && Y >= 0 && Y < H) {
      const float *p = img + (size_t)Y * stride + X;
      if (X >= 1 && X <= W - 2) gx = (double)p[1] - (double)p[-1];
      if (Y >= 1 && Y <= H - 2) gy = (double)p[stride] - (double)p[-stride];
    }
    P[e] = gx * gx;
    P[PH * PW + e] = gx * gy;
    P[2 * PH * PW + e] = gy * gy;
  }
  __syncthreads();
  for (int e = tid; e < PH * kGfTW; e += kBlock) {
    const int ly = e / kGfTW, lx = e - ly * kGfTW;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double *row = P + c * PH * PW + ly * PW + lx;
      double s = 0.0;
      for (int d = 0; d <= 2 * win; ++d) s += row[d];
      R[c * PH * kGfTW + e] = s;
    }
  }
  __syncthreads();
  double m = 0.0;
  for (int e = tid; e < kGfTH * kGfTW; e += kBlock) {
    const int ly = e / kGfTW, lx = e - ly * kGfTW;
    const int X = x0 + lx, Y = y0 + ly;
    if (X >= W || Y >= H) continue;
    double s[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double *col = R + c * PH * kGfTW + ly * kGfTW + lx;
      double a = 0.0;
      for (int d = 0; d <= 2 * win; ++d) a += col[d * kGfTW];
      s[c] = a;
    }
    const double sxx = s[0], sxy = s[1], syy = s[2];
    const double df = sxx - syy;
    double v = 0.5 * (sxx + syy) - sqrt(0.25 * (df * df) + sxy * sxy);
    if (X < mindist || X >= W - mindist || Y < mindist || Y >= H - mindist) v = 0.0;
    lam[(size_t)Y * W + X] = v;
    if (v > m) m = v;
  }
  __syncthreads();  // P is free: the workgroup's maximum
  P[tid] = m;
  __syncthreads();
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if (tid < o && P[tid + o] > P[tid]) P[tid] = P[tid + o];
    __syncthreads();
  }
  if (tid == 0 && P[0] > 0.0) atomicMax(&ctl->maxbits, (unsigned long long)__double_as_longlong(P[0]));
}

// one thread per mindist x mindist cell: its candidate (lam > thr, lam >= each neighbour inside the image) with the largest
// lam, ties to the smallest y W + x (the scan order). key = bits of that lam (> 0), 0 for a cell without a candidate
__global__ __launch_bounds__(kBlock) void k_gf_cells(const double *__restrict__ lam, int W, int H, int mindist, double quality,
                                                     const GfCtl *ctl, int ncx, int ncells,
                                                     unsigned long long *__restrict__ key, int *__restrict__ idx) {
  const int c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= ncells) return;
  const double thr = quality * __longlong_as_double((long long)ctl->maxbits);
  const int cy = c / ncx, cx = c - cy * ncx;
  const int ys = cy * mindist, xs = cx * mindist;
  const int ye = min(ys + mindist, H), xe = min(xs + mindist, W);
  double best = 0.0;
  int bi = -1;
  for (int y = ys; y < ye; ++y)
    for (int x = xs; x < xe; ++x) {
      const double v = lam[(size_t)y * W + x];
      if (!(v > thr) || !(v > best)) continue;
      bool ismax = true;
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int yy = y + dy, xx = x + dx;
          if ((dy | dx) == 0 || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;  // outside counts as -1 < v
          ismax &= v >= lam[(size_t)yy * W + xx];
        }
      if (ismax) {
        best = v;
        bi = y * W + x;
      }
    }
  key[c] = bi >= 0 ? (unsigned long long)__double_as_longlong(best) : 0ull;
  idx[c] = bi;
}

// one workgroup: radix select (8 passes of 8 bits, most significant first) of the maxcorners-th largest key. Writes the
// threshold key (0 when there are no more than maxcorners winners), the corner count min(winners, maxcorners) to *count and
// clears the survivor counter.
__global__ __launch_bounds__(kGfSelBlock) void k_gf_select(const unsigned long long *__restrict__ key, int ncells,
                                                           int maxcorners, GfCtl *ctl, int *count) {
  __shared__ unsigned hist[256];
  __shared__ unsigned long long s_prefix;
  __shared__ unsigned s_k;
  __shared__ int s_done;
  const int tid = threadIdx.x;
  if (tid == 0) {
    s_prefix = 0;
    s_k = (unsigned)maxcorners;
    s_done = 0;
  }
  for (int pass = 7; pass >= 0; --pass) {
    const int shift = 8 * pass;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    const unsigned long long prefix = s_prefix;
    for (int i = tid; i < ncells; i += kGfSelBlock) {
      const unsigned long long k = key[i];
      if (k == 0) continue;
      if (pass < 7 && (k >> (shift + 8)) != (prefix >> (shift + 8))) continue;
      atomicAdd(&hist[(unsigned)(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned total = 0;
      for (int d = 0; d < 256; ++d) total += hist[d];
      if (pass == 7 && total <= (unsigned)maxcorners) {  // every winner is a corner
        ctl->thr = 0;
        *count = (int)total;
        s_done = 1;
      } else {
        unsigned cum = 0, k = s_k;
        int d = 255;
        for (; d > 0; --d) {
          if (cum + hist[d] >= k) break;
          cum += hist[d];
        }
        s_k = k - cum;
        s_prefix = prefix | ((unsigned long long)d << shift);
      }
    }
    __syncthreads();
    if (s_done) break;
  }
  if (tid == 0) {
    if (!s_done) {
      ctl->thr = s_prefix;
      *count = maxcorners;
    }
    ctl->nsurv = 0;
  }
}

// the winners with key >= thr, in any order (their ranks do not depend on it)
__global__ __launch_bounds__(kBlock) void k_gf_compact(const unsigned long long *__restrict__ key, const int *__restrict__ idx,
                                                       int ncells, GfCtl *ctl, unsigned long long *__restrict__ lkey,
                                                       int *__restrict__ lidx) {
  const int c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= ncells) return;
  const unsigned long long k = key[c];
  if (k == 0 || k < ctl->thr) return;
  const int slot = atomicAdd(&ctl->nsurv, 1);  // < ncells: the list has ncells entries
  lkey[slot] = k;
  lidx[slot] = idx[c];
}

// rank of a survivor = survivors that precede it (lam descending, then index ascending); rank < maxcorners: out[rank]
__global__ __launch_bounds__(kBlock) void k_gf_rank(const unsigned long long *__restrict__ lkey, const int *__restrict__ lidx,
                                                    const GfCtl *ctl, int maxcorners, int W, float *__restrict__ out) {
  __shared__ unsigned long long sk[kBlock];
  __shared__ int si[kBlock];
  const int n = ctl->nsurv;
  for (int base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {  // uniform per workgroup
    const int i = base + threadIdx.x;
    const bool have = i < n;
    const unsigned long long k = have ? lkey[i] : 0ull;
    const int id = have ? lidx[i] : 0;
    int rank = 0;
    for (int t0 = 0; t0 < n; t0 += kBlock) {
      __syncthreads();
      const int j = t0 + threadIdx.x;
      sk[threadIdx.x] = j < n ? lkey[j] : 0ull;  // key 0 precedes nothing
      si[threadIdx.x] = j < n ? lidx[j] : 0;
      __syncthreads();
      const int m = min(kBlock, n - t0);
      for (int q = 0; q < m; ++q) rank += (sk[q] > k) | ((sk[q] == k) & (si[q] < id));
    }
    if (have && rank < maxcorners) {
      const int y = id / W, x = id - y * W;
      out[2 * rank] = (float)x;
      out[2 * rank + 1] = (float)y;
    }
  }
}

struct GfWork {
  int w = 0, h = 0, mindist = 0, win = 0, ncx = 0, ncells = 0;
  DevBuf<double> lam;
  DevBuf<unsigned long long> key, lkey;
  DevBuf<int> idx, lidx;
  DevBuf<GfCtl> ctl;
};

static int gf_alloc(GfWork *g, int w, int h, int mindist, int win) {
  if (w < 1 || h < 1 || mindist < 1 || win < 0) return fail(ICTR_ERR_INVALID, "good_features: needs mindist >= 1 and win >= 0");
  if ((int64_t)w * h > (int64_t)1 << 30) return fail(ICTR_ERR_INVALID, "good_features: the image is too large");
  if (gf_lds_bytes(win) > kGfMaxLds)
    return fail(ICTR_ERR_INVALID, "good_features: win = %d needs more than 64 KiB of LDS per tile (win <= 8)", win);
  g->w = w;
  g->h = h;
  g->mindist = mindist;
  g->win = win;
  g->ncx = (w + mindist - 1) / mindist;
  g->ncells = g->ncx * ((h + mindist - 1) / mindist);
  const size_t nc = (size_t)g->ncells;
  if (int rc = g->lam.alloc(sizeof(double) * (size_t)w * h)) return rc;
  if (int rc = g->key.alloc(sizeof(unsigned long long) * nc)) return rc;
  if (int rc = g->lkey.alloc(sizeof(unsigned long long) * nc)) return rc;
  if (int rc = g->idx.alloc(sizeof(int) * nc)) return rc;
  if (int rc = g->lidx.alloc(sizeof(int) * nc)) return rc;
  return g->ctl.alloc(sizeof(GfCtl));
}

// corners of the plane img (stride floats per row) -> out[maxcorners][2] (rows past the count are left as they are) and
// *count, both in device memory
static int gf_run(const GfWork &g, const float *img, int stride, int maxcorners, double quality, float *out, int *count,
                  hipStream_t s) {
  double *lam = g.lam.get();
  unsigned long long *key = g.key.get(), *lkey = g.lkey.get();
  int *idx = g.idx.get(), *lidx = g.lidx.get();
  GfCtl *ctl = g.ctl.get();
  HIPCHK(hipMemsetAsync(ctl, 0, sizeof(GfCtl), s));
  const dim3 tiles((g.w + kGfTW - 1) / kGfTW, (g.h + kGfTH - 1) / kGfTH);
  hipLaunchKernelGGL(k_gf_response, tiles, dim3(kBlock), gf_lds_bytes(g.win), s, img, stride, g.w, g.h, g.win, g.mindist, lam,
                     ctl);
  const dim3 cg((g.ncells + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(k_gf_cells, cg, dim3(kBlock), 0, s, lam, g.w, g.h, g.mindist, quality, ctl, g.ncx, g.ncells, key, idx);
  hipLaunchKernelGGL(k_gf_select, dim3(1), dim3(kGfSelBlock), 0, s, key, g.ncells, maxcorners, ctl, count);
  hipLaunchKernelGGL(k_gf_compact, cg, dim3(kBlock), 0, s, key, idx, g.ncells, ctl, lkey, lidx);
  const int rg = std::max(1, std::min((std::min(g.ncells, maxcorners) + kBlock - 1) / kBlock, 256));
  hipLaunchKernelGGL(k_gf_rank, dim3(rg), dim3(kBlock), 0, s, lkey, lidx, ctl, maxcorners, g.w, out);
  HIPCHK(hipGetLastError());
  return ICTR_OK;
}

// ---------------------------------------------------------------- flow grid
// FgDev, fg_value, fg_gather: ictr_flowgrid_dev.h

__global__ __launch_bounds__(kBlock) void k_fg_nodes(float *__restrict__ pts, int nx, int K, int step) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= K) return;
  const int j = k / nx, i = k - j * nx;
  pts[k] = (float)(step / 2 + i * step);
  pts[k + K] = (float)(step / 2 + j * step);
}
__global__ __launch_bounds__(kBlock) void k_fg_diff(const float *__restrict__ pts, const float *__restrict__ out,
                                                    const int *__restrict__ status, int K, float *__restrict__ draw,
                                                    unsigned char *__restrict__ lost) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= K) return;
  draw[2 * k] = out[k] - pts[k];
  draw[2 * k + 1] = out[k + K] - pts[k + K];
  lost[k] = status[k] ? 0 : 1;
}
// The fill runs on 1 .. kSetMax grids of one geometry at once (DESIGN.md §4 "Lockstep sets"; a grid's own fill is a set
// of one): member blockIdx.y's node buffers, and its ny rows of the rowhas block.
struct FgFillArgs {
  const float *draw[kSetMax];
  const unsigned char *lost[kSetMax];
  float *d[kSetMax];
  int *rowhas;  // [n][ny]
};
// a lost node takes the nearest tracked node to its left in its row, else the nearest to its right; rowhas[y] = the row has
// a tracked node (cleared before the launch). Nodes of a row without one are left for k_fg_colfill.
__global__ __launch_bounds__(kBlock) void k_fg_rowfill(FgFillArgs a, int nx, int ny, int K) {
  const int m = blockIdx.y;
  const float *__restrict__ draw = a.draw[m];
  const unsigned char *__restrict__ lost = a.lost[m];
  float *__restrict__ d = a.d[m];
  int *__restrict__ rowhas = a.rowhas + (size_t)m * ny;
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= K) return;
  const int j = k / nx, i = k - j * nx;
  const unsigned char *lr = lost + (size_t)j * nx;
  int src = -1;
  for (int q = i; q >= 0 && src < 0; --q)
    if (!lr[q]) src = q;
  for (int q = i + 1; q < nx && src < 0; ++q)
    if (!lr[q]) src = q;
  if (src < 0) return;
  d[2 * k] = draw[2 * (j * nx + src)];
  d[2 * k + 1] = draw[2 * (j * nx + src) + 1];
  if (src == i) rowhas[j] = 1;
}
// a row without a tracked node takes, node by node, the nearest row above that has one, else the nearest below, else 0
__global__ __launch_bounds__(kBlock) void k_fg_colfill(FgFillArgs a, int nx, int ny, int K) {
  const int m = blockIdx.y;
  float *__restrict__ d = a.d[m];
  const int *__restrict__ rowhas = a.rowhas + (size_t)m * ny;
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= K) return;
  const int j = k / nx, i = k - j * nx;
  if (rowhas[j]) return;
  int src = -1;
  for (int q = j - 1; q >= 0 && src < 0; --q)
    if (rowhas[q]) src = q;
  for (int q = j + 1; q < ny && src < 0; ++q)
    if (rowhas[q]) src = q;
  d[2 * k] = src >= 0 ? d[2 * (src * nx + i)] : 0.0f;  // rows that have a tracked node are not written by this launch
  d[2 * k + 1] = src >= 0 ? d[2 * (src * nx + i) + 1] : 0.0f;
}
__global__ __launch_bounds__(kBlock) void k_fg_gather(FgDev g, const double *__restrict__ xy, int K, double *__restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= K) return;
  double ox, oy;
  fg_gather(g, xy[2 * i], xy[2 * i + 1], &ox, &oy);
  out[2 * i] = ox;
  out[2 * i + 1] = oy;
}
__global__ __launch_bounds__(kBlock) void k_fg_dense(FgDev g, float2 *__restrict__ out) {
  const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * kWaves + (threadIdx.x >> 6);
  if (X >= g.w || Y >= g.h) return;
  float u, v;
  fg_value(g, X, Y, &u, &v);
  out[(size_t)Y * g.w + X] = make_float2(u, v);
}
void launch_fg_dense(const FgDev &g, float2 *out, hipStream_t s) {
  hipLaunchKernelGGL(k_fg_dense, pixel_rows_grid(g.w, g.h), dim3(kBlock), 0, s, g, out);
}

// ---------------------------------------------------------------- track window
// one block slot: absmovement f64 [mc] | tracks f32 [mc][2][bsize] | count i32 (+ 4 bytes) | valid u8 [mc]
struct PtSlot {
  double *absmov;
  float *tracks;
  int *count;
  unsigned char *valid;
};
struct PtGeom {
  int mc, bsize;
  size_t off_tracks, off_count, off_valid, bytes;
};
static PtGeom pt_geom(int mc, int bsize) {
  PtGeom g;
  g.mc = mc;
  g.bsize = bsize;
  g.off_tracks = sizeof(double) * (size_t)mc;
  g.off_count = g.off_tracks + sizeof(float) * 2 * (size_t)mc * bsize;
  g.off_valid = g.off_count + 8;
  g.bytes = (g.off_valid + (size_t)mc + 15) / 16 * 16;
  return g;
}
template <typename B>
static PtSlot pt_slot(B *base, const PtGeom &g) {
  char *p = (char *)base;
  return PtSlot{reinterpret_cast<double *>(p), reinterpret_cast<float *>(p + g.off_tracks),
                reinterpret_cast<int *>(p + g.off_count), reinterpret_cast<unsigned char *>(p + g.off_valid)};
}

// a new block: column 0 = the corners (already written to tracks[i][.][0]'s staging `corners`), every other column NaN
__global__ __launch_bounds__(kBlock) void k_pt_open(PtSlot s, const float *__restrict__ corners, int mc, int bsize) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= mc) return;
  const bool have = i < *s.count;
  const float nanv = __int_as_float(0x7fc00000);
  float *t = s.tracks + (size_t)i * 2 * bsize;
  for (int c = 0; c < 2 * bsize; ++c) t[c] = nanv;
  if (have) {
    t[0] = corners[2 * i];
    t[bsize] = corners[2 * i + 1];
  }
  s.valid[i] = have ? 1 : 0;
  s.absmov[i] = 0.0;
}

// oftrack.addframe for the live points of one block: column col -> col + 1
__global__ __launch_bounds__(kBlock) void k_pt_advance(PtSlot s, int bsize, int col, FgDev fw, FgDev bw, double th_ratio,
                                                       double th_abs) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= *s.count || !s.valid[i]) return;
  float *t = s.tracks + (size_t)i * 2 * bsize;
  const double xl = (double)t[col], yl = (double)t[bsize + col];
  double xf, yf, xb, yb;
  fg_gather(fw, xl, yl, &xf, &yf);
  fg_gather(bw, xf, yf, &xb, &yb);
  const double ex = xl - xb, ey = yl - yb;
  const double fb = sqrt(ex * ex + ey * ey);
  const double mx = xl - xf, my = yl - yf;
  const double mv = sqrt(mx * mx + my * my);
  const bool ok = (fb / mv < th_ratio) & (fb < th_abs);  // NaN compares false
  if (!ok) xf = yf = __builtin_nan("");
  t[col + 1] = (float)xf;
  t[bsize + col + 1] = (float)yf;
  const double ax = (double)t[0] - xf, ay = (double)t[bsize] - yf;
  s.absmov[i] = sqrt(ax * ax + ay * ay);
  s.valid[i] = ((xf == xf) | (yf == yf)) ? 1 : 0;
}

}  // namespace ictr

using namespace ictr;

// ================================================================ C-ABI
extern "C" int ictr_good_features(const ictr_pyramid *pyr, const float *img, int w, int h, int maxcorners, double quality,
                                  int mindist, int win, float *out_xy, int *out_count) {
  if ((!pyr && !img) || maxcorners < 1 || !out_count || !out_xy)
    return fail(ICTR_ERR_INVALID, "good_features: bad arguments (a pyramid or an image, maxcorners >= 1)");
  if (int rc = need_device()) return rc;
  ictr_level0 l0{nullptr, w, w, h};  // a host image is staged below, rows of w
  if (pyr) {
    if (int rc = ictr_pyramid_level0(pyr, "good_features", &l0)) return rc;
  } else if (w < 1 || h < 1) {
    return fail(ICTR_ERR_INVALID, "good_features: bad image size");
  }
  GfWork g;
  if (int rc = gf_alloc(&g, l0.w, l0.h, mindist, win)) return rc;
  DevBuf<float> stage, d_out;
  if (!pyr) {
    if (int rc = stage.alloc(sizeof(float) * (size_t)w * h)) return rc;
    HIPCHK(hipMemcpy(stage.get(), img, sizeof(float) * (size_t)w * h, hipMemcpyHostToDevice));
    l0.img = stage.get();
  }
  if (int rc = d_out.alloc(sizeof(float) * 2 * (size_t)maxcorners + sizeof(int))) return rc;
  int *d_count = reinterpret_cast<int *>(d_out.get() + 2 * (size_t)maxcorners);
  if (int rc = gf_run(g, l0.img, l0.stride, maxcorners, quality, d_out.get(), d_count, nullptr)) return rc;
  HIPCHK(hipMemcpy(out_count, d_count, sizeof(int), hipMemcpyDeviceToHost));
  if (*out_count > 0) HIPCHK(hipMemcpy(out_xy, d_out.get(), sizeof(float) * 2 * (size_t)*out_count, hipMemcpyDeviceToHost));
  return ICTR_OK;
}

struct ictr_flowgrid {
  int w = 0, h = 0, step = 0, nx = 0, ny = 0, K = 0;
  int filled = 0;  // d holds a field
  float *pts = nullptr, *out = nullptr, *draw = nullptr, *d = nullptr;
  int *status = nullptr, *iters = nullptr, *rowhas = nullptr;
  unsigned char *lost = nullptr;
  DevBuf<char> arena;  // everything above
};
static FgDev fg_dev(const ictr_flowgrid *g) { return FgDev{g->d, g->nx, g->ny, g->step, g->w, g->h}; }
extern "C" int ictr_flowgrid_view_(const ictr_flowgrid *g, FgDev *v) {
  if (!g || !v) return fail(ICTR_ERR_INVALID, "flowgrid is NULL");
  if (!g->filled) return fail(ICTR_ERR_STATE, "flowgrid: no field yet (compute or set_nodes first)");
  *v = fg_dev(g);
  return ICTR_OK;
}
extern "C" int ictr_flowgrid_view_lost_(const ictr_flowgrid *g, FgDev *v, const unsigned char **lost) {
  if (!lost) return fail(ICTR_ERR_INVALID, "flowgrid is NULL");
  if (int rc = ictr_flowgrid_view_(g, v)) return rc;
  *lost = g->lost;
  return ICTR_OK;
}

extern "C" void ictr_flowgrid_destroy(ictr_flowgrid *g) { delete g; }
extern "C" int ictr_flowgrid_create(ictr_flowgrid **out, int w, int h, int step) {
  if (!out || w < 1 || h < 1 || step < 1 || step / 2 >= w || step / 2 >= h)
    return fail(ICTR_ERR_INVALID, "flowgrid: bad arguments (the grid needs at least one node)");
  if (int rc = need_device()) return rc;
  auto g = std::make_unique<ictr_flowgrid>();
  g->w = w;
  g->h = h;
  g->step = step;
  g->nx = (w - step / 2 + step - 1) / step;
  g->ny = (h - step / 2 + step - 1) / step;
  g->K = g->nx * g->ny;
  const size_t K = (size_t)g->K;
  // pts 2K f32 | out 2K | draw 2K | d 2K | status K i32 | iters K | rowhas ny | lost K u8
  const size_t bytes = 4 * (8 * K + 2 * K + (size_t)g->ny) + K;
  if (int rc = g->arena.alloc(bytes)) return rc;
  float *f = reinterpret_cast<float *>(g->arena.get());
  g->pts = f;
  g->out = f + 2 * K;
  g->draw = f + 4 * K;
  g->d = f + 6 * K;
  g->status = reinterpret_cast<int *>(f + 8 * K);
  g->iters = g->status + K;
  g->rowhas = g->iters + K;
  g->lost = reinterpret_cast<unsigned char *>(g->rowhas + g->ny);
  *out = g.release();
  return ICTR_OK;
}
extern "C" int ictr_flowgrid_dims(const ictr_flowgrid *g, int *nx, int *ny) {
  if (!g) return fail(ICTR_ERR_INVALID, "flowgrid is NULL");
  if (nx) *nx = g->nx;
  if (ny) *ny = g->ny;
  return ICTR_OK;
}
extern "C" int ictr_flowgrid_node_buffers_(ictr_flowgrid *g, float **draw, unsigned char **lost) {
  if (!g || !draw || !lost) return fail(ICTR_ERR_INVALID, "flowgrid is NULL");
  *draw = g->draw;
  *lost = g->lost;
  return ICTR_OK;
}
// draw + lost -> d, of n grids of one geometry at once: one memset of rowhas [n][ny] (the caller's block; NULL with
// n = 1: the grid's own), two launches
extern "C" int ictr_flowgrid_fill_(ictr_flowgrid *const *g, int n, int *rowhas, void *hip_stream) {
  if (!g || n < 1 || n > kSetMax || !g[0] || (!rowhas && n != 1)) return fail(ICTR_ERR_INVALID, "flowgrid_fill: bad arguments");
  if (!rowhas) rowhas = g[0]->rowhas;
  FgFillArgs a;
  memset(&a, 0, sizeof(a));
  for (int m = 0; m < n; ++m) {
    if (!g[m] || g[m]->nx != g[0]->nx || g[m]->ny != g[0]->ny)
      return fail(ICTR_ERR_INVALID, "flowgrid_fill: grid %d is NULL or differs in geometry", m);
    a.draw[m] = g[m]->draw, a.lost[m] = g[m]->lost, a.d[m] = g[m]->d;
  }
  a.rowhas = rowhas;
  hipStream_t s = (hipStream_t)hip_stream;
  const int nx = g[0]->nx, ny = g[0]->ny, K = g[0]->K;
  const dim3 grid((K + kBlock - 1) / kBlock, n), blk(kBlock);
  HIPCHK(hipMemsetAsync(rowhas, 0, sizeof(int) * (size_t)n * ny, s));
  hipLaunchKernelGGL(k_fg_rowfill, grid, blk, 0, s, a, nx, ny, K);
  hipLaunchKernelGGL(k_fg_colfill, grid, blk, 0, s, a, nx, ny, K);
  HIPCHK(hipGetLastError());
  for (int m = 0; m < n; ++m) g[m]->filled = 1;
  return ICTR_OK;
}
// nodes -> tracking (the 2-D launch or the 1-D one) -> d = out - pts -> fill
static int fg_compute(ictr_flowgrid *g, const ictr_pyramid *pa, const ictr_pyramid *pb, int psz, int lv_f, int maxiter,
                      float eps, void *hip_stream, void (*launch)(const PFArgs &, hipStream_t)) {
  if (!g) return fail(ICTR_ERR_INVALID, "flowgrid is NULL");
  PFArgs a;
  if (int rc = patchflow_args(pa, pb, psz, lv_f, 0, maxiter, eps, &a)) return rc;
  if ((int)a.lv[0].swo != g->w || (int)a.lv[0].sho != g->h)
    return fail(ICTR_ERR_INVALID, "flowgrid: the pyramids are not %d x %d", g->w, g->h);
  hipStream_t s = (hipStream_t)hip_stream;
  a.K = g->K;
  a.pts = g->pts;
  a.out = g->out;
  a.status = g->status;
  a.iters = g->iters;
  const dim3 grid((g->K + kBlock - 1) / kBlock), blk(kBlock);
  hipLaunchKernelGGL(k_fg_nodes, grid, blk, 0, s, g->pts, g->nx, g->K, g->step);
  launch(a, s);
  hipLaunchKernelGGL(k_fg_diff, grid, blk, 0, s, g->pts, g->out, g->status, g->K, g->draw, g->lost);
  return ictr_flowgrid_fill_(&g, 1, nullptr, s);
}
extern "C" int ictr_flowgrid_compute(ictr_flowgrid *g, const ictr_pyramid *pa, const ictr_pyramid *pb, int psz, int lv_f,
                                     int maxiter, float eps, void *hip_stream) {
  return fg_compute(g, pa, pb, psz, lv_f, maxiter, eps, hip_stream, launch_patchflow);
}
// the 1-D kernel returns a node's y with its input bits: every y displacement of the grid is y0 - y0 = +0.0
extern "C" int ictr_flowgrid_compute_x(ictr_flowgrid *g, const ictr_pyramid *pa, const ictr_pyramid *pb, int psz, int lv_f,
                                       int maxiter, float eps, void *hip_stream) {
  return fg_compute(g, pa, pb, psz, lv_f, maxiter, eps, hip_stream, launch_patchdisp);
}
extern "C" int ictr_flowgrid_set_nodes(ictr_flowgrid *g, const float *d, const unsigned char *lost) {
  if (!g || !d || !lost) return fail(ICTR_ERR_INVALID, "flowgrid_set_nodes: NULL argument");
  HIPCHK(hipMemcpy(g->draw, d, sizeof(float) * 2 * (size_t)g->K, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(g->lost, lost, (size_t)g->K, hipMemcpyHostToDevice));
  if (int rc = ictr_flowgrid_fill_(&g, 1, nullptr, nullptr)) return rc;
  HIPCHK(hipStreamSynchronize(nullptr));
  return ICTR_OK;
}
extern "C" int ictr_flowgrid_nodes(const ictr_flowgrid *g, float *d, unsigned char *lost) {
  if (!g) return fail(ICTR_ERR_INVALID, "flowgrid is NULL");
  if (!g->filled) return fail(ICTR_ERR_STATE, "flowgrid: no field yet (compute or set_nodes first)");
  HIPCHK(hipDeviceSynchronize());
  if (d) HIPCHK(hipMemcpy(d, g->d, sizeof(float) * 2 * (size_t)g->K, hipMemcpyDeviceToHost));
  if (lost) HIPCHK(hipMemcpy(lost, g->lost, (size_t)g->K, hipMemcpyDeviceToHost));
  return ICTR_OK;
}
extern "C" int ictr_flowgrid_gather(const ictr_flowgrid *g, const double *xy, int64_t K, double *out) {
  if (!g || K < 0 || (K > 0 && (!xy || !out)) || K > INT32_MAX) return fail(ICTR_ERR_INVALID, "flowgrid_gather: bad arguments");
  if (!g->filled) return fail(ICTR_ERR_STATE, "flowgrid: no field yet (compute or set_nodes first)");
  if (K == 0) return ICTR_OK;
  DevBuf<double> buf;
  if (int rc = buf.alloc(sizeof(double) * 4 * (size_t)K)) return rc;
  double *d = buf.get();
  HIPCHK(hipDeviceSynchronize());  // a compute on another stream has finished
  HIPCHK(hipMemcpy(d, xy, sizeof(double) * 2 * (size_t)K, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_fg_gather, dim3(((int)K + kBlock - 1) / kBlock), dim3(kBlock), 0, nullptr, fg_dev(g), d, (int)K,
                     d + 2 * K);
  HIPCHK(hipMemcpy(out, d + 2 * K, sizeof(double) * 2 * (size_t)K, hipMemcpyDeviceToHost));
  return ICTR_OK;
}
extern "C" int ictr_flowgrid_dense(const ictr_flowgrid *g, float *out, int on_device) {
  if (!g || !out) return fail(ICTR_ERR_INVALID, "flowgrid_dense: NULL argument");
  if (!g->filled) return fail(ICTR_ERR_STATE, "flowgrid: no field yet (compute or set_nodes first)");
  const size_t bytes = sizeof(float) * 2 * (size_t)g->w * g->h;
  DevBuf<float> own;  // the field on the device when `out` is host memory
  if (!on_device)
    if (int rc = own.alloc(bytes)) return rc;
  float *d = on_device ? out : own.get();
  HIPCHK(hipDeviceSynchronize());
  launch_fg_dense(fg_dev(g), reinterpret_cast<float2 *>(d), nullptr);
  HIPCHK(on_device ? hipStreamSynchronize(nullptr) : hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost));
  return ICTR_OK;
}

struct ictr_pointtrack {
  int w = 0, h = 0, bsize = 0, mc = 0, lv_f = 0, psz = 0, step = 0, maxiter = 0, mindist = 0, win = 0;
  float eps = 0;
  double quality = 0, th_ratio = 0, th_abs = 0;
  int64_t nframes = 0;          // frames pushed; frcounter = max(nframes - 1, 0)
  ictr_pyramid *pyr[2] = {nullptr, nullptr};  // owned; opaque here, so released through ictr_pyramid_destroy
  std::unique_ptr<ictr_flowgrid> fw, bw;
  GfWork gf;
  PtGeom geom;
  DevBuf<char> ring;                 // bsize slots
  DevBuf<float> corners;             // [mc][2] staging of the corner picker
  std::vector<PinBuf<char>> store;   // pinned host copies of the blocks that left the window, in block order
  ~ictr_pointtrack() {
    (void)hipDeviceSynchronize();  // nothing in flight reads what goes now
    ictr_pyramid_destroy(pyr[0]);
    ictr_pyramid_destroy(pyr[1]);
  }
};

extern "C" void ictr_pointtrack_destroy(ictr_pointtrack *t) { delete t; }
extern "C" int ictr_pointtrack_create(ictr_pointtrack **out, int w, int h, int bsize, int maxcorners, int lv_f, int psz,
                                      int step, int maxiter, float eps, double quality, int mindist, int win,
                                      double th_ratio, double th_abs) {
  if (!out || bsize < 1 || maxcorners < 1 || psz < 1 || psz > 32 || lv_f < 0 || lv_f > 15 || maxiter < 0)
    return fail(ICTR_ERR_INVALID, "pointtrack: bad arguments (bsize >= 1, maxcorners >= 1, psz 1..32)");
  if (int rc = need_device()) return rc;
  auto t = std::make_unique<ictr_pointtrack>();
  t->w = w, t->h = h, t->bsize = bsize, t->mc = maxcorners, t->lv_f = lv_f, t->psz = psz, t->step = step;
  t->maxiter = maxiter, t->eps = eps, t->quality = quality, t->mindist = mindist, t->win = win;
  t->th_ratio = th_ratio, t->th_abs = th_abs;
  t->geom = pt_geom(maxcorners, bsize);
  for (auto *grid : {&t->fw, &t->bw}) {
    ictr_flowgrid *g = nullptr;
    if (int rc = ictr_flowgrid_create(&g, w, h, step)) return rc;
    grid->reset(g);
  }
  if (int rc = gf_alloc(&t->gf, w, h, mindist, win)) return rc;
  if (int rc = t->ring.alloc(t->geom.bytes * (size_t)bsize)) return rc;
  if (int rc = t->corners.alloc(sizeof(float) * 2 * (size_t)maxcorners)) return rc;
  HIPCHK(hipMemset(t->ring.get(), 0, t->geom.bytes * (size_t)bsize));
  *out = t.release();
  return ICTR_OK;
}
extern "C" int ictr_pointtrack_push_frame(ictr_pointtrack *t, const float *img) {
  if (!t || !img) return fail(ICTR_ERR_INVALID, "pointtrack_push_frame: NULL argument");
  hipStream_t s = nullptr;
  const int64_t f = t->nframes;
  ictr_pyramid *&cur = t->pyr[f & 1];
  if (!cur) {  // the first two frames allocate their pyramids
    if (int rc = ictr_pyramid_create(&cur, img, t->w, t->h, t->lv_f, 1, t->psz)) return rc;
  } else if (int rc = ictr_pyramid_rebuild(cur, img, s)) {
    return rc;
  }
  t->nframes = f + 1;
  if (f == 0) return ICTR_OK;
  const int64_t k = f - 1;  // the pair (k, k + 1); addframe number k + 1
  ictr_pyramid *pa = t->pyr[k & 1], *pb = cur;
  if (int rc = ictr_flowgrid_compute(t->fw.get(), pa, pb, t->psz, t->lv_f, t->maxiter, t->eps, s)) return rc;
  if (int rc = ictr_flowgrid_compute(t->bw.get(), pb, pa, t->psz, t->lv_f, t->maxiter, t->eps, s)) return rc;
  ictr_level0 l0;
  if (int rc = ictr_pyramid_level0(pa, "pointtrack_push_frame", &l0)) return rc;
  const PtGeom &g = t->geom;
  const dim3 grid((g.mc + kBlock - 1) / kBlock), blk(kBlock);
  char *ring = t->ring.get();
  const PtSlot open = pt_slot(ring + g.bytes * (size_t)(k % g.bsize), g);
  if (int rc = gf_run(t->gf, l0.img, l0.stride, g.mc, t->quality, t->corners.get(), open.count, s)) return rc;
  hipLaunchKernelGGL(k_pt_open, grid, blk, 0, s, open, t->corners.get(), g.mc, g.bsize);
  for (int age = 0; age <= g.bsize - 2 && age <= k; ++age) {  // the blocks k - age, column age -> age + 1
    const PtSlot sl = pt_slot(ring + g.bytes * (size_t)((k - age) % g.bsize), g);
    hipLaunchKernelGGL(k_pt_advance, grid, blk, 0, s, sl, g.bsize, age, fg_dev(t->fw.get()), fg_dev(t->bw.get()), t->th_ratio,
                       t->th_abs);
  }
  HIPCHK(hipGetLastError());
  const int64_t gone = k - g.bsize + 1;  // leaves the window with this pair; its slot is opened again by pair k + 1
  if (gone >= 0) {
    PinBuf<char> hp;
    if (int rc = hp.alloc(g.bytes)) return rc;
    t->store.push_back(std::move(hp));
    HIPCHK(hipMemcpyAsync(t->store.back().get(), ring + g.bytes * (size_t)(gone % g.bsize), g.bytes, hipMemcpyDeviceToHost,
                          s));
  }
  return ICTR_OK;
}
extern "C" int ictr_pointtrack_frcounter(const ictr_pointtrack *t, int64_t *frcounter) {
  if (!t || !frcounter) return fail(ICTR_ERR_INVALID, "pointtrack_frcounter: NULL argument");
  *frcounter = t->nframes > 0 ? t->nframes - 1 : 0;
  return ICTR_OK;
}
extern "C" int ictr_pointtrack_read_block(ictr_pointtrack *t, int64_t block, float *tracks, unsigned char *valid,
                                          double *absmovement, int *count) {
  if (!t || !count) return fail(ICTR_ERR_INVALID, "pointtrack_read_block: NULL argument");
  const int64_t frc = t->nframes > 0 ? t->nframes - 1 : 0;
  if (block < 0 || block >= frc) return fail(ICTR_ERR_INVALID, "pointtrack_read_block: no such block");
  const PtGeom &g = t->geom;
  HIPCHK(hipStreamSynchronize(nullptr));
  std::vector<char> tmp;
  const char *src;
  if (block < (int64_t)t->store.size()) {
    src = t->store[(size_t)block].get();
  } else {
    tmp.resize(g.bytes);
    HIPCHK(hipMemcpy(tmp.data(), t->ring.get() + g.bytes * (size_t)(block % g.bsize), g.bytes, hipMemcpyDeviceToHost));
    src = tmp.data();
  }
  const PtSlot sl = pt_slot(src, g);
  const int n = *sl.count;
  *count = n;
  if (tracks) memcpy(tracks, sl.tracks, sizeof(float) * 2 * (size_t)g.bsize * n);
  if (valid) memcpy(valid, sl.valid, (size_t)n);
  if (absmovement) memcpy(absmovement, sl.absmov, sizeof(double) * (size_t)n);
  return ICTR_OK;
}
