// ictr_host.hip -- implementation of the C-ABI in include/ictr.h: handle objects, device arenas and the
// launch sequences. Host-side maths here is only what the reference also does per call on a handful of
// scalars (pose normalisation pose.cpp:25-113, point-cloud normalisation odometer.cpp:171-239); everything
// that touches pixels or points runs in the kernels of ictr_kernels.hip. There is no CPU fallback.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "ictr_dev.h"
#include "ictr_launch.h"
#include "se3_math.h"
#include "ictr_pose_hd.h"

using namespace ictr;

// ---------------------------------------------------------------- errors
static thread_local std::string g_err;
int ictr::fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

extern "C" const char *ictr_last_error(void) { return g_err.c_str(); }
extern "C" int ictr_version(void) { return 100; }
extern "C" int ictr_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
extern "C" int ictr_set_device(int device) {
  HIPCHK(hipSetDevice(device));
  return ICTR_OK;
}
// Measured streaming-read bandwidth of this GPU in GB/s: `bytes` of freshly allocated memory (>> the 256 MB Infinity
// Cache) read `reps` times with plain wide loads. A yardstick for roofline reports next to the vendor peak.
extern "C" int ictr_stream_read_bandwidth(size_t bytes, int reps, double *gbps_out) {
  if (!gbps_out || bytes < (1u << 20) || reps < 1) return fail(ICTR_ERR_INVALID, "stream_read_bandwidth: bad arguments");
  if (int rc = need_device()) return rc;
  DevBuf<float> buf, sink;
  Event e0, e1;
  if (int rc = buf.alloc(bytes)) return rc;
  if (int rc = sink.alloc(sizeof(float) * 8192 * kBlock)) return rc;
  HIPCHK(hipMemset(buf.get(), 0, bytes));
  if (int rc = e0.create()) return rc;
  if (int rc = e1.create()) return rc;
  float ms = 0.0f;
  launch_stream_read(buf.get(), bytes / 4, sink.get(), nullptr);  // warm-up
  HIPCHK(hipEventRecord(e0.get(), nullptr));
  for (int r = 0; r < reps; ++r) launch_stream_read(buf.get(), bytes / 4, sink.get(), nullptr);
  HIPCHK(hipEventRecord(e1.get(), nullptr));
  HIPCHK(hipEventSynchronize(e1.get()));
  HIPCHK(hipEventElapsedTime(&ms, e0.get(), e1.get()));
  *gbps_out = (double)bytes * reps / (ms * 1e-3) / 1e9;
  return ICTR_OK;
}
// inspection: the resident-iteration kernel's transposing wave reduction alone (ictr_resident.hip, TrAcc) on caller data.
// vals[64 lanes][64 values = 2 patch + kind] -> out[lane] = the 64-lane sum of value 2 patch_of_lane + kind_of_lane
extern "C" int ictr_debug_transpose_reduce(const float *vals, float *out, int *patch_of_lane, int *kind_of_lane,
                                           int patches_per_wave) {
  if (!vals || !out || !patch_of_lane || !kind_of_lane || (patches_per_wave != 16 && patches_per_wave != 32))
    return fail(ICTR_ERR_INVALID, "debug_transpose_reduce: bad arguments (patches per wave 16 or 32)");
  if (int rc = need_device()) return rc;
  DevBuf<float> dv, dout;
  DevBuf<int> dpb;
  if (int rc = dv.alloc(sizeof(float) * 64 * 64)) return rc;
  if (int rc = dout.alloc(sizeof(float) * 64)) return rc;
  if (int rc = dpb.alloc(sizeof(int) * 128)) return rc;
  int *dp = dpb.get();
  HIPCHK(hipMemcpy(dv.get(), vals, sizeof(float) * 64 * 64, hipMemcpyHostToDevice));
  HIPCHK(launch_debug_transpose_reduce(dv.get(), dout.get(), dp, dp + 64, patches_per_wave, nullptr));
  HIPCHK(hipMemcpy(out, dout.get(), sizeof(float) * 64, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(patch_of_lane, dp, sizeof(int) * 64, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(kind_of_lane, dp + 64, sizeof(int) * 64, hipMemcpyDeviceToHost));
  return ICTR_OK;
}

// inspection: the resident-iteration kernel's half-window fetch path alone (ictr_devfn.h hw_*), one wave, eight windows.
// plane[rows][sw]; top_left[8] = texel index of each window's top-left texel (the 9x9 window must lie in the plane) ->
// out[window][lane = pixel][4] = the taps a, b, c, d = (x,y), (x-1,y), (x,y-1), (x-1,y-1) of the lane's pixel
extern "C" int ictr_debug_half_window(const float *plane, int rows, int sw, const int *top_left, float *out) {
  if (!plane || !top_left || !out || rows < 9 || sw < 9 || (int64_t)rows * sw > (1 << 24))
    return fail(ICTR_ERR_INVALID, "debug_half_window: bad arguments (a plane of at least 9 x 9 texels)");
  for (int g = 0; g < 8; ++g) {
    const int r = top_left[g] / sw, c = top_left[g] % sw;
    if (top_left[g] < 0 || r + 9 > rows || c + 9 > sw) return fail(ICTR_ERR_INVALID, "debug_half_window: a window leaves the plane");
  }
  if (int rc = need_device()) return rc;
  const int n = rows * sw;
  DevBuf<float> dpl, dout;
  DevBuf<int> dtl;
  if (int rc = dpl.alloc(sizeof(float) * n)) return rc;
  if (int rc = dout.alloc(sizeof(float) * 8 * 64 * 4)) return rc;
  if (int rc = dtl.alloc(sizeof(int) * 8)) return rc;
  HIPCHK(hipMemcpy(dpl.get(), plane, sizeof(float) * n, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dtl.get(), top_left, sizeof(int) * 8, hipMemcpyHostToDevice));
  HIPCHK(launch_debug_half_window(dpl.get(), n, sw, dtl.get(), dout.get(), nullptr));
  HIPCHK(hipMemcpy(out, dout.get(), sizeof(float) * 8 * 64 * 4, hipMemcpyDeviceToHost));
  return ICTR_OK;
}

// inspection: the solver turn's linear algebra (WaveSolver, ictr_devfn.h) alone on caller systems, one wave each.
// through_state: the factors go through ProbState (ws_store_factor) and a second launch reloads them (ws_load_factor).
extern "C" int ictr_debug_wave_solve(const float *H36, const float *b6, int64_t n, int through_state, float *x6, int *rank,
                                     int *nonzero, int *rowmap6, int *colmap6, float *lu36) {
  if (!H36 || !b6 || !x6 || !rank || !nonzero || !rowmap6 || !colmap6 || !lu36 || n < 1 || n > (1 << 20))
    return fail(ICTR_ERR_INVALID, "debug_wave_solve: bad arguments (1 .. 2^20 systems)");
  if (int rc = need_device()) return rc;
  const size_t N = (size_t)n;
  DevBuf<float> dfb;  // H[36 n] | b[6 n] | x[6 n] | lu[36 n]
  DevBuf<int> dib;    // rank[n] | nonzero[n] | rowmap[6 n] | colmap[6 n]
  DevBuf<ProbState> st;
  if (int rc = dfb.alloc(sizeof(float) * 84 * N)) return rc;
  if (int rc = dib.alloc(sizeof(int) * 14 * N)) return rc;
  if (int rc = st.alloc(sizeof(ProbState) * N, true)) return rc;
  float *df = dfb.get();
  int *di = dib.get();
  HIPCHK(hipMemset(df + 42 * N, 0xff, sizeof(float) * 42 * N));
  HIPCHK(hipMemset(di, 0xff, sizeof(int) * 14 * N));
  HIPCHK(hipMemcpy(df, H36, sizeof(float) * 36 * N, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(df + 36 * N, b6, sizeof(float) * 6 * N, hipMemcpyHostToDevice));
  HIPCHK(launch_debug_wave_solve(df, df + 36 * N, (int)n, st.get(), through_state, df + 42 * N, di, di + N, di + 2 * N,
                                 di + 8 * N, df + 48 * N, nullptr));
  HIPCHK(hipMemcpy(x6, df + 42 * N, sizeof(float) * 6 * N, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(lu36, df + 48 * N, sizeof(float) * 36 * N, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(rank, di, sizeof(int) * N, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(nonzero, di + N, sizeof(int) * N, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(rowmap6, di + 2 * N, sizeof(int) * 6 * N, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(colmap6, di + 8 * N, sizeof(int) * 6 * N, hipMemcpyDeviceToHost));
  return ICTR_OK;
}
// inspection: the device builds of se3_exp<float> (in p[6] -> out G[12]) / se3_log<float> (in G[12] -> out p[6])
extern "C" int ictr_debug_se3(const float *in, int64_t n, int log_not_exp, float *out) {
  if (!in || !out || n < 1 || n > (1 << 24)) return fail(ICTR_ERR_INVALID, "debug_se3: bad arguments");
  if (int rc = need_device()) return rc;
  const size_t ni = (size_t)n * (log_not_exp ? 12 : 6), no = (size_t)n * (log_not_exp ? 6 : 12);
  DevBuf<float> buf;
  if (int rc = buf.alloc(sizeof(float) * (ni + no))) return rc;
  float *d = buf.get();
  HIPCHK(hipMemcpy(d, in, sizeof(float) * ni, hipMemcpyHostToDevice));
  HIPCHK(launch_debug_se3(d, d + ni, (long long)n, log_not_exp ? 1 : 0, nullptr));
  HIPCHK(hipMemcpy(out, d + ni, sizeof(float) * no, hipMemcpyDeviceToHost));
  return ICTR_OK;
}

int ictr::need_device() {
  if (ictr_device_count() <= 0)
    return fail(ICTR_ERR_NO_DEVICE, "no usable HIP device: the tracker has no CPU fallback");
  return ICTR_OK;
}

extern "C" int ictr_optparam_init(ictr_optparam *op, int lv_f, int lv_l, int psz, int maxiter, float normdp_ratio,
                                  int donorm, int dopatchnorm, int maxpttrack, int verbosity) {
  if (!op) return fail(ICTR_ERR_INVALID, "op is NULL");
  memset(op, 0, sizeof(*op));
  op->lv_f = lv_f;
  op->lv_l = lv_l;
  op->psz = psz;
  op->pszd2 = psz / 2;
  op->pszd2m3 = psz + op->pszd2 - 1;
  op->novals = psz * psz;
  op->maxiter = maxiter;
  op->normdp_ratio = normdp_ratio;
  op->donorm = donorm != 0;
  op->dopatchnorm = dopatchnorm != 0;
  op->maxpttrack = maxpttrack;
  const int r = op->maxpttrack % 4;  // SSEMULTIPL padding of the drivers (run_io_reprojection_test.cpp:123-126)
  if (r > 0) op->maxpttrack += 4 - r;
  op->verbosity = verbosity;
  return ICTR_OK;
}

// ---------------------------------------------------------------- CamClass
struct ictr_cam {
  int noscales;
  int padding;
  int wh[2];
  std::vector<float> fx, fy, cx, cy, swo, sho, sw, sh;
};

extern "C" int ictr_cam_create(ictr_cam **out, int noscales, const float *fc, const float *cc, const int *wh,
                               int padding) {
  if (!out || !fc || !cc || !wh || noscales < 1 || noscales > 16 || padding < 0)
    return fail(ICTR_ERR_INVALID, "ictr_cam_create: bad arguments (noscales must be 1..16)");
  ictr_cam *c = new ictr_cam;
  c->noscales = noscales;
  c->padding = padding;
  c->wh[0] = wh[0];
  c->wh[1] = wh[1];
  for (auto *v : {&c->fx, &c->fy, &c->cx, &c->cy, &c->swo, &c->sho, &c->sw, &c->sh}) v->resize(noscales);
  for (int i = 0; i < noscales; ++i) {
    const float s = (float)(1 / pow(2, i));  // camera.cpp:33
    c->fx[i] = s * fc[0];
    c->fy[i] = s * fc[1];
    c->cx[i] = s * cc[0];
    c->cy[i] = s * cc[1];
    c->swo[i] = s * (float)wh[0];
    c->sho[i] = s * (float)wh[1];
    c->sw[i] = c->swo[i] + 2 * padding;
    c->sh[i] = c->sho[i] + 2 * padding;
  }
  *out = c;
  return ICTR_OK;
}
extern "C" void ictr_cam_destroy(ictr_cam *cam) { delete cam; }
#define CAMGET(name, field) \
  extern "C" float ictr_cam_##name(const ictr_cam *cam, int sc) { return cam->field[sc]; }
CAMGET(getfx, fx)
CAMGET(getfy, fy)
CAMGET(getcx, cx)
CAMGET(getcy, cy)
CAMGET(getswo, swo)
CAMGET(getsho, sho)
CAMGET(getsw, sw)
CAMGET(getsh, sh)

static LevelCam level_cam(const ictr_cam *c, int l) {
  LevelCam lc;
  lc.fx = c->fx[l];
  lc.fy = c->fy[l];
  lc.cx = c->cx[l];
  lc.cy = c->cy[l];
  lc.swo = c->swo[l];
  lc.sho = c->sho[l];
  lc.sw = (int)c->sw[l];
  return lc;
}

// ---------------------------------------------------------------- SE(3) helpers on the host
extern "C" void ictr_se3_coeff_to_group_f(float *G, const float *p) { se3_exp<float>(G, p); }
extern "C" void ictr_se3_coeff_to_group_d(double *G, const double *p) { se3_exp<double>(G, p); }
extern "C" void ictr_se3_group_to_coeff_f(float *p, const float *G) { se3_log<float>(p, G); }
extern "C" void ictr_se3_group_to_coeff_d(double *p, const double *G) { se3_log<double>(p, G); }
extern "C" void ictr_solve6(const float *H, const float *b, float *x) {
  // the device path (factor once per level + substitute per iteration), run back to back on the host
  float A[36], c[6];
  int piv[12], info[2];
  memcpy(A, H, sizeof(A));
  lu_factor_ws<6>(A, piv, info);
  lu_apply_ws<6>(A, piv, info, b, x, c);
}

// ---------------------------------------------------------------- pyramid
struct ictr_pyramid {
  int nlev = 0, pad = 0, w0 = 0, h0 = 0, getgrad = 0;  // getgrad: 0 image only, 1 + dx / dy / packed planes,
                                                       // 2 image only, gradients formed on the fly by the consumers
  int builder_made = 0;  // the planes were computed by pyramid_build (dx / dy ARE the central differences of img)
  std::vector<int> w, h, sw, sh;
  std::vector<float *> img, dx, dy;  // device planes
  std::vector<float *> pack;         // with gradients: the level again as interleaved {img, dx, dy, 0} texels
  DevBuf<float> arena;  // every plane of every level
  DevBuf<float> stage;  // device copy of a host frame handed to ictr_pyramid_rebuild (allocated on first use)
};

// internal: what ictr_icgn.hip needs to know about a pyramid
extern "C" int ictr_pyramid_view_(const ictr_pyramid *p, ictr_pyramid_view *v) {
  v->nlev = p->nlev;
  v->pad = p->pad;
  v->w = p->w.data();
  v->h = p->h.data();
  v->sw = p->sw.data();
  v->img = p->img.data();
  v->dx = p->dx.data();
  v->dy = p->dy.data();
  v->getgrad = p->getgrad == 1 ? 1 : 0;  // (gradient PLANES; image-only pyramids of the tracker's OTF path have none)
  return 0;
}

static void level_size(int w, int h, int level, int *wl, int *hl) {
  auto half = [](int v) {  // cvRound(v*0.5), round-half-even, as cv::resize(dsize=Size(), fx=.5) sizes its output
    const int q = v / 2;
    if (v % 2 == 0) return q;
    return (q % 2 == 0) ? q : q + 1;
  };
  for (int i = 0; i < level; ++i) {
    w = half(w);
    h = half(h);
  }
  *wl = w;
  *hl = h;
}

void ictr::pyramid_level_size(int w, int h, int level, int *wl, int *hl) { level_size(w, h, level, wl, hl); }

static int pyramid_alloc(ictr_pyramid **out, int w, int h, int lv_f, int getgrad, int pad) {
  if (!out || w < 1 || h < 1 || lv_f < 0 || lv_f > 15 || pad < 0 || getgrad < 0 || getgrad > 2)
    return fail(ICTR_ERR_INVALID, "pyramid: bad arguments");
  if (int rc = need_device()) return rc;
  auto p = std::make_unique<ictr_pyramid>();
  p->nlev = lv_f + 1;
  p->pad = pad;
  p->w0 = w;
  p->h0 = h;
  p->getgrad = getgrad;
  size_t total = 0;
  for (int l = 0; l <= lv_f; ++l) {
    int wl, hl;
    level_size(w, h, l, &wl, &hl);
    if (wl < 1 || hl < 1) return fail(ICTR_ERR_INVALID, "pyramid: level %d is empty", l);
    p->w.push_back(wl);
    p->h.push_back(hl);
    p->sw.push_back(wl + 2 * pad);
    p->sh.push_back(hl + 2 * pad);
    size_t plane = (size_t)(wl + 2 * pad) * (hl + 2 * pad);
    plane = (plane + 63) / 64 * 64;  // 256-B aligned planes
    total += plane * (getgrad == 1 ? 7 : getgrad == 2 ? 1 : 3);
  }
  if (int rc = p->arena.alloc(total * sizeof(float))) return rc;
  float *cur = p->arena.get();
  for (int l = 0; l <= lv_f; ++l) {
    size_t plane = (size_t)p->sw[l] * p->sh[l];
    plane = (plane + 63) / 64 * 64;
    p->img.push_back(cur);
    p->dx.push_back(getgrad == 2 ? nullptr : cur + plane);
    p->dy.push_back(getgrad == 2 ? nullptr : cur + 2 * plane);
    p->pack.push_back(getgrad == 1 ? cur + 3 * plane : nullptr);
    cur += (getgrad == 1 ? 7 : getgrad == 2 ? 1 : 3) * plane;
  }
  *out = p.release();
  return ICTR_OK;
}

static int pyramid_build(ictr_pyramid *p, const float *img_dev, hipStream_t s) {
  p->builder_made = 1;
  const int planes = p->getgrad == 1 ? 1 : 0;  // getgrad 2: the image levels only
  for (int l = 0; l < p->nlev; ++l) {  // one launch per level (k_pyr_level)
    if (l == 0)
      launch_pyr_level(img_dev, 1, p->w[0], p->h[0], p->w[0], p->img[0], p->dx[0], p->dy[0], p->pack[0], p->w[0], p->h[0],
                       p->pad, p->sw[0], p->sh[0], planes, s);
    else
      launch_pyr_level(p->img[l - 1], 0, p->w[l - 1], p->h[l - 1], p->sw[l - 1], p->img[l], p->dx[l], p->dy[l], p->pack[l],
                       p->w[l], p->h[l], p->pad, p->sw[l], p->sh[l], planes, s);
  }
  HIPCHK(hipGetLastError());
  return ICTR_OK;
}

// A video loop builds one pyramid per incoming frame (run_track_nposes.cpp:180: one per image of the sequence): refill an
// existing pyramid in place -- no allocation, every plane keeps its address (batches / graphs that hold them stay valid).
extern "C" int ictr_pyramid_rebuild_device(ictr_pyramid *p, const float *img_dev, void *hip_stream) {
  if (!p || !img_dev) return fail(ICTR_ERR_INVALID, "pyramid_rebuild: NULL argument");
  return pyramid_build(p, img_dev, (hipStream_t)hip_stream);
}
extern "C" int ictr_pyramid_rebuild(ictr_pyramid *p, const float *img, void *hip_stream) {
  if (!p || !img) return fail(ICTR_ERR_INVALID, "pyramid_rebuild: NULL argument");
  const size_t bytes = sizeof(float) * (size_t)p->w0 * p->h0;
  if (!p->stage)
    if (int rc = p->stage.alloc(bytes)) return rc;
  // pageable host memory: the copy has left `img` when the call returns; the kernels are ordered behind it on the stream
  HIPCHK(hipMemcpyAsync(p->stage.get(), img, bytes, hipMemcpyHostToDevice, (hipStream_t)hip_stream));
  return pyramid_build(p, p->stage.get(), (hipStream_t)hip_stream);
}

extern "C" int ictr_pyramid_create_device(ictr_pyramid **out, const float *img_dev, int w, int h, int lv_f, int getgrad,
                                          int pad, void *hip_stream) {
  if (!img_dev) return fail(ICTR_ERR_INVALID, "pyramid: img is NULL");
  ictr_pyramid *raw = nullptr;
  if (int rc = pyramid_alloc(&raw, w, h, lv_f, getgrad, pad)) return rc;
  std::unique_ptr<ictr_pyramid> p(raw);
  if (int rc = pyramid_build(raw, img_dev, (hipStream_t)hip_stream)) return rc;
  *out = p.release();
  return ICTR_OK;
}

extern "C" int ictr_pyramid_create(ictr_pyramid **out, const float *img, int w, int h, int lv_f, int getgrad,
                                   int pad) {
  if (!img) return fail(ICTR_ERR_INVALID, "pyramid: img is NULL");
  if (int rc = need_device()) return rc;
  DevBuf<float> d;
  if (int rc = d.alloc(sizeof(float) * (size_t)w * h)) return rc;
  HIPCHK(hipMemcpy(d.get(), img, sizeof(float) * (size_t)w * h, hipMemcpyHostToDevice));
  ictr_pyramid *raw = nullptr;
  const int rc = ictr_pyramid_create_device(&raw, d.get(), w, h, lv_f, getgrad, pad, nullptr);
  std::unique_ptr<ictr_pyramid> p(raw);
  const hipError_t e = hipDeviceSynchronize();  // the kernels have read `d` before it goes
  if (rc) return rc;
  if (e != hipSuccess) return fail(ICTR_ERR_HIP, "pyramid kernels failed: %s", hipGetErrorString(e));
  *out = p.release();
  return ICTR_OK;
}

extern "C" int ictr_pyramid_create_from_host_planes(ictr_pyramid **out, const float **img_pyr, const float **dx_pyr,
                                                    const float **dy_pyr, int w, int h, int lv_f, int pad) {
  if (!img_pyr) return fail(ICTR_ERR_INVALID, "pyramid: img_pyr is NULL");
  ictr_pyramid *raw = nullptr;
  if (int rc = pyramid_alloc(&raw, w, h, lv_f, dx_pyr && dy_pyr, pad)) return rc;
  std::unique_ptr<ictr_pyramid> p(raw);
  for (int l = 0; l <= lv_f; ++l) {
    const size_t bytes = sizeof(float) * (size_t)p->sw[l] * p->sh[l];
    HIPCHK(hipMemcpy(p->img[l], img_pyr[l], bytes, hipMemcpyHostToDevice));
    if (dx_pyr && dy_pyr) {
      HIPCHK(hipMemcpy(p->dx[l], dx_pyr[l], bytes, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(p->dy[l], dy_pyr[l], bytes, hipMemcpyHostToDevice));
    }
    if (p->getgrad) launch_pyr_pack(p->img[l], p->dx[l], p->dy[l], p->pack[l], (size_t)p->sw[l] * p->sh[l], nullptr);
  }
  if (p->getgrad) HIPCHK(hipStreamSynchronize(nullptr));
  *out = p.release();
  return ICTR_OK;
}

extern "C" void ictr_pyramid_destroy(ictr_pyramid *p) { delete p; }
extern "C" int ictr_pyramid_levels(const ictr_pyramid *p) { return p ? p->nlev : 0; }
extern "C" int ictr_pyramid_level_dims(const ictr_pyramid *p, int level, int *sw, int *sh) {
  if (!p || level < 0 || level >= p->nlev) return fail(ICTR_ERR_INVALID, "pyramid: bad level");
  if (sw) *sw = p->sw[level];
  if (sh) *sh = p->sh[level];
  return ICTR_OK;
}
static float *pyr_plane(const ictr_pyramid *p, int level, int which) {
  if (!p || level < 0 || level >= p->nlev) return nullptr;
  return which == 0 ? p->img[level] : which == 1 ? p->dx[level] : which == 2 ? p->dy[level] : nullptr;
}
extern "C" const float *ictr_pyramid_device_plane(const ictr_pyramid *p, int level, int which) {
  return pyr_plane(p, level, which);
}
extern "C" int ictr_pyramid_download(const ictr_pyramid *p, int level, int which, float *host_out) {
  const float *d = pyr_plane(p, level, which);
  if (!d || !host_out) return fail(ICTR_ERR_INVALID, "pyramid_download: bad arguments");
  HIPCHK(hipMemcpy(host_out, d, sizeof(float) * (size_t)p->sw[level] * p->sh[level], hipMemcpyDeviceToHost));
  return ICTR_OK;
}

static int get_patch_impl(const ictr_pyramid *pyr, int level, const float *mids, int64_t K, int psz, int dopatchnorm,
                          float *out, float *out_dx, float *out_dy, bool grad) {
  if (!pyr || level < 0 || level >= pyr->nlev || !mids || !out || K < 0 || psz < 1 || psz > pyr->pad)
    return fail(ICTR_ERR_INVALID, "get_patch: bad arguments (psz must be <= pyramid padding)");
  if (grad && (!out_dx || !out_dy || pyr->getgrad != 1)) return fail(ICTR_ERR_INVALID, "get_patch_grad: no gradient planes");
  if (K == 0) return ICTR_OK;
  // centres must lie inside [0,swo] x [0,sho] like the callers guarantee (odometer.cpp:273-276)
  for (int64_t i = 0; i < K; ++i)
    if (!(mids[i] >= 0 && mids[i] <= (float)pyr->w[level] && mids[i + K] >= 0 && mids[i + K] <= (float)pyr->h[level]))
      return fail(ICTR_ERR_INVALID, "get_patch: centre %lld outside the image", (long long)i);
  const size_t nf = (size_t)K * psz * psz;
  DevBuf<float> d_m, d_ob;
  if (int rc = d_m.alloc(sizeof(float) * 2 * K)) return rc;
  if (int rc = d_ob.alloc(sizeof(float) * nf * (grad ? 3 : 1))) return rc;
  float *d_o = d_ob.get();
  HIPCHK(hipMemcpy(d_m.get(), mids, sizeof(float) * 2 * K, hipMemcpyHostToDevice));
  launch_getpatch(pyr->img[level], grad ? pyr->dx[level] : nullptr, grad ? pyr->dy[level] : nullptr, d_m.get(), (int)K, psz,
                  pyr->sw[level], dopatchnorm, d_o, grad ? d_o + nf : nullptr, grad ? d_o + 2 * nf : nullptr, nullptr);
  HIPCHK(hipMemcpy(out, d_o, sizeof(float) * nf, hipMemcpyDeviceToHost));
  if (grad) {
    HIPCHK(hipMemcpy(out_dx, d_o + nf, sizeof(float) * nf, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_dy, d_o + 2 * nf, sizeof(float) * nf, hipMemcpyDeviceToHost));
  }
  return ICTR_OK;
}
extern "C" int ictr_get_patch(const ictr_pyramid *pyr, int level, const float *mids, int64_t K, int psz,
                              int dopatchnorm, float *out) {
  return get_patch_impl(pyr, level, mids, K, psz, dopatchnorm, out, nullptr, nullptr, false);
}
extern "C" int ictr_get_patch_grad(const ictr_pyramid *pyr, int level, const float *mids, int64_t K, int psz,
                                   int dopatchnorm, float *out, float *out_dx, float *out_dy) {
  return get_patch_impl(pyr, level, mids, K, psz, dopatchnorm, out, out_dx, out_dy, true);
}

// run_track_nposes.cpp:271-355: per-point patch correlation, computed on the device (k_ncc)
extern "C" int ictr_ncc_score(const ictr_pyramid *pyr_back, const ictr_pyramid *pyr_ref, const ictr_pyramid *pyr_fwd,
                              int level, const float *mids, int64_t K, int psz, float w_back, float w_fwd,
                              float *out_corr) {
  if (!pyr_back || !pyr_ref || !pyr_fwd || K < 0 || (K > 0 && (!mids || !out_corr)) || psz < 1 || psz > 64)
    return fail(ICTR_ERR_INVALID, "ncc_score: bad arguments");
  for (const ictr_pyramid *py : {pyr_back, pyr_ref, pyr_fwd})
    if (level < 0 || level >= py->nlev || psz > py->pad || py->sw[level] != pyr_ref->sw[level] ||
        py->w[level] != pyr_ref->w[level] || py->h[level] != pyr_ref->h[level])
      return fail(ICTR_ERR_INVALID, "ncc_score: pyramids differ at level %d or padding < psz", level);
  if (K == 0) return ICTR_OK;
  if (int rc = need_device()) return rc;
  DevBuf<float> buf;
  if (int rc = buf.alloc(sizeof(float) * 7 * K)) return rc;
  float *d = buf.get();
  HIPCHK(hipMemcpy(d, mids, sizeof(float) * 6 * K, hipMemcpyHostToDevice));
  launch_ncc(pyr_back->img[level], pyr_ref->img[level], pyr_fwd->img[level], d, (int)K, psz, pyr_ref->sw[level],
             (float)pyr_ref->w[level], (float)pyr_ref->h[level], w_back, w_fwd, d + 6 * K, nullptr);
  HIPCHK(hipMemcpy(out_corr, d + 6 * K, sizeof(float) * K, hipMemcpyDeviceToHost));
  return ICTR_OK;
}

// ---------------------------------------------------------------- Python flow-tracking surface (misc_src) on the device
// classoftrack.func_get_transf_position (classoftrack.py:4-34). disp_u / disp_v: (H, W) planes, float32 or float64,
// on the host or (fields_on_device) already on the device; disp_v may be NULL. xy, out: host (K, 2) float64.
extern "C" int ictr_flow_gather(const void *disp_u, const void *disp_v, int is_f64, int fields_on_device, int H, int W,
                                const double *xy, int64_t K, double *out) {
  if (!disp_u || H < 1 || W < 1 || K < 0 || (K > 0 && (!xy || !out)))
    return fail(ICTR_ERR_INVALID, "flow_gather: bad arguments");
  if (K == 0) return ICTR_OK;
  if (int rc = need_device()) return rc;
  const size_t fb = (size_t)H * W * (is_f64 ? 8 : 4);
  DevBuf<char> d_f;
  DevBuf<double> d_xy;
  if (int rc = d_xy.alloc(sizeof(double) * 4 * K)) return rc;
  const void *du = disp_u, *dv = disp_v;
  if (!fields_on_device) {
    if (int rc = d_f.alloc(fb * 2)) return rc;
    HIPCHK(hipMemcpy(d_f.get(), disp_u, fb, hipMemcpyHostToDevice));
    if (disp_v) HIPCHK(hipMemcpy(d_f.get() + fb, disp_v, fb, hipMemcpyHostToDevice));
    du = d_f.get();
    dv = disp_v ? d_f.get() + fb : nullptr;
  }
  HIPCHK(hipMemcpy(d_xy.get(), xy, sizeof(double) * 2 * K, hipMemcpyHostToDevice));
  launch_flow_gather(du, dv, is_f64, H, W, d_xy.get(), (int)K, d_xy.get() + 2 * K, nullptr);
  HIPCHK(hipMemcpy(out, d_xy.get() + 2 * K, sizeof(double) * 2 * K, hipMemcpyDeviceToHost));
  return ICTR_OK;
}

// func_OF_util.func_extract_bil_patch (func_OF_util.py:87-129), batched: img host (H, W, C) float64, pts host (K, 2)
// float64 (x, y), out host (K, side, side, C) float64 with side = 2 (pz / 2). Every window must lie inside the image.
extern "C" int ictr_extract_bil_patches(const double *img, int H, int W, int C, const double *pts, int64_t K, int pz,
                                        double *out) {
  const int half = pz / 2;
  if (!img || H < 2 || W < 2 || C < 1 || K < 0 || pz < 2 || (K > 0 && (!pts || !out)))
    return fail(ICTR_ERR_INVALID, "extract_bil_patches: bad arguments");
  for (int64_t k = 0; k < K; ++k) {
    const double fx = floor(pts[2 * k]), fy = floor(pts[2 * k + 1]);
    if (!(fx - half >= 0 && fy - half >= 0 && fx + half < W && fy + half < H))  // taps x0 .. x0 + side (ceil window)
      return fail(ICTR_ERR_INVALID, "extract_bil_patches: the window of point %lld leaves the image", (long long)k);
  }
  if (K == 0) return ICTR_OK;
  if (int rc = need_device()) return rc;
  const size_t ib = sizeof(double) * (size_t)H * W * C, ob = sizeof(double) * (size_t)K * 4 * half * half * C;
  DevBuf<double> d_img, d_pts, d_out;
  if (int rc = d_img.alloc(ib)) return rc;
  if (int rc = d_pts.alloc(sizeof(double) * 2 * K)) return rc;
  if (int rc = d_out.alloc(ob)) return rc;
  HIPCHK(hipMemcpy(d_img.get(), img, ib, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_pts.get(), pts, sizeof(double) * 2 * K, hipMemcpyHostToDevice));
  launch_bil_patches(d_img.get(), H, W, C, d_pts.get(), (int)K, half, d_out.get(), nullptr);
  HIPCHK(hipMemcpy(out, d_out.get(), ob, hipMemcpyDeviceToHost));
  return ICTR_OK;
}

// ---------------------------------------------------------------- PoseClass
struct ictr_pose {
  const ictr_cam *cam;
  const ictr_optparam *op;
  double meanshift[3] = {0, 0, 0};
  double varval = 0;
  float p[6] = {0, 0, 0, 0, 0, 0};
  float G[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
};

extern "C" int ictr_pose_create(ictr_pose **out, const ictr_cam *cam, const ictr_optparam *op) {
  if (!out || !cam || !op) return fail(ICTR_ERR_INVALID, "ictr_pose_create: NULL argument");
  ictr_pose *p = new ictr_pose;
  p->cam = cam;
  p->op = op;
  *out = p;
  return ICTR_OK;
}
extern "C" void ictr_pose_destroy(ictr_pose *pose) { delete pose; }
extern "C" int ictr_pose_setpose_se3(ictr_pose *pose, const double *p_in, const double *meanshift3, double varval) {
  if (!pose || !p_in) return fail(ICTR_ERR_INVALID, "setpose_se3: NULL argument");
  if (pose->op->donorm) {
    if (!meanshift3) return fail(ICTR_ERR_INVALID, "setpose_se3: donorm needs meanshift");
    pose->varval = varval;
    memcpy(pose->meanshift, meanshift3, sizeof(double) * 3);
  }
  host_setpose(pose->op->donorm, p_in, pose->meanshift, pose->varval, pose->p, pose->G);
  return ICTR_OK;
}
extern "C" int ictr_pose_addpose_se3(ictr_pose *pose, const float *dp) {
  if (!pose || !dp) return fail(ICTR_ERR_INVALID, "addpose_se3: NULL argument");
  for (int i = 0; i < 6; ++i) pose->p[i] += dp[i];
  se3_exp<float>(pose->G, pose->p);
  return ICTR_OK;
}
extern "C" int ictr_pose_subpose_se3(ictr_pose *pose, const float *dp) {
  if (!pose || !dp) return fail(ICTR_ERR_INVALID, "subpose_se3: NULL argument");
  for (int i = 0; i < 6; ++i) pose->p[i] -= dp[i];
  se3_exp<float>(pose->G, pose->p);
  return ICTR_OK;
}
extern "C" int ictr_pose_getpose_se3(const ictr_pose *pose, double *p_out) {
  if (!pose || !p_out) return fail(ICTR_ERR_INVALID, "getpose_se3: NULL argument");
  host_getpose(pose->op->donorm, pose->p, pose->G, pose->meanshift, pose->varval, p_out);
  return ICTR_OK;
}
extern "C" int ictr_pose_get_state(const ictr_pose *pose, float *p6, float *G12) {
  if (!pose) return fail(ICTR_ERR_INVALID, "pose is NULL");
  if (p6) memcpy(p6, pose->p, sizeof(float) * 6);
  if (G12) memcpy(G12, pose->G, sizeof(float) * 12);
  return ICTR_OK;
}

static int project_impl(const ictr_pose *pose, const float *pt3d, float *pt3d_rot, float *pt2d, int64_t nopoints,
                        int sc) {
  if (!pose || !pt3d || !pt2d || nopoints < 0 || sc < 0 || sc >= pose->cam->noscales)
    return fail(ICTR_ERR_INVALID, "project_pt: bad arguments");
  if (int rc = need_device()) return rc;
  const int M = pose->op->maxpttrack;
  if (nopoints > M) return fail(ICTR_ERR_INVALID, "project_pt: nopoints > maxpttrack");
  if (nopoints == 0) return ICTR_OK;
  DevBuf<float> buf;
  if (int rc = buf.alloc(sizeof(float) * (size_t)(8 * M + 12))) return rc;
  float *d3 = buf.get(), *dr = d3 + 3 * M, *d2 = d3 + 6 * M, *dG = d3 + 8 * M;
  HIPCHK(hipMemcpy(d3, pt3d, sizeof(float) * 3 * M, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dG, pose->G, sizeof(float) * 12, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d2, pt2d, sizeof(float) * 2 * M, hipMemcpyHostToDevice));
  if (pt3d_rot) HIPCHK(hipMemcpy(dr, pt3d_rot, sizeof(float) * 3 * M, hipMemcpyHostToDevice));
  launch_project_generic(d3, pt3d_rot ? dr : nullptr, d2, (int)nopoints, M, dG, level_cam(pose->cam, sc), nullptr);
  HIPCHK(hipMemcpy(pt2d, d2, sizeof(float) * 2 * M, hipMemcpyDeviceToHost));
  if (pt3d_rot) HIPCHK(hipMemcpy(pt3d_rot, dr, sizeof(float) * 3 * M, hipMemcpyDeviceToHost));
  return ICTR_OK;
}
extern "C" int ictr_pose_project_pt(const ictr_pose *pose, const float *pt3d, float *pt2d, int64_t nopoints, int sc) {
  return project_impl(pose, pt3d, nullptr, pt2d, nopoints, sc);
}
extern "C" int ictr_pose_project_pt_save_rotated(const ictr_pose *pose, const float *pt3d, float *pt3d_rot,
                                                 float *pt2d, int64_t nopoints, int sc) {
  if (!pt3d_rot) return fail(ICTR_ERR_INVALID, "project_pt_save_rotated: pt3d_rot is NULL");
  return project_impl(pose, pt3d, pt3d_rot, pt2d, nopoints, sc);
}

// ---------------------------------------------------------------- batched engine
// How one tracking runs (plan_tracking): the launch form and its geometry, worked out once per tracking from the
// selection bits, the knobs and the sizes. Plain ints, no padding: the graph key holds its bytes.
enum TrackForm : int {  // = ictr_batch_last_path
  kFormLaunches = 0,     // per-iteration launches (ictr_kernels.hip)
  kFormTrack1 = 1,       // the one-launch tracker k_track1 (ictr_track1.hip), one workgroup or a team per problem
  kFormGraph = 2,        // the per-iteration launches replayed as one hipGraph
  kFormTrack1Begin = 3,  // k_track1 that also carries ictr_batch_begin's device part and writes the host mirror
  kFormResident = 4,     // per level: the setup launch, then ONE resident launch for all iterations (ictr_resident.hip)
};
struct TrackPlan {
  int form;          // TrackForm
  int variant;       // selection bits as the launchers see them (ICTR_VARIANT_*, ANY_SIZE forced by a robustness option)
  int team, team_q;  // k_track1: workgroups per problem (1: not the team form), points per workgroup of a team
  int project_here;  // kFormTrack1 without an explicit begin: the launch projects itself and mirrors the final records
  int mute;          // ICTR_VARIANT_DEBUG_MUTE: one workgroup of every problem never posts (time-out tests)
  ResidentGeom res;  // kFormResident: worker workgroups per pair, pairs in flight, patches per wave
  int setup_cpw[16], setup_gridx8[16];  // kFormResident: points per wave chunk and workgroups of each level's setup
};
// device mailbox of an in-launch exchange; it grows, never shrinks
struct Mailbox {
  DevBuf<unsigned long long> d;
  size_t bytes = 0;
  unsigned epoch = 0;  // of the last launch on it (ictr_xchg.h)
};
struct ProbHost {
  int npts = 0;
  double meanshift[3] = {0, 0, 0};
  double varval = 0;
  float p[6] = {0, 0, 0, 0, 0, 0};
  float G[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  const ictr_pyramid *ref = nullptr, *cur = nullptr;
  bool pose_set = false;
  int iters = 0;
};

struct ictr_batch {
  const ictr_cam *cam = nullptr;
  const ictr_optparam *op = nullptr;
  int B = 0, M = 0, n = 0, nlev = 0, P = 0;
  hipStream_t stream = nullptr;
  int variant = 0;
  int robust = 0;        // ICTR_ROBUST_* (off by default)
  float huber_k = 0.0f;
  int sharded = 0;
  int gridx = 1;
  int cpw = 64, gridx8 = 1;  // P=8 fast path: points per wave chunk, workgroups per problem
  bool trace_on = false;
  bool projected = false;
  // device
  DevBuf<float> d_pt3d, d_pt3d_ref, d_pt2d, d_T, d_Gx, d_Gy, d_coef, d_partH, d_partb, d_red_own;
  float *d_red = nullptr;  // d_red_own, or the caller's (ictr_batch_set_reduction_buffer)
  DevBuf<ProbState> d_st;  // the records, and behind them the plane table ...
  PlaneSet *d_planes = nullptr;  // ... (inside d_st's block, up_planes_offset)
  DevBuf<ictr_trace_rec> d_trace;
  DevBuf<int> d_trace_count;
  int trace_cap = 0;
  // host mirrors
  std::vector<ProbHost> probs;
  std::vector<ProbState> h_st;
  std::vector<PlaneSet> h_planes;
  std::vector<float> h_pt2d;  // Get2DPoints mirror of problem 0 (or scratch)
  std::vector<float> h_stage;
  // optional HIP-event timing (bench.py): per level e0 -> setup kernel -> e1 -> iteration launches -> e2
  bool timing = false;
  std::vector<Event> ev;  // 3 per level
  std::vector<char> ev_used;
  std::vector<Event> evk;  // 2 per (level, iteration): around the accumulate kernel alone
  int evk_iters = 0;
  bool evk_valid = true;  // the per-iteration kernel events of the last tracking were recorded (not in the resident form)
  ResXchg xchg = {};  // sharded resident form (ictr_batch_set_peer_exchange): xchg.world > 1 = the resident launches sum
                     // H and b over the ranks themselves
  DevBuf<unsigned> d_xseq;  // [B] exchange counters of that form
  int otf = 0;       // every reference pyramid of the current tracking is builder-made (1), and some of them image-only
                     // (2): see EngineDev.otf
  int maxpts = 0;    // largest nopoints over the problems of the current tracking (set by ictr_batch_begin)
  TrackPlan plan = {};  // of the last tracking (plan_tracking)
  // the per-iteration launch sequence of one tracking as an instantiated hipGraph (launch-bound sizes, enqueue_levels)
  hipGraphExec_t gexec = nullptr;
  std::string gkey;               // everything the captured launches depend on; a change rebuilds the graph
  hipStream_t cap_stream = nullptr;  // capture needs a non-null stream; nothing ever executes on it
  bool graph_broken = false;      // capture / instantiate failed once: plain launches from then on
  int phase_it = 0;  // iteration counter of the phase API (event slot of the next iter_accumulate)
  // results of the last track_async: the final states are copied to pinned host memory in-stream and an event marks
  // the end, so that get_poses / the timing getters wait for THIS tracking only and the caller may already have
  // enqueued the next one on the same stream (another engine): the host runs one step ahead of the GPU
  PinBuf<ProbState> h_st_pin;
  ProbState *d_st_mirror = nullptr;  // h_st_pin as the device sees it (the one-launch tracker stores final states there)
  PinBuf<char> h_up_pin;  // pinned staging of the per-tracking uploads (states + plane table): truly asynchronous
  // mailboxes of the in-launch exchanges, allocated on first use (exchange_prepare): the team form of the one-launch
  // tracker ([B][2][team][32] granules, ictr_track1.hip "Teams") and the resident-iteration form (per slot a gather box
  // and a broadcast box, ictr_resident.hip)
  Mailbox team_mail, res_mail;
  int team_target = 0;        // points per workgroup aimed at (0: automatic, < 0: no teams); ictr_batch_set_team
  int team_lo = 128, team_hi = 8192;  // problem sizes (points) served by teams: lo < maxpts <= hi
  PinBuf<int> h_team_err;     // an exchange of some launch timed out (sticky)
  int *d_team_err = nullptr;  // ... as the device sees it
  Event done_ev, up_ev;
  bool done_valid = false, up_pending = false;
  ~ictr_batch() {  // the graph and its capture stream go before any buffer
    if (gexec) (void)hipGraphExecDestroy(gexec);
    if (cap_stream) (void)hipStreamDestroy(cap_stream);
  }
};

// the plane table's place behind the B records in their common device block / staging buffer (16-byte aligned)
static size_t up_planes_offset(int B) { return (sizeof(ProbState) * (size_t)B + 15) / 16 * 16; }
int ictr::env_int(const char *name, int dflt) {
  const char *s = getenv(name);
  return s ? atoi(s) : dflt;
}

// kernel-selection bits as the launchers see them: any robustness option routes P = 8 through the any-size kernels
static int engine_variant(const ictr_batch *b) { return b->variant | (b->robust ? ICTR_VARIANT_ANY_SIZE : 0); }

static EngineDev engine_dev(const ictr_batch *b) {
  EngineDev e;
  memset(&e, 0, sizeof(e));  // (graph_key compares its bytes)
  e.B = b->B;
  e.M = b->M;
  e.P = b->P;
  e.n = b->n;
  e.nlev = b->nlev;
  e.lv_f = b->op->lv_f;
  e.lv_l = b->op->lv_l;
  e.maxiter = b->op->maxiter;
  e.ratio = b->op->normdp_ratio;
  e.dopatchnorm = b->op->dopatchnorm ? 1 : 0;
  e.sharded = b->sharded;
  e.otf = b->otf;
  e.robust = b->robust;
  e.huber_k = b->huber_k;
  e.pt3d = b->d_pt3d.get();
  e.pt3d_ref = b->d_pt3d_ref.get();
  e.pt2d = b->d_pt2d.get();
  e.T = b->d_T.get();
  e.Gx = b->d_Gx.get();
  e.Gy = b->d_Gy.get();
  e.coef = b->d_coef.get();
  e.st = b->d_st.get();
  e.planes = b->d_planes;
  e.partH = b->d_partH.get();
  e.partb = b->d_partb.get();
  e.red = b->d_red;
  e.trace.rec = b->trace_on ? b->d_trace.get() : nullptr;
  e.trace.count = b->d_trace_count.get();
  e.trace.capacity = b->trace_cap;
  return e;
}

static int check_op(const ictr_optparam *op, const ictr_cam *cam) {
  if (op->psz < 1 || op->psz > 64) return fail(ICTR_ERR_INVALID, "psz must be 1..64");
  if (op->novals != op->psz * op->psz || op->pszd2 != op->psz / 2)
    return fail(ICTR_ERR_INVALID, "optparam derived fields inconsistent (use ictr_optparam_init)");
  if (op->lv_l < 0 || op->lv_f < op->lv_l || op->lv_f >= cam->noscales)
    return fail(ICTR_ERR_INVALID, "need 0 <= lv_l <= lv_f < cam.noscales");
  if (op->maxpttrack < 1) return fail(ICTR_ERR_INVALID, "maxpttrack must be >= 1");
  if (cam->padding < op->psz) return fail(ICTR_ERR_INVALID, "camera padding must be >= psz");
  return ICTR_OK;
}

extern "C" int ictr_batch_create(ictr_batch **out, const ictr_cam *cam, const ictr_optparam *op, int64_t nproblems) {
  if (!out || !cam || !op || nproblems < 1 || nproblems > 65535)
    return fail(ICTR_ERR_INVALID, "batch_create: bad arguments (1..65535 problems)");
  if (int rc = check_op(op, cam)) return rc;
  if (int rc = need_device()) return rc;
  auto b = std::make_unique<ictr_batch>();
  b->cam = cam;
  b->op = op;
  b->B = (int)nproblems;
  b->M = op->maxpttrack;
  b->P = op->psz;
  b->n = op->novals;
  b->nlev = op->lv_f + 1;
  b->team_target = env_int("ICTR_TEAM_TARGET", 0);  // 0: automatic (team_points), < 0: never
  b->team_lo = env_int("ICTR_TEAM_MINPTS", 128);    // up to here ONE workgroup per problem is as fast (tools/team_sweep.py)
  b->team_hi = env_int("ICTR_TEAM_MAXPTS", 8192);   // beyond: the per-iteration kernels
  const size_t B = b->B, M = b->M, n = b->n, L = b->nlev;
  const int ppw = (b->n <= 64 && 64 % b->n == 0) ? 64 / b->n : 1;
  const int64_t groups = (b->M + ppw - 1) / ppw;
  // workgroups per problem: enough to cover the points once, capped so that B problems together stay near
  // 256 CUs x 8 resident workgroups x 2 (the rest is grid-strided)
  const int64_t cap = std::min<int64_t>(kMaxGridX, std::max<int64_t>(64, 2 * kMaxGridX / (int64_t)B));
  b->gridx = (int)std::min<int64_t>(std::max<int64_t>((groups + kWaves - 1) / kWaves, 1), cap);
  b->trace_cap = std::max(1, (int)L * std::max(1, op->maxiter));
  if (int rc = b->d_pt3d.alloc(sizeof(float) * B * 3 * M, true)) return rc;
  if (int rc = b->d_pt3d_ref.alloc(sizeof(float) * B * 3 * M, true)) return rc;
  if (int rc = b->d_pt2d.alloc(sizeof(float) * B * L * 2 * M, true)) return rc;
  if (int rc = b->d_T.alloc(sizeof(float) * B * M * n, true)) return rc;
  if (int rc = b->d_Gx.alloc(sizeof(float) * B * M * n, true)) return rc;
  if (int rc = b->d_Gy.alloc(sizeof(float) * B * M * n, true)) return rc;
  if (int rc = b->d_coef.alloc(sizeof(float) * B * M * kCoefStride, true)) return rc;
  if (int rc = b->d_partH.alloc(sizeof(float) * B * b->gridx * kPartHStride, true)) return rc;
  if (int rc = b->d_partb.alloc(sizeof(float) * B * b->gridx * kPartBStride, true)) return rc;
  if (int rc = b->d_red_own.alloc(sizeof(float) * B * kRedStride, true)) return rc;
  b->d_red = b->d_red_own.get();
  // the records and the plane table in ONE block: one upload per SetPose round instead of two (each small transfer is an
  // engine switch of 5-8 us in front of the tracking's first kernel)
  if (int rc = b->d_st.alloc(up_planes_offset(B) + sizeof(PlaneSet) * B * L, true)) return rc;
  b->d_planes = reinterpret_cast<PlaneSet *>(reinterpret_cast<char *>(b->d_st.get()) + up_planes_offset(B));
  if (int rc = b->d_trace.alloc(sizeof(ictr_trace_rec) * b->trace_cap, true)) return rc;
  if (int rc = b->d_trace_count.alloc(sizeof(int), true)) return rc;
  if (int rc = b->h_st_pin.alloc(sizeof(ProbState) * B)) return rc;
  if (int rc = b->h_up_pin.alloc(up_planes_offset(B) + sizeof(PlaneSet) * B * L)) return rc;
  if (hipHostGetDevicePointer((void **)&b->d_st_mirror, b->h_st_pin.get(), 0) != hipSuccess) {
    (void)hipGetLastError();
    b->d_st_mirror = nullptr;  // no mapped view: final states come back by copy
  }
  if (int rc = b->done_ev.create(hipEventDisableTiming)) return rc;
  if (int rc = b->up_ev.create(hipEventDisableTiming)) return rc;
  b->probs.resize(B);
  b->h_st.resize(B);
  b->h_planes.resize(B * L);
  b->h_pt2d.assign(2 * M, 0.0f);
  b->h_stage.assign(3 * M, 0.0f);
  *out = b.release();
  return ICTR_OK;
}
extern "C" void ictr_batch_destroy(ictr_batch *b) { delete b; }
extern "C" int ictr_batch_set_stream(ictr_batch *b, void *hip_stream) {
  if (!b) return fail(ICTR_ERR_INVALID, "batch is NULL");
  b->stream = (hipStream_t)hip_stream;
  return ICTR_OK;
}
extern "C" int ictr_batch_set_robust(ictr_batch *b, int flags, float huber_k) {
  if (!b) return fail(ICTR_ERR_INVALID, "batch is NULL");
  if (flags & ~(ICTR_ROBUST_CLEAN | ICTR_ROBUST_COMPOSE | ICTR_ROBUST_HUBER))
    return fail(ICTR_ERR_INVALID, "set_robust: unknown flag bits 0x%x", flags);
  if ((flags & ICTR_ROBUST_HUBER) && !(huber_k > 0.0f))
    return fail(ICTR_ERR_INVALID, "set_robust: the Huber threshold must be positive");
  b->robust = flags;
  b->huber_k = huber_k;
  return ICTR_OK;
}
extern "C" int ictr_batch_set_team(ictr_batch *b, int target_points, int min_points, int max_points) {
  if (!b) return fail(ICTR_ERR_INVALID, "batch is NULL");
  if (min_points < 0 || max_points < min_points)
    return fail(ICTR_ERR_INVALID, "set_team: need 0 <= min_points <= max_points");
  b->team_target = target_points;
  b->team_lo = min_points;
  b->team_hi = max_points;
  return ICTR_OK;
}
// Sharded resident form: the batch holds this rank's SHARD of every problem's points; its resident-iteration launches
// then add H (once per level) and b (once per iteration) over the ranks themselves -- the solver workgroup of a frame
// pair writes its sums into every rank's mailbox and polls its own (ictr_p2p.hip's one-hop protocol, inside the launch).
// p: a connected ictr_p2p of at least 64 granules per problem, the same on every rank; NULL: back to a plain batch.
// Every rank must track the same sequence of (problems, levels, iteration limits); the ranks' loop decisions stay in
// lockstep because every rank solves on identical sums. Needs the resident form (8x8 patches, no robustness option, no
// patch normalisation); a tracking that cannot take it fails with ICTR_ERR_STATE rather than run unsynchronised.
extern "C" int ictr_batch_set_peer_exchange(ictr_batch *b, ictr_p2p *p) {
  if (!b) return fail(ICTR_ERR_INVALID, "batch is NULL");
  if (!p) {
    memset(&b->xchg, 0, sizeof(b->xchg));
    return ICTR_OK;
  }
  ResXchg x;
  if (ictr_p2p_fill_xchg_(p, &x)) return fail(ICTR_ERR_STATE, "set_peer_exchange: the p2p object is not connected");
  if (x.cap < (long long)kXchgPerPair * b->B)
    return fail(ICTR_ERR_INVALID, "set_peer_exchange: the mailboxes hold %lld granules per rank, %d x %d needed", x.cap,
                kXchgPerPair, b->B);
  if (!b->d_xseq)
    if (int rc = b->d_xseq.alloc(sizeof(unsigned) * b->B)) return rc;
  HIPCHK(hipMemsetAsync(b->d_xseq.get(), 0, sizeof(unsigned) * b->B, b->stream));
  x.xseq = b->d_xseq.get();
  b->xchg = x;
  return ICTR_OK;
}

extern "C" int ictr_batch_set_variant(ictr_batch *b, int variant) {
  if (!b) return fail(ICTR_ERR_INVALID, "batch is NULL");
  if (variant & ~ICTR_SELECT_ALL)
    return fail(ICTR_ERR_INVALID, "set_variant: unknown selection bits 0x%x (known: ICTR_VARIANT_ANY_SIZE, H_BY_SETUP, "
                                  "LAUNCHES, ONE_LAUNCH, NO_GRAPH, SEPARATE_BEGIN, NO_TEAMS, NO_RESIDENT, DEBUG_MUTE, "
                                  "GRAD_PLANES, DYNAMIC_LOOP, ICTR_REF8_DIRECT_TAPS = 0x%x)", variant & ~ICTR_SELECT_ALL, ICTR_SELECT_ALL);
  b->variant = variant;
  return ICTR_OK;
}

// odometer.cpp:171-239 (ResetOdometer + normalisation + f64->f32 SoA).
// given_ms/given_var: normalisation computed elsewhere (sharded runs need the GLOBAL mean / variance).
static int set3dpoints_impl(ictr_batch *b, int64_t problem, double *pt_in, int64_t nopoints_in, const double *given_ms,
                            double given_var) {
  if (!b || problem < 0 || problem >= b->B || nopoints_in < 0 || (nopoints_in > 0 && !pt_in))
    return fail(ICTR_ERR_INVALID, "set3dpoints: bad arguments");
  ProbHost &ph = b->probs[problem];
  const size_t M = b->M, n = b->n;
  // ResetOdometer (odometer.cpp:580-609): patch / sd state of this problem back to zero
  HIPCHK(hipMemsetAsync(b->d_T.get() + problem * M * n, 0, sizeof(float) * M * n, b->stream));
  HIPCHK(hipMemsetAsync(b->d_Gx.get() + problem * M * n, 0, sizeof(float) * M * n, b->stream));
  HIPCHK(hipMemsetAsync(b->d_Gy.get() + problem * M * n, 0, sizeof(float) * M * n, b->stream));
  HIPCHK(hipMemsetAsync(b->d_coef.get() + problem * M * kCoefStride, 0, sizeof(float) * M * kCoefStride, b->stream));
  ph.meanshift[0] = ph.meanshift[1] = ph.meanshift[2] = 0;
  ph.varval = 0;
  ph.npts = (int)std::min<int64_t>(nopoints_in, b->M);
  ph.pose_set = false;
  const int np = ph.npts;
  double *p1 = pt_in, *p2 = pt_in + nopoints_in, *p3 = pt_in + 2 * nopoints_in;
  std::fill(b->h_stage.begin(), b->h_stage.end(), 0.0f);
  float *s = b->h_stage.data();
  if (b->op->donorm) {
    const double nd = (double)np;
    if (given_ms) {
      memcpy(ph.meanshift, given_ms, sizeof(double) * 3);
    } else {
      for (int i = 0; i < np; ++i) ph.meanshift[0] += p1[i];
      for (int i = 0; i < np; ++i) ph.meanshift[1] += p2[i];
      for (int i = 0; i < np; ++i) ph.meanshift[2] += p3[i];
      ph.meanshift[0] /= nd;
      ph.meanshift[1] /= nd;
      ph.meanshift[2] /= nd;
    }
    for (int i = 0; i < np; ++i) {  // writes back into the caller's array, like odometer.cpp:207-212
      p1[i] -= ph.meanshift[0];
      p2[i] -= ph.meanshift[1];
      p3[i] -= ph.meanshift[2];
      ph.varval += p1[i] * p1[i] + p2[i] * p2[i] + p3[i] * p3[i];
    }
    ph.varval /= nd;  // mean squared radius (no sqrt), odometer.cpp:214
    if (given_ms) ph.varval = given_var;
    for (int i = 0; i < np; ++i) {
      s[i] = (float)(p1[i] / ph.varval);
      s[i + M] = (float)(p2[i] / ph.varval);
      s[i + 2 * M] = (float)(p3[i] / ph.varval);
    }
  } else {
    for (int i = 0; i < np; ++i) {
      s[i] = (float)p1[i];
      s[i + M] = (float)p2[i];
      s[i + 2 * M] = (float)p3[i];
    }
  }
  HIPCHK(hipMemcpyAsync(b->d_pt3d.get() + problem * 3 * M, s, sizeof(float) * 3 * M, hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));  // h_stage is reused by the next call
  return ICTR_OK;
}
extern "C" int ictr_batch_set3dpoints(ictr_batch *b, int64_t problem, double *pt_in, int64_t nopoints_in) {
  return set3dpoints_impl(b, problem, pt_in, nopoints_in, nullptr, 0.0);
}
extern "C" int ictr_batch_set3dpoints_norm(ictr_batch *b, int64_t problem, double *pt_in, int64_t nopoints_in,
                                           const double *meanshift3, double varval) {
  if (!meanshift3) return fail(ICTR_ERR_INVALID, "set3dpoints_norm: meanshift is NULL");
  return set3dpoints_impl(b, problem, pt_in, nopoints_in, meanshift3, varval);
}
extern "C" int ictr_batch_get_norm(const ictr_batch *b, int64_t problem, double *meanshift3, double *varval) {
  if (!b || problem < 0 || problem >= b->B) return fail(ICTR_ERR_INVALID, "get_norm: bad arguments");
  if (meanshift3) memcpy(meanshift3, b->probs[problem].meanshift, sizeof(double) * 3);
  if (varval) *varval = b->probs[problem].varval;
  return ICTR_OK;
}

extern "C" int ictr_batch_setpose(ictr_batch *b, int64_t problem, const double *p_in, const ictr_pyramid *pyr_ref,
                                  const ictr_pyramid *pyr_new) {
  if (!b || problem < 0 || problem >= b->B || !p_in || !pyr_ref || !pyr_new)
    return fail(ICTR_ERR_INVALID, "setpose: bad arguments");
  for (const ictr_pyramid *py : {pyr_ref, pyr_new}) {
    if (py->nlev < b->nlev || py->pad != b->cam->padding)
      return fail(ICTR_ERR_INVALID, "setpose: pyramid has %d levels / pad %d, engine needs %d / %d", py->nlev, py->pad,
                  b->nlev, b->cam->padding);
    for (int l = 0; l < b->nlev; ++l)
      if (py->sw[l] != (int)b->cam->sw[l] || py->sh[l] < (int)b->cam->sh[l])
        return fail(ICTR_ERR_INVALID, "setpose: pyramid level %d is %dx%d, camera expects %dx%d", l, py->sw[l],
                    py->sh[l], (int)b->cam->sw[l], (int)b->cam->sh[l]);
  }
  if (!pyr_ref->getgrad) return fail(ICTR_ERR_INVALID, "setpose: reference pyramid has no gradients");
  ProbHost &ph = b->probs[problem];
  host_setpose(b->op->donorm, p_in, ph.meanshift, ph.varval, ph.p, ph.G);
  ph.ref = pyr_ref;
  ph.cur = pyr_new;
  ph.pose_set = true;
  b->projected = false;
  return ICTR_OK;
}

// SetPose for every problem of the batch in one call: p_all[6 * nproblems], one frame pair shared by all (the
// run_track_nposes shape: every pose sample tracks the same pair, run_track_nposes.cpp:232-258)
extern "C" int ictr_batch_setpose_all(ictr_batch *b, const double *p_all, const ictr_pyramid *pyr_ref,
                                      const ictr_pyramid *pyr_new) {
  if (!b || !p_all) return fail(ICTR_ERR_INVALID, "setpose_all: bad arguments");
  for (int64_t k = 0; k < b->B; ++k)
    if (int rc = ictr_batch_setpose(b, k, p_all + 6 * k, pyr_ref, pyr_new)) return rc;
  return ICTR_OK;
}

// ICTR_CPW: points per wave chunk of the 8x8 / 4x4 fast paths, forced (experiments, tests); 0 = the host picks
static int cpw_forced() {
  const char *env = getenv("ICTR_CPW");
  const int v = env ? atoi(env) : 0;
  return v >= 1 && v <= 64 ? v : 0;
}
// ictr_batch_begin, host part: initial states, plane table and launch geometry of the coming tracking
static int begin_prepare(ictr_batch *b) {
  if (int rc = check_op(b->op, b->cam)) return rc;
  if (b->op->maxpttrack != b->M || b->op->psz != b->P || b->op->lv_f + 1 != b->nlev)
    return fail(ICTR_ERR_STATE, "optparam maxpttrack/psz/lv_f changed after creation");
  b->done_valid = false;
  b->phase_it = 0;
  bool all_builder = true, any_image_only = false;
  if (b->timing) std::fill(b->ev_used.begin(), b->ev_used.end(), 0);
  int maxpts = 0;
  for (int i = 0; i < b->B; ++i) {
    const ProbHost &ph = b->probs[i];
    if (!ph.pose_set) return fail(ICTR_ERR_STATE, "problem %d: SetPose has not been called", i);
    ProbState &st = b->h_st[i];
    memset(&st, 0, sizeof(st));
    memcpy(st.p, ph.p, sizeof(st.p));
    memcpy(st.G, ph.G, sizeof(st.G));
    st.npts = ph.npts;
    st.normdp = st.normdp_init = 1e-10f;
    maxpts = std::max(maxpts, ph.npts);
    for (int l = 0; l < b->nlev; ++l) {
      PlaneSet &ps = b->h_planes[(size_t)i * b->nlev + l];
      ps.ref = ph.ref->img[l];
      ps.dx = ph.ref->dx[l];
      ps.dy = ph.ref->dy[l];
      ps.cur = ph.cur->img[l];
      ps.pack = ph.ref->pack[l];
    }
    if (!ph.ref->builder_made) all_builder = false;
    if (ph.ref->getgrad == 2) any_image_only = true;
  }
  // setpose refuses a reference without gradients (getgrad 0), and every other pyramid that is not image-only carries
  // the packed planes: they are there exactly when otf != 2
  if (any_image_only && !all_builder)
    return fail(ICTR_ERR_STATE, "a batch cannot mix image-only reference pyramids (getgrad = 2) with pyramids made from "
                                "caller-supplied planes: the setup kernel reads either the planes or the image, for all "
                                "problems of a launch");
  b->otf = !all_builder ? 0 : (any_image_only ? 2 : 1);

  b->maxpts = maxpts;
  {
    // P=8 fast path geometry: a wave owns `cpw` consecutive points. Small problems get small chunks (more
    // waves, latency hidden by occupancy); large batches get 64-point chunks (coalesced stage 1, deep ILP).
    const int64_t total = (int64_t)std::max(maxpts, 1) * b->B;
    int cpw = 4;
    while (cpw < 64 && total / cpw > 32768) cpw *= 2;
    if (const int v = cpw_forced()) cpw = v;
    b->cpw = cpw;
    const int64_t chunks = ((int64_t)std::max(maxpts, 1) + cpw - 1) / cpw;
    const int64_t want = (chunks + kWaves - 1) / kWaves;
    const int64_t capx = std::max<int64_t>(1, (int64_t)b->gridx);  // partial buffers are sized for gridx blocks
    b->gridx8 = (int)std::min<int64_t>(std::max<int64_t>(want, 1), capx);
    if (b->gridx8 >= 64)  // multiple of 8: XCD-aware order (xcd_band_block)
      b->gridx8 = (int)std::min<int64_t>((b->gridx8 + 7) / 8 * 8, capx / 8 * 8);
  }
  if (b->otf == 2 && (b->P != 8 || b->robust || (engine_variant(b) & ICTR_VARIANT_ANY_SIZE)))
    return fail(ICTR_ERR_STATE, "a reference pyramid without gradient planes (getgrad = 2: gradients formed on the fly) is "
                                "served by the 8x8 setup kernel k_ref8 only: psz 8, no robustness option, variant bit 1 "
                                "clear (small problems then run the per-iteration launches instead of the one-launch "
                                "tracker)");
  return ICTR_OK;
}
// ... device part: upload states + plane table, clear the trace counter, run step 3 for every problem
static int begin_device(ictr_batch *b, bool project = true) {
  const int maxpts = project ? b->maxpts : 0;  // (!project: the tracking's own launch projects, see track_enqueue)
  {
    const size_t nst = sizeof(ProbState) * b->B, npl = sizeof(PlaneSet) * b->h_planes.size();
    if (b->up_pending) HIPCHK(hipEventSynchronize(b->up_ev.get()));  // the previous upload has left the staging buffer
    const size_t off = up_planes_offset(b->B);
    memcpy(b->h_up_pin.get(), b->h_st.data(), nst);
    memcpy(b->h_up_pin.get() + off, b->h_planes.data(), npl);
    // (d_planes follows d_st)
    HIPCHK(hipMemcpyAsync(b->d_st.get(), b->h_up_pin.get(), off + npl, hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipEventRecord(b->up_ev.get(), b->stream));
    b->up_pending = true;
  }
  if (maxpts > 0) {  // (the launch also clears the trace counter)
    LevelCam cams[16];
    for (int l = 0; l < b->nlev; ++l) cams[l] = level_cam(b->cam, l);
    launch_project_ref(engine_dev(b), cams, maxpts, b->stream);
  } else {
    HIPCHK(hipMemsetAsync(b->d_trace_count.get(), 0, sizeof(int), b->stream));
  }
  HIPCHK(hipGetLastError());
  return ICTR_OK;
}
extern "C" int ictr_batch_begin(ictr_batch *b) {
  if (!b) return fail(ICTR_ERR_INVALID, "batch is NULL");
  if (int rc = begin_prepare(b)) return rc;
  if (int rc = begin_device(b)) return rc;
  b->projected = true;
  return ICTR_OK;
}

extern "C" int ictr_batch_enable_sharding(ictr_batch *b, int enable) {
  if (!b) return fail(ICTR_ERR_INVALID, "batch is NULL");
  b->sharded = enable ? 1 : 0;
  return ICTR_OK;
}
extern "C" float *ictr_batch_reduction_buffer(ictr_batch *b) { return b ? b->d_red : nullptr; }

// Launch geometry of one level's kernels. p: the tracking's plan (NULL: the phase API, which has none) -- the setup
// launches of the resident form have a chunk size of their own (resident_setup_plan)
static LevelLaunch level_launch(const ictr_batch *b, const TrackPlan *p, int level) {
  const bool res = p && p->form == kFormResident;
  LevelLaunch ll;
  ll.level = level;
  ll.variant = p ? p->variant : engine_variant(b);
  ll.gridx = b->gridx;
  ll.cpw = res ? p->setup_cpw[level] : b->cpw;
  ll.gridx8 = res ? p->setup_gridx8[level] : b->gridx8;
  return ll;
}
static int level_ok(ictr_batch *b, int level) {
  if (!b) return fail(ICTR_ERR_INVALID, "batch is NULL");
  if (!b->projected) return fail(ICTR_ERR_STATE, "ictr_batch_begin has not run since the last SetPose");
  if (level < b->op->lv_l || level > b->op->lv_f) return fail(ICTR_ERR_INVALID, "level out of range");
  return ICTR_OK;
}
// 1: the level phase leaves a partial H in the reduction buffer that must be summed over ranks before level_finish;
// 0 (P = 8 fast path, deferred H): H travels with the first iteration's b, the level phase needs no collective
extern "C" int ictr_batch_level_allreduce_needed(ictr_batch *b) {
  if (!b) return 1;
  return defer_h(engine_dev(b), engine_variant(b)) ? 0 : 1;
}
extern "C" int ictr_batch_level_accumulate(ictr_batch *b, int level) {
  if (int rc = level_ok(b, level)) return rc;
  b->phase_it = 0;
  launch_ref_level(engine_dev(b), level_cam(b->cam, level), level_launch(b, nullptr, level), true, b->stream);
  HIPCHK(hipGetLastError());
  return ICTR_OK;
}
extern "C" int ictr_batch_level_finish(ictr_batch *b, int level) {
  if (int rc = level_ok(b, level)) return rc;
  b->phase_it = 0;
  if (b->sharded) launch_level_finish(engine_dev(b), level_launch(b, nullptr, level), b->stream);
  HIPCHK(hipGetLastError());
  return ICTR_OK;
}
extern "C" int ictr_batch_iter_accumulate(ictr_batch *b, int level) {
  if (int rc = level_ok(b, level)) return rc;
  // with timing on, HIP events bracket the accumulate kernel alone, as in the fused run (get_kernel_times)
  const bool tk = b->timing && b->phase_it < b->evk_iters && (int)b->evk.size() >= 2 * b->nlev * b->evk_iters;
  const EngineDev e = engine_dev(b);
  const LevelCam lc = level_cam(b->cam, level);
  const LevelLaunch ll = level_launch(b, nullptr, level);
  const int first = b->phase_it == 0;
  const int ke = 2 * (level * b->evk_iters + b->phase_it);
  launch_iter_main(e, lc, ll, first, b->stream, tk ? b->evk[ke].get() : nullptr, tk ? b->evk[ke + 1].get() : nullptr);
  if (tk && b->phase_it + 1 == std::min(b->op->maxiter, b->evk_iters)) b->ev_used[level] = 2;  // kernel events complete
  b->phase_it++;
  launch_iter_tail(e, ll, first, b->stream);
  HIPCHK(hipGetLastError());
  return ICTR_OK;
}
extern "C" int ictr_batch_iter_finish(ictr_batch *b, int level) {
  if (int rc = level_ok(b, level)) return rc;
  if (b->sharded) launch_iter_finish(engine_dev(b), level_launch(b, nullptr, level), b->phase_it == 1, b->stream);
  HIPCHK(hipGetLastError());
  return ICTR_OK;
}

// ---------------------------------------------------------------- launch forms of a batch tracking
// CUs of the calling thread's current device, queried once per device
int ictr::cu_count() {
  static std::atomic<int> n_cu[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
    (void)hipGetLastError();
    dev = 0;
  }
  int v = n_cu[dev].load(std::memory_order_relaxed);
  if (v == 0) {
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1) {
      (void)hipGetLastError();
      v = 256;
    }
    n_cu[dev].store(v, std::memory_order_relaxed);
  }
  return v;
}

// Always the same workgroup shape of the one-launch tracker: which wave owns which patch -- and with it the order of every
// sum -- then depends on the problem's own point count only, so a problem gives the same bits whatever else shares its
// launch (run_track_nposes: any split of the pose samples over batches or ranks writes the same file).
constexpr int kTrack1Waves = 8;
constexpr int kTeamMaxWorkgroups = 4096;  // workgroups of one team launch

// Team form ("Teams", ictr_track1.hip): 8x8 problems above the one-workgroup range are shared by several workgroups
// that all-gather their partial sums through a device mailbox -- still one launch per tracking.
// Points per workgroup aimed at for the current tracking; 0 = no teams. Explicit (ictr_batch_set_team, ICTR_TEAM_TARGET):
// a function of the problem size alone. Automatic (measured, tools/team_sweep.py, profiles/r02_notes.md): a lone problem
// is fastest in shares of 40 points (five patches per wave; the all-gather of up to 64 shares is one round trip);
// a batch wants all its workgroups resident at once, one per CU, down to the largest share whose patches fit the LDS
// (160 points); when even that does not fit the chip, problems of up to 384 points go back to one workgroup each
// (two per CU in the 128-register build), larger ones take the smallest team.
static int team_points(const ictr_batch *b) {
  if (b->team_target != 0) return b->team_target >= 8 ? b->team_target : 0;
  const int n = b->maxpts;
  const int upper = std::min(64, (n + 39) / 40), lower = (n + 159) / 160;
  const int fit = std::max(1, cu_count() / std::max(1, b->B));
  if (fit < lower && n <= 384) return 0;
  const int team = std::min(upper, std::max(lower, fit));
  return team < 2 ? 0 : (n + team - 1) / team;
}
// workgroups per problem of the team form for the current tracking (1: not the team form); *q: points per workgroup
static int track1_team(const ictr_batch *b, int *q) {
  if (b->P != 8 || (engine_variant(b) & ICTR_VARIANT_ANY_SIZE)) return 1;  // teams: the lean 8x8 form only
  if (b->maxpts <= b->team_lo || b->maxpts > b->team_hi) return 1;
  if ((int64_t)b->nlev * (1 + std::max(0, b->op->maxiter)) >= kXchgMaxSeq) return 1;  // exchange number of the tag
  const int target = team_points(b);
  if (target < 1) return 1;
  const int team = track1_team_size(b->maxpts, target);
  if (team < 2 || (int64_t)team * b->B > kTeamMaxWorkgroups) return 1;
  *q = track1_team_q(b->maxpts, target);
  return team;
}

// Resident-iteration form (ictr_resident.hip): problems of thousands of 8x8 patches run all iterations of a level in
// ONE launch with their templates resident in registers -- `parts` worker workgroups of 128 points + one solver
// workgroup per frame pair, `slots` pairs in flight -- instead of streaming T/Gx/Gy from HBM in every iteration. Needs
// every workgroup of the launch resident at once: slots * (parts + 1) <= CUs * occupancy. Taken for problems of at least
// 8193 points, and for batches of mid-size problems with >= 48 000 points together, which also run faster here than as
// teams of the one-launch tracker (r03: 64 x 1000 points 0.88 -> 0.76 ms, 16 x 3000 0.91 -> 0.56, 12 x 4000 0.91 ->
// 0.56, 8 x 6000 0.97 -> 0.58, 128 x 500 0.85 -> 0.75, 256 x 1000 3.39 -> 2.06; below that total the teams win: 8 x 5000
// 0.49 against 0.53, 16 x 2500 0.49 / 0.54, 32 x 800 0.43 / 0.48; so do problems of 300 points at any batch size).
// Fills p->res; false: not this form.
static bool resident_plan(const ictr_batch *b, TrackPlan *p) {
  if (b->P != 8 || b->robust || b->sharded || b->op->dopatchnorm || b->op->maxiter < 1) return false;
  const bool xchg = b->xchg.world > 1;  // sharded resident form: any shard size (an empty shard still runs its solvers)
  const bool big_batch = b->maxpts >= 500 && (int64_t)b->B * b->maxpts >= 48000;
  if (b->maxpts < 8193 && !xchg && !big_batch) return false;
  static const int max_slots = env_int("ICTR_RESIDENT_SLOTS", 1 << 20);  // experiments: pairs in flight per launch
  // sixteen patches per wave (twice the workgroups, half the patch loop) when ALL pairs of the batch are then in flight
  // at once; thirty-two (the most templates a CU can hold: four 1080p pairs in flight) otherwise
  for (int np : {16, 32}) {
    const int bpc = resident_blocks_per_cu(np);
    if (bpc < 1) continue;
    const int q = resident_points_per_workgroup(np);
    const int parts = std::max(1, (b->maxpts + q - 1) / q);
    const int64_t capacity = (int64_t)bpc * cu_count();
    const int slots = (int)std::min<int64_t>(std::min<int64_t>(b->B, max_slots), capacity / (parts + 1));
    if (slots < 1) continue;
    if (np == 16 && slots < b->B && !xchg) continue;
    if ((int64_t)((b->B + slots - 1) / slots) * b->op->maxiter >= kXchgMaxSeq) return false;  // exchange number
    p->res = ResidentGeom{parts, slots, np};
    return true;
  }
  return false;
}
// The setup launches of the resident form: their chunk size (the resident launch itself has its own geometry; the
// batch's chunk size serves the per-iteration kernels). (1) At least 16 points per wave chunk (32 from three problems
// on): the setup leaves one H partial per workgroup, and the pair's solver workgroup sums them before the first
// iteration -- 2025 of them with the 4-point chunks a single dense pair gets. One / two / four dense 1080p pairs: 0.42 /
// 0.52 / 0.73 -> 0.38 / 0.45 / 0.59 ms per tracking. (2) 64 at the coarser levels of batches of eight or more -- frames
// that fit the caches: 32 pairs x 32 400 points 339-345 / 265-269 / 240-250 us at levels 0 / 1 / 2 with 32, 364-375 /
// 253-260 / 214-225 with 64 (profiles/r03_notes.md 10, 12). Both as long as the launch keeps about two workgroups per
// CU (16 x 3000 points: 32 would leave 384). A chunk size forced by ICTR_CPW holds for these launches too.
static void resident_setup_plan(const ictr_batch *b, bool forced_cpw, TrackPlan *p) {
  auto blocks_for = [&](int c) {  // workgroups per problem with c points per wave chunk
    const int64_t want = (((int64_t)std::max(b->maxpts, 1) + c - 1) / c + kWaves - 1) / kWaves;
    int g = (int)std::min<int64_t>(std::max<int64_t>(want, 1), std::max(b->gridx8, 1));
    if (g >= 64) g = std::min((g + 7) / 8 * 8, b->gridx8);
    return g;
  };
  const int64_t enough = 2 * (int64_t)cu_count() - 16;
  for (int sl = b->op->lv_l; sl <= b->op->lv_f; ++sl) {
    int cpw_l = b->cpw;
    if (!forced_cpw) {
      for (int c = b->B <= 2 ? 16 : 32; c > cpw_l; c /= 2)
        if ((int64_t)b->B * blocks_for(c) >= enough) {
          cpw_l = c;
          break;
        }
      if (sl > 0 && b->B >= 8 && cpw_l >= 16 && (int64_t)b->B * blocks_for(64) >= enough) cpw_l = 64;
    }
    p->setup_cpw[sl] = cpw_l;
    p->setup_gridx8[sl] = cpw_l != b->cpw ? blocks_for(cpw_l) : b->gridx8;
  }
}

// The launch form of the coming tracking, in this order:
// - the resident-iteration form where resident_plan takes the tracking and the problems have at least 8193 points;
// - the one-launch tracker k_track1 (ictr_track1.hip): the team form where track1_team gives one, else one workgroup
//   per problem for problems whose point records fit its LDS and that are small -- measured (tools/latency.py, r02): one
//   problem costs 0.17 ms + 1.9 us per 8x8 patch in one launch against a flat 0.52 ms of dependent launches ->
//   cross-over near 190 points; a batch of independent problems (run_track_nposes: one workgroup per pose sample, all
//   CUs busy) still wins at 300 points each (64 x 300: 0.87 vs 0.98 ms). Without an explicit ictr_batch_begin the launch
//   also carries the begin phase in its arguments when the records fit them (kFormTrack1Begin), else it projects itself
//   and mirrors the final records (500 pose samples x 60 points: 0.42 -> 0.39 ms per frame pair). Not for sharded batches,
//   not with event timing, not for image-only reference pyramids (only k_ref8 forms the gradient patches on the fly);
//   - the resident-iteration form (batches of mid-size problems);
// - launch-bound sizes (up to 65 536 points in the batch): the per-iteration launches replayed as one hipGraph;
// - the per-iteration launches.
// ICTR_VARIANT_LAUNCHES / ONE_LAUNCH / NO_GRAPH / SEPARATE_BEGIN / NO_TEAMS / NO_RESIDENT move a tracking off its form.
// begun: ictr_batch_begin has run the begin phase already.
static TrackPlan plan_tracking(const ictr_batch *b, bool begun) {
  TrackPlan p;
  memset(&p, 0, sizeof(p));
  const int v = engine_variant(b);
  p.variant = v;
  p.team = 1;
  p.mute = (v & ICTR_VARIANT_DEBUG_MUTE) ? 1 : 0;
  const bool resident = !(v & (ICTR_VARIANT_NO_RESIDENT | ICTR_VARIANT_LAUNCHES | ICTR_VARIANT_ANY_SIZE)) &&
                        resident_plan(b, &p);
  bool t1 = !b->sharded && !b->timing && !(v & ICTR_VARIANT_LAUNCHES) && b->xchg.world <= 1 && b->otf != 2 &&
            !(b->maxpts < 8193 && resident) && b->maxpts >= 1;
  if (t1) {
    int q = 0;
    const int team = (v & ICTR_VARIANT_NO_TEAMS) ? 1 : track1_team(b, &q);
    if (team > 1) {
      p.team = team;
      p.team_q = q;
    } else if ((size_t)b->maxpts * 64 > 128 * 1024) {  // point records must fit in LDS
      t1 = false;
    } else if (!(v & ICTR_VARIANT_ONE_LAUNCH)) {
      const int limit = b->B >= 16 ? 384 : 192;
      t1 = (int64_t)b->maxpts * b->n <= (int64_t)limit * 64;
    }
  }
  if (t1) {
    p.res = ResidentGeom{0, 0, 0};
    const bool separate = begun || b->trace_on || !b->d_st_mirror || (v & ICTR_VARIANT_SEPARATE_BEGIN);
    const size_t up = sizeof(ProbState) * b->B + sizeof(PlaneSet) * b->h_planes.size();
    p.form = (!separate && up <= track1_blob_bytes()) ? kFormTrack1Begin : kFormTrack1;
    p.project_here = p.form == kFormTrack1 && !separate;
  } else if (resident) {
    p.form = kFormResident;
    resident_setup_plan(b, cpw_forced() != 0, &p);
  } else if (!b->sharded && !b->timing && !b->graph_broken && !(v & ICTR_VARIANT_NO_GRAPH) &&
             (int64_t)b->maxpts * b->B <= 65536) {
    p.form = kFormGraph;
  } else {
    p.form = kFormLaunches;
  }
  return p;
}

// Admission of team launches. A team's workgroups wait for each other inside the kernel, so they must all become
// resident. One launch alone is safe whatever its size (in-order dispatch: the lowest unfinished team always gets its
// CUs). Several team launches on different streams are dispatched interleaved, each with at most ONE partly resident
// team at its dispatch front; if those fronts could fill every CU, nobody would ever be complete. So the launches in
// flight (process-wide, any batch, any stream) are kept to sum(team - 1) < CUs: a launch that would exceed it first
// makes its stream wait (hipStreamWaitEvent, the host does not block) for the oldest team launches still in flight.
// With teams of at most 64 workgroups and 256 CUs that is four concurrent launches of the largest team, more of smaller.
struct TeamFlight {
  hipEvent_t ev;
  int weight;  // quarter-CU slots, see team_launch
};
struct TeamDevice {  // per device: launches in flight (oldest first), recycled events
  std::deque<TeamFlight> flights;
  std::vector<hipEvent_t> events;
};
static std::mutex g_team_mu;
static std::map<int, TeamDevice> g_team_dev;
// Admit + launch + record as ONE critical section (two host threads driving two engines must not both pass the budget
// test before either launch is visible): make `s` wait until the launch fits beside the launches in flight on this
// device, run `launch` (which enqueues the kernel on `s`), record an event behind it and enter it in the flight list.
// weight, in quarter-CU slots (four workgroups of the resident-iteration kernel share a CU): a team launch
// 4 (team - 1) -- its partly resident dispatch front, a whole CU per workgroup --, a resident-iteration launch one per
// workgroup x (4 / workgroups per CU, rounded up): ALL of them must be resident. Budget 4 CUs - 4: sum(team - 1) < CUs
// as before; a resident launch that fills every slot but four fits alone.
template <class F>
static int team_launch(int weight, hipStream_t s, F &&launch) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    (void)hipGetLastError();
    dev = 0;
  }
  const int budget = 4 * cu_count() - 4;
  std::lock_guard<std::mutex> lk(g_team_mu);
  TeamDevice &d = g_team_dev[dev];
  while (!d.flights.empty() && hipEventQuery(d.flights.front().ev) == hipSuccess) {  // retire finished ones
    d.events.push_back(d.flights.front().ev);
    d.flights.pop_front();
  }
  (void)hipGetLastError();  // hipEventQuery's "not ready" is not an error
  int load = 0;
  for (const TeamFlight &f : d.flights) load += f.weight;
  for (size_t i = 0; i < d.flights.size() && load + weight > budget; ++i) {
    HIPCHK(hipStreamWaitEvent(s, d.flights[i].ev, 0));  // this launch starts behind flight i
    load -= d.flights[i].weight;
  }
  hipEvent_t ev = nullptr;
  if (!d.events.empty()) {
    ev = d.events.back();
    d.events.pop_back();
  } else {
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  }
  const int rc = launch();
  hipError_t er = rc == ICTR_OK ? hipEventRecord(ev, s) : hipSuccess;
  if (rc != ICTR_OK || er != hipSuccess) {
    d.events.push_back(ev);  // nothing is in flight behind this event: keep it for the next launch
    if (rc != ICTR_OK) return rc;
    return fail(ICTR_ERR_HIP, "team_launch: hipEventRecord failed: %s", hipGetErrorString(er));
  }
  d.flights.push_back(TeamFlight{ev, weight});
  return ICTR_OK;
}

// bound of an in-launch poll (team form, resident-iteration form), seconds. Read at every launch: tests shorten it
static double team_timeout_s() {
  const char *s = getenv("ICTR_TEAM_TIMEOUT_S");
  return s ? std::max(0.001, atof(s)) : 5.0;
}
// Mailbox, tag epoch, polling limit and error flag of the next launch with an in-launch exchange (team form of k_track1,
// k_level_resident) that will run on `s` and needs `granules` granules of mailbox `m`: the host side of ictr_xchg.h's
// protocol, whole. The mailbox is cleared on the stream of the launch. what: the mailbox's name in the error text.
static int exchange_prepare(ictr_batch *b, Mailbox *m, size_t granules, const char *what, int mute, hipStream_t s,
                            Exchange *x) {
  const size_t need = sizeof(unsigned long long) * granules;
  if (need > m->bytes) {
    if (m->d) HIPCHK(hipStreamSynchronize(s));  // an earlier launch may still be polling the old mailbox
    m->d.reset();
    m->bytes = 0;
    // granules are written and polled with agent-scope accesses; uncached device memory keeps them out of the L2s
    unsigned long long *uncached = nullptr;
    if (hipExtMallocWithFlags((void **)&uncached, need, hipDeviceMallocUncached) == hipSuccess) {
      m->d.adopt(uncached);
    } else {
      (void)hipGetLastError();
      if (m->d.alloc(need)) return fail(ICTR_ERR_HIP, "%s mailbox allocation failed (%zu bytes)", what, need);
    }
    HIPCHK(hipMemsetAsync(m->d.get(), 0, need, s));
    m->bytes = need;
    m->epoch = 0;
  }
  if (!b->h_team_err) {  // the pinned sticky time-out flag, shared by every exchange of the batch
    if (int rc = b->h_team_err.alloc(sizeof(int))) return rc;
    *b->h_team_err.get() = 0;
    HIPCHK(hipHostGetDevicePointer((void **)&b->d_team_err, b->h_team_err.get(), 0));
  }
  const XchgEpoch next = xchg_next_epoch(m->epoch);
  if (next.clear) HIPCHK(hipMemsetAsync(m->d.get(), 0, m->bytes, s));
  m->epoch = next.epoch;
  x->tag0 = xchg_tag0(m->epoch);
  x->limit = (unsigned long long)(team_timeout_s() * kWallClockHz);
  x->mail = m->d.get();
  x->err = b->d_team_err;
  x->mute = mute;
  return ICTR_OK;
}
// the team of the next k_track1 launch with its exchange (p.team == 1: not a team launch, nothing allocated)
static int team_prepare(ictr_batch *b, const TrackPlan &p, T1Team *tm) {
  memset(tm, 0, sizeof(*tm));
  tm->team = 1;
  if (p.team < 2) return ICTR_OK;
  tm->team = p.team;
  tm->q = p.team_q;
  return exchange_prepare(b, &b->team_mail, team_mail_granules(b->B, p.team), "team", p.mute, b->stream, &tm->x);
}
// ONE k_track1 launch for every problem of `e` on the batch's stream, through the team admission when the plan has
// teams. blob: the begin phase in the arguments (kFormTrack1Begin); host_st: the pinned mirror the launch writes the final
// records to; project_here: the launch projects (step 3) itself
static int track1_launch(ictr_batch *b, const EngineDev &e, const TrackPlan &p, const void *blob, ProbState *host_st,
                         bool project_here) {
  LevelCam cams[16];
  for (int l = 0; l < b->nlev; ++l) cams[l] = level_cam(b->cam, l);
  T1Team tm;
  if (int rc = team_prepare(b, p, &tm)) return rc;
  auto launch = [&]() -> int {
    HIPCHK(launch_track1(e, cams, b->maxpts, kTrack1Waves, blob, host_st, b->stream, tm.team > 1 ? &tm : nullptr,
                         project_here, (p.variant & ICTR_VARIANT_ANY_SIZE) != 0));
    return ICTR_OK;
  };
  if (tm.team > 1) return team_launch(4 * (tm.team - 1), b->stream, launch);
  return launch();
}

// one level's iterations as ONE resident launch (behind the level's setup launches on the same stream)
static int launch_resident(ictr_batch *b, const EngineDev &e, const LevelCam &lc, const LevelLaunch &ll,
                           const TrackPlan &p, hipStream_t s) {
  const ResidentGeom &g = p.res;
  Exchange x;
  if (int rc = exchange_prepare(b, &b->res_mail, res_mail_granules(g.parts, g.slots), "resident", p.mute, s, &x)) return rc;
  // every workgroup of the launch must be resident: it starts when its slots are free of team / resident launches
  const int bpc = std::max(1, std::min(4, resident_blocks_per_cu(g.np)));
  const int weight = g.slots * (g.parts + 1) * ((4 + bpc - 1) / bpc);
  return team_launch(weight, s, [&]() -> int {
    HIPCHK(launch_level_resident(e, lc, ll.level, g, tail_partials(e, ll), x, b->xchg.world > 1 ? &b->xchg : nullptr, s));
    return ICTR_OK;
  });
}

// the per-level launches of the plan's form (kFormLaunches / kFormGraph: the split launchers of ictr_kernels.hip --
// accumulate kernel and tail kernel separately, so that events can bracket the accumulate kernel alone; kFormResident:
// the setup launch, then ONE launch for all iterations of the level)
static int enqueue_level_kernels(ictr_batch *b, const EngineDev &e, const TrackPlan &p, hipStream_t s, bool events) {
  const int mi = b->op->maxiter;
  const bool resident = p.form == kFormResident;
  const bool tk = !resident && events && (int)b->evk.size() >= 2 * b->nlev * mi && mi <= b->evk_iters;
  b->evk_valid = tk;  // (resident: no per-iteration launches, the kernel-time getters report zeros)
  for (int sl = b->op->lv_f; sl >= b->op->lv_l; --sl) {
    const LevelCam lc = level_cam(b->cam, sl);
    if (events) HIPCHK(hipEventRecord(b->ev[3 * sl + 0].get(), s));
    const LevelLaunch ll = level_launch(b, &p, sl);
    launch_ref_level(e, lc, ll, !resident, s);
    if (events) HIPCHK(hipEventRecord(b->ev[3 * sl + 1].get(), s));
    if (resident) {
      if (int rc = launch_resident(b, e, lc, ll, p, s)) return rc;
    } else {
      for (int it = 0; it < mi; ++it) {
        const int ke = 2 * (sl * b->evk_iters + it);
        launch_iter_main(e, lc, ll, it == 0, s, tk ? b->evk[ke].get() : nullptr, tk ? b->evk[ke + 1].get() : nullptr);
        launch_iter_tail(e, ll, it == 0, s);
      }
    }
    if (events) {
      HIPCHK(hipEventRecord(b->ev[3 * sl + 2].get(), s));
      b->ev_used[sl] = 1;
    }
  }
  return ICTR_OK;
}

// Launch-bound sizes (a few hundred to a few thousand points: every kernel of the per-iteration form runs 2-5 us)
// replay the whole launch sequence of a tracking -- (setup + tail) per level, (accumulate + tail) per iteration, 111
// kernels for 5 levels x 10 iterations -- as ONE instantiated hipGraph: the host pays one graph launch instead of 111
// kernel launches and the GPU finds the next packet already queued. The graph is captured once per batch and reused for
// as long as nothing the launches depend on changes. Kernel arguments are passed by value, so the key is all of them:
// the engine's device view byte for byte (engine_dev zero-fills it; it has no padding), the plan, the cameras and the
// grid shapes -- a field added to EngineDev is covered by construction.
template <class T>
static void key_put(std::string &k, const T &v) { k.append(reinterpret_cast<const char *>(&v), sizeof(T)); }
static std::string graph_key(const ictr_batch *b, const EngineDev &e, const TrackPlan &p) {
  static_assert(sizeof(EngineDev) == 14 * 4 + 14 * 8 + 2 * 4, "EngineDev must have no padding (graph_key)");
  static_assert(sizeof(TrackPlan) % 4 == 0 && sizeof(LevelCam) == 7 * 4, "plain ints and floats only");
  std::string k;
  key_put(k, e);
  key_put(k, p);
  for (int l = 0; l < b->nlev; ++l) key_put(k, level_cam(b->cam, l));
  for (int v : {b->cpw, b->gridx, b->gridx8}) key_put(k, v);
  return k;
}
// (re)build the graph of the current tracking's launches; false: fall back to plain launches for good
static bool build_graph(ictr_batch *b, const EngineDev &e, const TrackPlan &p, const std::string &key) {
  if (b->gexec) {
    (void)hipGraphExecDestroy(b->gexec);
    b->gexec = nullptr;
  }
  b->gkey.clear();
  if (!b->cap_stream && hipStreamCreateWithFlags(&b->cap_stream, hipStreamNonBlocking) != hipSuccess) return false;
  if (hipStreamBeginCapture(b->cap_stream, hipStreamCaptureModeThreadLocal) != hipSuccess) return false;
  const int rc = enqueue_level_kernels(b, e, p, b->cap_stream, false);
  hipGraph_t g = nullptr;
  const hipError_t ec = hipStreamEndCapture(b->cap_stream, &g);
  bool ok = rc == ICTR_OK && ec == hipSuccess && g != nullptr;
  if (ok) ok = hipGraphInstantiate(&b->gexec, g, nullptr, nullptr, 0) == hipSuccess;
  if (g) (void)hipGraphDestroy(g);
  if (!ok) {
    (void)hipGetLastError();  // clear the sticky error of the failed capture
    b->gexec = nullptr;
    return false;
  }
  b->gkey = key;
  return true;
}

// the launches of b->plan (any form but kFormTrack1Begin)
static int enqueue_levels(ictr_batch *b) {
  const EngineDev e = engine_dev(b);
  TrackPlan &p = b->plan;
  if (b->xchg.world > 1 && p.form != kFormResident)
    return fail(ICTR_ERR_STATE, "a peer exchange is set (sharded resident form) but this tracking cannot run in the "
                                "resident-iteration form (8x8 patches, no robustness option, no patch normalisation, builder-"
                                "made pyramids, at most %d pair-rounds x iterations per level)", kXchgMaxSeq);
  if (p.form == kFormTrack1)
    return track1_launch(b, e, p, nullptr, p.project_here ? b->d_st_mirror : nullptr, p.project_here != 0);
  if (p.form == kFormGraph) {
    const std::string key = graph_key(b, e, p);
    if ((b->gexec && key == b->gkey) || build_graph(b, e, p, key)) {
      HIPCHK(hipGraphLaunch(b->gexec, b->stream));
      return ICTR_OK;
    }
    b->graph_broken = true;
    p.form = kFormLaunches;
  }
  if (b->timing) std::fill(b->ev_used.begin(), b->ev_used.end(), 0);
  if (int rc = enqueue_level_kernels(b, e, p, b->stream, b->timing)) return rc;
  HIPCHK(hipGetLastError());
  return ICTR_OK;
}

// One tracking of every problem, enqueued on the stream up to and including the final states' way into the pinned host
// mirror and the event that marks them. When SetPose has not been followed by an explicit begin and the plan is
// kFormTrack1Begin, the batch goes out as ONE launch that also carries ictr_batch_begin's device part in its arguments
// (T1Args in ictr_track1.hip) and writes the final states to the mirror itself: no upload copies, no fill, no projection
// launch, no read-back copy. With project_here the records are uploaded and the launch projects and mirrors itself.
static int track_enqueue(ictr_batch *b) {
  if (b->h_team_err && *(volatile int *)b->h_team_err.get()) {
    // the previous tracking of this batch ran into an exchange time-out (reported by its wait): let whatever it left on
    // the stream finish, then start clean -- mailbox tags carry the launch epoch, nothing of the failed launch survives
    HIPCHK(hipStreamSynchronize(b->stream));
    *(volatile int *)b->h_team_err.get() = 0;
  }
  const bool begun = b->projected;
  if (!begun)
    if (int rc = begin_prepare(b)) return rc;
  b->plan = plan_tracking(b, begun);
  const TrackPlan &p = b->plan;
  if (!begun) {
    if (p.form != kFormTrack1Begin)
      if (int rc = begin_device(b, !p.project_here)) return rc;
    b->projected = true;
  }
  bool mirrored = false;
  if (p.form == kFormTrack1Begin) {
    const size_t nst = sizeof(ProbState) * b->B, npl = sizeof(PlaneSet) * b->h_planes.size();
    unsigned char blob[4096];
    memcpy(blob, b->h_st.data(), nst);
    memcpy(blob + nst, b->h_planes.data(), npl);
    if (int rc = track1_launch(b, engine_dev(b), p, blob, b->d_st_mirror, false)) return rc;
    mirrored = true;
  } else {
    if (int rc = enqueue_levels(b)) return rc;
    mirrored = p.project_here != 0;
  }
  if (!mirrored)
    HIPCHK(hipMemcpyAsync(b->h_st_pin.get(), b->d_st.get(), sizeof(ProbState) * b->B, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipEventRecord(b->done_ev.get(), b->stream));
  b->done_valid = true;
  return ICTR_OK;
}

extern "C" int ictr_batch_track_async(ictr_batch *b) {
  if (!b) return fail(ICTR_ERR_INVALID, "batch is NULL");
  if (b->sharded) return fail(ICTR_ERR_STATE, "sharded batches are driven phase by phase (see ictr.h)");
  b->projected = false;  // a batch tracking always starts from the poses of the last SetPose calls
  return track_enqueue(b);
}
// an in-launch exchange of the last tracking timed out (team form of the one-launch tracker, resident-iteration form):
// its results are invalid. The flag stays set until the next tracking is enqueued (track_enqueue).
static int team_error_check(const ictr_batch *b) {
  if (b->h_team_err && *(volatile int *)b->h_team_err.get())
    return fail(ICTR_ERR_HIP, "%s: a workgroup waited in vain for its peers' partial sums (in-launch exchange timed out "
                              "after %.3f s; are all workgroups of the launch resident?); the results of this tracking "
                              "are invalid",
                b->plan.form == kFormResident ? "resident-iteration form (k_level_resident)" : "one-launch tracker, team form (k_track1_p8)",
                team_timeout_s());
  return ICTR_OK;
}
// wait for the engine's last tracking (not for whatever else was enqueued on the stream after it)
static int batch_wait(ictr_batch *b) {
  if (b->done_valid)
    HIPCHK(hipEventSynchronize(b->done_ev.get()));
  else
    HIPCHK(hipStreamSynchronize(b->stream));
  return team_error_check(b);
}

extern "C" int ictr_batch_set_timing(ictr_batch *b, int enable) {
  if (!b) return fail(ICTR_ERR_INVALID, "batch is NULL");
  if (enable && b->ev.empty()) {  // all events or none: a failure half way leaves the batch without timing
    const int iters = std::max(1, b->op->maxiter);
    std::vector<Event> ev(3 * b->nlev), evk((size_t)2 * b->nlev * iters);
    for (Event &e : ev)
      if (int rc = e.create()) return rc;
    for (Event &e : evk)
      if (int rc = e.create()) return rc;
    b->ev = std::move(ev);
    b->evk = std::move(evk);
    b->ev_used.assign(b->nlev, 0);
    b->evk_iters = iters;
  }
  b->timing = enable != 0;
  return ICTR_OK;
}
extern "C" int ictr_batch_get_level_times(ictr_batch *b, float *ms_setup, float *ms_iters) {
  if (!b || !ms_setup || !ms_iters) return fail(ICTR_ERR_INVALID, "get_level_times: NULL argument");
  if (b->ev.empty()) return fail(ICTR_ERR_STATE, "timing was never enabled");
  if (int rc = batch_wait(b)) return rc;
  for (int l = 0; l < b->nlev; ++l) {
    ms_setup[l] = ms_iters[l] = 0.0f;
    if (b->ev_used[l] != 1) continue;
    HIPCHK(hipEventElapsedTime(&ms_setup[l], b->ev[3 * l + 0].get(), b->ev[3 * l + 1].get()));
    HIPCHK(hipEventElapsedTime(&ms_iters[l], b->ev[3 * l + 1].get(), b->ev[3 * l + 2].get()));
  }
  return ICTR_OK;
}
extern "C" int ictr_batch_get_kernel_times(ictr_batch *b, float *ms_kernel) {
  if (!b || !ms_kernel) return fail(ICTR_ERR_INVALID, "get_kernel_times: NULL argument");
  if (b->evk.empty()) return fail(ICTR_ERR_STATE, "timing was never enabled");
  if (int rc = batch_wait(b)) return rc;
  const int mi = std::min(b->op->maxiter, b->evk_iters);
  for (int l = 0; l < b->nlev; ++l) {
    ms_kernel[l] = 0.0f;
    if (!b->ev_used[l] || !b->evk_valid) continue;
    for (int it = 0; it < mi; ++it) {
      float ms = 0.0f;
      const int ke = 2 * (l * b->evk_iters + it);
      HIPCHK(hipEventElapsedTime(&ms, b->evk[ke].get(), b->evk[ke + 1].get()));
      ms_kernel[l] += ms;
    }
  }
  return ICTR_OK;
}
// the first accumulate launch of each level alone (on the 8x8 fast path it is a different kernel instantiation: it
// also accumulates the 21 H sums), so that callers can report the regular iteration kernel separately
extern "C" int ictr_batch_get_first_iter_times(ictr_batch *b, float *ms_first) {
  if (!b || !ms_first) return fail(ICTR_ERR_INVALID, "get_first_iter_times: NULL argument");
  if (b->evk.empty()) return fail(ICTR_ERR_STATE, "timing was never enabled");
  if (int rc = batch_wait(b)) return rc;
  for (int l = 0; l < b->nlev; ++l) {
    ms_first[l] = 0.0f;
    if (!b->ev_used[l] || !b->evk_valid || b->op->maxiter < 1) continue;
    HIPCHK(hipEventElapsedTime(&ms_first[l], b->evk[2 * (l * b->evk_iters)].get(), b->evk[2 * (l * b->evk_iters) + 1].get()));
  }
  return ICTR_OK;
}
// Absolute launch intervals (for callers that run several engines concurrently on different streams and need to know
// which launches overlapped): ms since the process-wide time base set by ictr_timebase_mark().
static hipEvent_t g_timebase = nullptr;
extern "C" int ictr_timebase_mark(void) {
  if (int rc = need_device()) return rc;
  if (!g_timebase) HIPCHK(hipEventCreate(&g_timebase));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipEventRecord(g_timebase, nullptr));
  HIPCHK(hipEventSynchronize(g_timebase));
  return ICTR_OK;
}
extern "C" int ictr_batch_get_kernel_intervals(ictr_batch *b, float *start_ms, float *end_ms) {
  if (!b || !start_ms || !end_ms) return fail(ICTR_ERR_INVALID, "get_kernel_intervals: NULL argument");
  if (b->evk.empty()) return fail(ICTR_ERR_STATE, "timing was never enabled");
  if (!g_timebase) return fail(ICTR_ERR_STATE, "ictr_timebase_mark has not been called");
  if (int rc = batch_wait(b)) return rc;
  const int mi = std::min(b->op->maxiter, b->evk_iters);
  for (int l = 0; l < b->nlev; ++l)
    for (int it = 0; it < b->evk_iters; ++it) {
      const int k = l * b->evk_iters + it;
      start_ms[k] = end_ms[k] = 0.0f;
      if (!b->ev_used[l] || !b->evk_valid || it >= mi) continue;
      HIPCHK(hipEventElapsedTime(&start_ms[k], g_timebase, b->evk[2 * k].get()));
      HIPCHK(hipEventElapsedTime(&end_ms[k], g_timebase, b->evk[2 * k + 1].get()));
    }
  return ICTR_OK;
}
// the same for the per-level setup launches (k_ref* + k_level_tail): [level]
extern "C" int ictr_batch_get_setup_intervals(ictr_batch *b, float *start_ms, float *end_ms) {
  if (!b || !start_ms || !end_ms) return fail(ICTR_ERR_INVALID, "get_setup_intervals: NULL argument");
  if (b->ev.empty()) return fail(ICTR_ERR_STATE, "timing was never enabled");
  if (!g_timebase) return fail(ICTR_ERR_STATE, "ictr_timebase_mark has not been called");
  if (int rc = batch_wait(b)) return rc;
  for (int l = 0; l < b->nlev; ++l) {
    start_ms[l] = end_ms[l] = 0.0f;
    if (b->ev_used[l] != 1) continue;
    HIPCHK(hipEventElapsedTime(&start_ms[l], g_timebase, b->ev[3 * l + 0].get()));
    HIPCHK(hipEventElapsedTime(&end_ms[l], g_timebase, b->ev[3 * l + 1].get()));
  }
  return ICTR_OK;
}
extern "C" int ictr_batch_last_path(const ictr_batch *b) { return b ? b->plan.form : -1; }
extern "C" int ictr_batch_last_team(const ictr_batch *b) {
  return b ? ((b->plan.form == kFormTrack1 || b->plan.form == kFormTrack1Begin) ? b->plan.team : 1) : -1;
}
extern "C" int ictr_batch_set_reduction_buffer(ictr_batch *b, float *dev_ptr) {
  if (!b) return fail(ICTR_ERR_INVALID, "batch is NULL");
  b->d_red = dev_ptr ? dev_ptr : b->d_red_own.get();
  return ICTR_OK;
}

static int batch_fetch_state(ictr_batch *b) {
  if (b->done_valid) {
    HIPCHK(hipEventSynchronize(b->done_ev.get()));
    memcpy(b->h_st.data(), b->h_st_pin.get(), sizeof(ProbState) * b->B);
  } else {
    HIPCHK(hipMemcpyAsync(b->h_st.data(), b->d_st.get(), sizeof(ProbState) * b->B, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
  }
  if (int rc = team_error_check(b)) return rc;  // never hand out the poses of a tracking whose exchanges timed out
  for (int i = 0; i < b->B; ++i) {
    memcpy(b->probs[i].p, b->h_st[i].p, sizeof(float) * 6);
    memcpy(b->probs[i].G, b->h_st[i].G, sizeof(float) * 12);
    b->probs[i].iters = b->h_st[i].total_iters;
  }
  return ICTR_OK;
}
extern "C" int ictr_batch_get_poses(ictr_batch *b, double *p_out) {
  if (!b || !p_out) return fail(ICTR_ERR_INVALID, "get_poses: NULL argument");
  if (int rc = batch_fetch_state(b)) return rc;
  for (int i = 0; i < b->B; ++i) {
    const ProbHost &ph = b->probs[i];
    host_getpose(b->op->donorm, ph.p, ph.G, ph.meanshift, ph.varval, p_out + 6 * i);
  }
  return ICTR_OK;
}
extern "C" int ictr_batch_get_iterations(ictr_batch *b, int *iters) {
  if (!b || !iters) return fail(ICTR_ERR_INVALID, "get_iterations: NULL argument");
  for (int i = 0; i < b->B; ++i) iters[i] = b->probs[i].iters;
  return ICTR_OK;
}
extern "C" int ictr_batch_get2dpoints(ictr_batch *b, int64_t problem, float *host_out) {
  if (!b || problem < 0 || problem >= b->B || !host_out) return fail(ICTR_ERR_INVALID, "get2dpoints: bad arguments");
  if (!b->projected)
    if (int rc = ictr_batch_begin(b)) return rc;
  const size_t M = b->M;
  HIPCHK(hipMemcpyAsync(host_out, b->d_pt2d.get() + ((size_t)problem * b->nlev + b->op->lv_l) * 2 * M, sizeof(float) * 2 * M,
                        hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return ICTR_OK;
}

// ---------------------------------------------------------------- OdometerClass = batch of one + a PoseClass
struct ictr_odometer {
  ictr_batch *b = nullptr;
  ictr_pose *pose = nullptr;
  ictr_pyramid *own_ref = nullptr, *own_new = nullptr;  // uploads made by setpose_host
  ~ictr_odometer() {
    delete own_ref;
    delete own_new;
    delete b;
  }
};

extern "C" int ictr_odometer_create(ictr_odometer **out, ictr_pose *pose, const ictr_optparam *op) {
  if (!out || !pose || !op) return fail(ICTR_ERR_INVALID, "odometer_create: NULL argument");
  ictr_batch *b = nullptr;
  if (int rc = ictr_batch_create(&b, pose->cam, op, 1)) return rc;
  ictr_odometer *o = new ictr_odometer;
  o->b = b;
  o->pose = pose;
  *out = o;
  return ICTR_OK;
}
extern "C" void ictr_odometer_destroy(ictr_odometer *o) { delete o; }
extern "C" int ictr_odometer_set_stream(ictr_odometer *o, void *s) {
  if (!o) return fail(ICTR_ERR_INVALID, "odometer is NULL");
  return ictr_batch_set_stream(o->b, s);
}
extern "C" int ictr_odometer_set_robust(ictr_odometer *o, int flags, float huber_k) {
  if (!o) return fail(ICTR_ERR_INVALID, "odometer is NULL");
  return ictr_batch_set_robust(o->b, flags, huber_k);
}
extern "C" int ictr_odometer_set_team(ictr_odometer *o, int target_points, int min_points, int max_points) {
  if (!o) return fail(ICTR_ERR_INVALID, "odometer is NULL");
  return ictr_batch_set_team(o->b, target_points, min_points, max_points);
}
extern "C" int ictr_odometer_set_variant(ictr_odometer *o, int v) {
  if (!o) return fail(ICTR_ERR_INVALID, "odometer is NULL");
  return ictr_batch_set_variant(o->b, v);  // (refuses unknown bits)
}
extern "C" int ictr_odometer_last_path(const ictr_odometer *o) { return o ? ictr_batch_last_path(o->b) : -1; }
extern "C" int ictr_odometer_last_team(const ictr_odometer *o) { return o ? ictr_batch_last_team(o->b) : -1; }
extern "C" int ictr_odometer_set3dpoints(ictr_odometer *o, double *pt_in, int64_t nopoints_in) {
  if (!o) return fail(ICTR_ERR_INVALID, "odometer is NULL");
  return ictr_batch_set3dpoints(o->b, 0, pt_in, nopoints_in);
}
extern "C" int ictr_odometer_setpose(ictr_odometer *o, const double *p_in, const ictr_pyramid *pyr_ref,
                                     const ictr_pyramid *pyr_new) {
  if (!o) return fail(ICTR_ERR_INVALID, "odometer is NULL");
  if (int rc = ictr_batch_setpose(o->b, 0, p_in, pyr_ref, pyr_new)) return rc;
  // PoseClass state follows (pose.cpp:25-76 is invoked through the odometer in the reference)
  ProbHost &ph = o->b->probs[0];
  memcpy(o->pose->meanshift, ph.meanshift, sizeof(ph.meanshift));
  o->pose->varval = ph.varval;
  memcpy(o->pose->p, ph.p, sizeof(ph.p));
  memcpy(o->pose->G, ph.G, sizeof(ph.G));
  // Step 3 (the projections) is deferred to whoever needs it first: Get2DPoints right after SetPose runs it on its own
  // (ictr_batch_get2dpoints), TrackPose folds it into its launch (track_enqueue). Argument errors surface here.
  return begin_prepare(o->b);
}
extern "C" int ictr_odometer_setpose_host(ictr_odometer *o, const double *p_in, const float **img_ref,
                                          const float **img_ref_dx, const float **img_ref_dy, const float **img_new) {
  if (!o || !img_ref || !img_ref_dx || !img_ref_dy || !img_new)
    return fail(ICTR_ERR_INVALID, "setpose_host: NULL argument");
  const ictr_cam *c = o->b->cam;
  delete o->own_ref;
  delete o->own_new;
  o->own_ref = o->own_new = nullptr;
  if (int rc = ictr_pyramid_create_from_host_planes(&o->own_ref, img_ref, img_ref_dx, img_ref_dy, c->wh[0], c->wh[1],
                                                    o->b->op->lv_f, c->padding))
    return rc;
  if (int rc = ictr_pyramid_create_from_host_planes(&o->own_new, img_new, nullptr, nullptr, c->wh[0], c->wh[1],
                                                    o->b->op->lv_f, c->padding))
    return rc;
  return ictr_odometer_setpose(o, p_in, o->own_ref, o->own_new);
}
extern "C" int ictr_odometer_trackpose(ictr_odometer *o, double *p_out) {
  if (!o || !p_out) return fail(ICTR_ERR_INVALID, "trackpose: NULL argument");
  ictr_batch *b = o->b;
  if (!b->probs[0].pose_set) return fail(ICTR_ERR_STATE, "TrackPose before SetPose");
  // verbosity == 2: the reference prints |delta_p|_1 after every iteration (odometer.cpp:416-417); the device
  // records every iteration (trace), printed below in the reference's format
  const bool verbose = b->op->verbosity == 2, trace_was_on = b->trace_on;
  if (verbose && !trace_was_on) {
    b->trace_on = true;
    if (b->projected) HIPCHK(hipMemsetAsync(b->d_trace_count.get(), 0, sizeof(int), b->stream));  // else: the begin phase
  }
  int rc_enq = track_enqueue(b);
  b->trace_on = trace_was_on;
  if (rc_enq) return rc_enq;
  // like the reference, a second TrackPose without SetPose continues from the current pose with the old
  // reference projections (device state persists)
  if (int rc = batch_fetch_state(b)) return rc;
  if (verbose) {
    int c = 0;
    HIPCHK(hipMemcpy(&c, b->d_trace_count.get(), sizeof(int), hipMemcpyDeviceToHost));
    c = std::min(c, b->trace_cap);
    std::vector<ictr_trace_rec> recs((size_t)std::max(c, 0));
    if (c > 0) HIPCHK(hipMemcpy(recs.data(), b->d_trace.get(), sizeof(ictr_trace_rec) * c, hipMemcpyDeviceToHost));
    for (const ictr_trace_rec &r : recs) {
      const float *d = r.dp;  // delta_p.lpNorm<1>() in Eigen's redux order, as on the device
      const float nd = (fabsf(d[0]) + (fabsf(d[1]) + fabsf(d[2]))) + (fabsf(d[3]) + (fabsf(d[4]) + fabsf(d[5])));
      printf("Sc%02i,It%02i: %g\n", r.level, r.iter, nd);
    }
    fflush(stdout);
  }
  memcpy(o->pose->p, b->probs[0].p, sizeof(float) * 6);
  memcpy(o->pose->G, b->probs[0].G, sizeof(float) * 12);
  return ictr_pose_getpose_se3(o->pose, p_out);
}
extern "C" const float *ictr_odometer_get2dpoints(ictr_odometer *o) {
  if (!o) return nullptr;
  if (ictr_batch_get2dpoints(o->b, 0, o->b->h_pt2d.data()) != ICTR_OK) return nullptr;
  return o->b->h_pt2d.data();
}
extern "C" int ictr_odometer_enable_trace(ictr_odometer *o, int enable) {
  if (!o) return fail(ICTR_ERR_INVALID, "odometer is NULL");
  o->b->trace_on = enable != 0;
  return ICTR_OK;
}
extern "C" int ictr_odometer_trace(ictr_odometer *o, ictr_trace_rec *out, int64_t capacity, int64_t *count) {
  if (!o || !count) return fail(ICTR_ERR_INVALID, "trace: NULL argument");
  int c = 0;
  HIPCHK(hipMemcpy(&c, o->b->d_trace_count.get(), sizeof(int), hipMemcpyDeviceToHost));
  c = std::min(c, o->b->trace_cap);
  *count = c;
  const int64_t ncopy = std::min<int64_t>(c, capacity);
  if (out && ncopy > 0) HIPCHK(hipMemcpy(out, o->b->d_trace.get(), sizeof(ictr_trace_rec) * ncopy, hipMemcpyDeviceToHost));
  return ICTR_OK;
}
// which: 0 T, 1 Gx, 2 Gy (novals*M), 4 pt3d, 5 pt3d_ref (3*M), 7 sd coefficients (16*M), 8 ProbState as floats,
// 100+l: pt2d of level l (2*M)
extern "C" int ictr_batch_read_buffer(ictr_batch *b, int64_t problem, int which, float *host_out, int64_t count) {
  if (!b || !host_out || count < 0 || problem < 0 || problem >= b->B)
    return fail(ICTR_ERR_INVALID, "read_buffer: bad arguments");
  const size_t M = b->M, n = b->n, pr = (size_t)problem;
  const float *src = nullptr;
  size_t avail = 0;
  switch (which) {
    case 0: src = b->d_T.get() + pr * M * n; avail = M * n; break;
    case 1: src = b->d_Gx.get() + pr * M * n; avail = M * n; break;
    case 2: src = b->d_Gy.get() + pr * M * n; avail = M * n; break;
    case 4: src = b->d_pt3d.get() + pr * 3 * M; avail = 3 * M; break;
    case 5: src = b->d_pt3d_ref.get() + pr * 3 * M; avail = 3 * M; break;
    case 7: src = b->d_coef.get() + pr * M * kCoefStride; avail = M * kCoefStride; break;
    case 8: src = reinterpret_cast<const float *>(b->d_st.get() + pr); avail = sizeof(ProbState) / sizeof(float); break;
    case 9: src = b->d_partH.get() + pr * 8; avail = pr == 0 ? 16 : 8; break;  // k_track1 phase cycle counters (ICTR_T1_PROF builds only)
    case 10: src = b->d_partH.get() + (size_t)b->B * 8 + pr * 4; avail = 4; break;  // ... and the solver's
    default:
      if (which >= 100 && which < 100 + b->nlev) {
        src = b->d_pt2d.get() + (pr * b->nlev + (size_t)(which - 100)) * 2 * M;
        avail = 2 * M;
      }
  }
  if (!src || (size_t)count > avail) return fail(ICTR_ERR_INVALID, "read_buffer: unknown buffer or count too large");
  if (!b->projected && (which == 5 || which == 8 || which >= 100)) {  // what SetPose's deferred step 3 produces
    bool all_set = true;
    for (const ProbHost &ph : b->probs) all_set = all_set && ph.pose_set;
    if (all_set)
      if (int rc = ictr_batch_begin(b)) return rc;
  }
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipMemcpy(host_out, src, sizeof(float) * count, hipMemcpyDeviceToHost));
  return ICTR_OK;
}
extern "C" int ictr_odometer_read_buffer(ictr_odometer *o, int which, float *host_out, int64_t count) {
  if (!o) return fail(ICTR_ERR_INVALID, "odometer is NULL");
  return ictr_batch_read_buffer(o->b, 0, which, host_out, count);
}
extern "C" int ictr_odometer_get_norm(const ictr_odometer *o, double *meanshift3, double *varval) {
  if (!o) return fail(ICTR_ERR_INVALID, "odometer is NULL");
  if (meanshift3) memcpy(meanshift3, o->b->probs[0].meanshift, sizeof(double) * 3);
  if (varval) *varval = o->b->probs[0].varval;
  return ICTR_OK;
}

// ---------------------------------------------------------------- frame-to-frame sequence (run_odometer_test.m:172-250)
// One engine of one problem (B = 1) tracks frame t -> t+1 from the pose found for frame t, for every t, with the step
// between two pairs on the device (ictr_sequence.hip): per pair one pyramid build, the selection launches and ONE
// one-launch tracking, all on one stream; no host synchronisation and no copy until the results come back at the end.
// The launch form follows the cap (maxpttrack), decided once at creation (the batch's plan): the team form where
// track1_team takes the cap (psz 8), else one workgroup per tracking while the cap's point records fit its LDS; anything
// else is refused.
struct ictr_sequence {
  const ictr_cam *cam = nullptr;
  ictr_optparam op;
  // declared first, so released last: the inner batch, then the ring pyramids, after the sequence's own buffers
  std::unique_ptr<ictr_batch> b;
  std::unique_ptr<ictr_pyramid> ring[2];
  int64_t nw = 0;
  int stride = 10, nblk = 0;
  hipStream_t stream = nullptr;
  DevBuf<double> d_world;
  DevBuf<unsigned long long> d_mask;
  DevBuf<unsigned> d_cnt;
  DevBuf<int> d_sel;
  DevBuf<SeqState> d_ss;
  DevBuf<PlaneSet> d_tab;  // [2][nlev]: (ring 0 -> ring 1), (ring 1 -> ring 0)
  const float *frames = nullptr;  // [N][h][w] on the device (borrowed, or d_frames_own)
  DevBuf<float> d_frames_own;
  size_t own_bytes = 0;
  int64_t nframes = 0;
  int64_t run_frames = 0;  // frames of the last run (its results' layout in the result block)
  bool points_set = false;
  // (seq_layout) declared last, so destroyed first: a run in flight ends before a buffer, a pyramid or the batch goes
  Readback out;
};

struct SeqLayout {  // poses [N][6] f64 | hash [N-1] u64 | npts [N-1] i32 | iters [N-1] i32, packed
  Part poses, hash, npts, iters, end;  // end: empty, at the block's size
};
static SeqLayout seq_layout(int64_t N) {
  Carve c;
  const size_t n = (size_t)N, p = (size_t)(N - 1);  // frames, pairs
  return {c.take(sizeof(double) * 6 * n), c.take(sizeof(uint64_t) * p), c.take(sizeof(int32_t) * p),
          c.take(sizeof(int32_t) * p), c.take(0)};  // braces: evaluated in this order
}

extern "C" int ictr_sequence_create(ictr_sequence **out, const ictr_cam *cam, const ictr_optparam *op, int64_t nworld,
                                    int stride) {
  if (!out || !cam || !op) return fail(ICTR_ERR_INVALID, "sequence_create: NULL argument");
  if (nworld < 1 || nworld > (int64_t)1 << 24)
    return fail(ICTR_ERR_INVALID, "sequence_create: %lld world points (1 .. 2^24)", (long long)nworld);
  if (stride < 1) return fail(ICTR_ERR_INVALID, "sequence_create: the subsampling stride must be >= 1");
  if (int rc = check_op(op, cam)) return rc;
  if (int rc = need_device()) return rc;
  auto s = std::make_unique<ictr_sequence>();
  s->cam = cam;
  s->op = *op;
  s->nw = nworld;
  s->stride = stride;
  s->nblk = (int)((nworld + kSeqChunk - 1) / kSeqChunk);
  ictr_batch *b = nullptr;
  if (int rc = ictr_batch_create(&b, cam, &s->op, 1)) return rc;
  s->b.reset(b);
  // the engine as every pair's tracking sees it: builder-made gradient pyramids (otf = 1, packed planes), the cap as
  // the point capacity of the launch
  b->maxpts = b->M;
  b->otf = 1;
  memset(&b->plan, 0, sizeof(b->plan));
  b->plan.form = kFormTrack1;
  b->plan.project_here = 1;
  b->plan.team = track1_team(b, &b->plan.team_q);
  if (b->plan.team < 2 && (size_t)b->M * 64 > 128 * 1024)
    return fail(ICTR_ERR_INVALID, "sequence_create: a cap (maxpttrack) of %d points has no one-launch form: one workgroup "
                                  "holds at most 2048 point records, and the team form serves psz 8 only, up to 8192 "
                                  "points", b->M);
  const int L = b->nlev;
  if (int rc = s->d_world.alloc(sizeof(double) * 3 * nworld, true)) return rc;
  if (int rc = s->d_mask.alloc(sizeof(unsigned long long) * (size_t)s->nblk * (kSeqChunk / 64), true)) return rc;
  if (int rc = s->d_cnt.alloc(sizeof(unsigned) * s->nblk, true)) return rc;
  if (int rc = s->d_sel.alloc(sizeof(int) * b->M, true)) return rc;
  if (int rc = s->d_ss.alloc(sizeof(SeqState), true)) return rc;
  if (int rc = s->d_tab.alloc(sizeof(PlaneSet) * 2 * L, true)) return rc;
  for (int k = 0; k < 2; ++k) {
    ictr_pyramid *p = nullptr;
    if (int rc = pyramid_alloc(&p, cam->wh[0], cam->wh[1], op->lv_f, 1, cam->padding)) return rc;
    s->ring[k].reset(p);
  }
  // both orders of the plane table, once: pair t reads table t % 2 (reference = frame t's pyramid, ring[t % 2])
  std::vector<PlaneSet> tab(2 * L);
  for (int k = 0; k < 2; ++k)
    for (int l = 0; l < L; ++l) {
      const ictr_pyramid *r = s->ring[k].get(), *c = s->ring[1 - k].get();
      tab[k * L + l] = PlaneSet{r->img[l], r->dx[l], r->dy[l], c->img[l], r->pack[l]};
    }
  HIPCHK(hipMemcpy(s->d_tab.get(), tab.data(), sizeof(PlaneSet) * 2 * L, hipMemcpyHostToDevice));
  if (b->plan.team > 1) {  // the mailbox now, not inside the first track_async
    T1Team tm;
    if (int rc = team_prepare(b, b->plan, &tm)) return rc;
    HIPCHK(hipStreamSynchronize(b->stream));
  }
  *out = s.release();
  return ICTR_OK;
}

extern "C" void ictr_sequence_destroy(ictr_sequence *s) { delete s; }

extern "C" int ictr_sequence_set_points(ictr_sequence *s, const double *pt3d) {
  if (!s || !pt3d) return fail(ICTR_ERR_INVALID, "sequence_set_points: NULL argument");
  if (int rc = s->out.refuse("sequence_set_points", "sequence")) return rc;
  HIPCHK(hipMemcpy(s->d_world.get(), pt3d, sizeof(double) * 3 * s->nw, hipMemcpyHostToDevice));
  s->points_set = true;
  return ICTR_OK;
}

extern "C" int ictr_sequence_set_frames(ictr_sequence *s, const float *frames, int64_t nframes, int w, int h,
                                        int on_device) {
  if (!s || !frames) return fail(ICTR_ERR_INVALID, "sequence_set_frames: NULL argument");
  if (nframes < 2) return fail(ICTR_ERR_INVALID, "sequence_set_frames: %lld frames, a sequence needs at least 2",
                               (long long)nframes);
  if (w != s->cam->wh[0] || h != s->cam->wh[1])
    return fail(ICTR_ERR_INVALID, "sequence_set_frames: frames are %dx%d, the camera's are %dx%d", w, h, s->cam->wh[0],
                s->cam->wh[1]);
  if (int rc = s->out.refuse("sequence_set_frames", "sequence")) return rc;
  const size_t bytes = sizeof(float) * (size_t)w * h * nframes;
  if (on_device) {
    s->frames = frames;
  } else {
    if (bytes > s->own_bytes) {
      s->own_bytes = 0;
      if (int rc = s->d_frames_own.alloc(bytes)) return rc;
      s->own_bytes = bytes;
    }
    HIPCHK(hipMemcpy(s->d_frames_own.get(), frames, bytes, hipMemcpyHostToDevice));
    s->frames = s->d_frames_own.get();
  }
  // result buffers sized here, so that track_async allocates nothing
  if (int rc = s->out.reserve(seq_layout(nframes).end.at, false)) return rc;
  s->nframes = nframes;
  return ICTR_OK;
}

extern "C" int ictr_sequence_set_stream(ictr_sequence *s, void *hip_stream) {
  if (!s) return fail(ICTR_ERR_INVALID, "sequence is NULL");
  if (int rc = s->out.refuse("sequence_set_stream", "sequence")) return rc;
  s->stream = (hipStream_t)hip_stream;
  s->b->stream = s->stream;
  return ICTR_OK;
}

extern "C" int ictr_sequence_set_robust(ictr_sequence *s, int flags, float huber_k) {
  if (!s) return fail(ICTR_ERR_INVALID, "sequence is NULL");
  (void)huber_k;
  if (flags != 0)
    return fail(ICTR_ERR_INVALID, "sequence_set_robust: a sequence runs the plain one-launch forms only; robustness "
                                  "options (0x%x) are not available", flags);
  return ICTR_OK;
}

extern "C" int ictr_sequence_track_async(ictr_sequence *s, const double *p0) {
  if (!s || !p0) return fail(ICTR_ERR_INVALID, "sequence_track_async: NULL argument");
  if (!s->points_set) return fail(ICTR_ERR_STATE, "sequence_track_async: ictr_sequence_set_points has not been called");
  if (!s->frames || s->nframes < 2) return fail(ICTR_ERR_STATE, "sequence_track_async: no frames set");
  if (s->out.pending()) return fail(ICTR_ERR_STATE, "sequence_track_async: wait for the previous run first");
  ictr_batch *b = s->b.get();
  if (b->h_team_err && *(volatile int *)b->h_team_err.get()) {  // an earlier run timed out (reported by its wait)
    HIPCHK(hipStreamSynchronize(s->stream));
    *(volatile int *)b->h_team_err.get() = 0;
  }
  const int64_t N = s->nframes;
  const int w = s->cam->wh[0], h = s->cam->wh[1], L = b->nlev;
  const size_t plane = (size_t)w * h;
  SeqArgs a;
  memset(&a, 0, sizeof(a));
  a.X = s->d_world.get();
  a.nw = s->nw;
  a.nblk = s->nblk;
  a.stride = s->stride;
  a.cap = b->M;
  a.M = b->M;
  a.n = b->n;
  a.donorm = s->op.donorm ? 1 : 0;
  a.fx = s->cam->fx[0];
  a.fy = s->cam->fy[0];
  a.cx = s->cam->cx[0];
  a.cy = s->cam->cy[0];
  a.w = (double)w;
  a.h = (double)h;
  memcpy(a.p0, p0, sizeof(a.p0));
  a.st = b->d_st.get();
  a.ss = s->d_ss.get();
  a.mask = s->d_mask.get();
  a.cnt = s->d_cnt.get();
  a.sel = s->d_sel.get();
  const SeqLayout lay = seq_layout(N);
  a.poses = reinterpret_cast<double *>(s->out.dev() + lay.poses.at);
  a.hash = reinterpret_cast<unsigned long long *>(s->out.dev() + lay.hash.at);
  a.npts_out = reinterpret_cast<int *>(s->out.dev() + lay.npts.at);
  a.iters_out = reinterpret_cast<int *>(s->out.dev() + lay.iters.at);
  a.pt3d = b->d_pt3d.get();
  a.T = b->d_T.get();
  a.Gx = b->d_Gx.get();
  a.Gy = b->d_Gy.get();
  a.coef = b->d_coef.get();
  if (int rc = pyramid_build(s->ring[0].get(), s->frames, s->stream)) return rc;
  for (int64_t t = 0; t + 1 < N; ++t) {
    if (int rc = pyramid_build(s->ring[(t + 1) & 1].get(), s->frames + (size_t)(t + 1) * plane, s->stream)) return rc;
    a.t = (int)t;
    a.tail = 0;
    launch_seq_select(a, s->stream);
    HIPCHK(hipGetLastError());
    EngineDev e = engine_dev(b);
    e.planes = s->d_tab.get() + (t & 1) * L;
    if (int rc = track1_launch(b, e, b->plan, nullptr, nullptr, true)) return rc;
  }
  a.t = (int)(N - 1);
  a.tail = 1;
  launch_seq_select(a, s->stream);
  HIPCHK(hipGetLastError());
  if (int rc = s->out.post(lay.end.at, s->stream)) return rc;
  s->run_frames = N;
  return ICTR_OK;
}

extern "C" int ictr_sequence_wait(ictr_sequence *s, double *poses, int32_t *npts, int32_t *iters) {
  if (!s) return fail(ICTR_ERR_INVALID, "sequence is NULL");
  if (!s->out.pending()) return fail(ICTR_ERR_STATE, "sequence_wait: nothing has been tracked");
  if (int rc = s->out.wait()) return rc;
  if (int rc = team_error_check(s->b.get())) return rc;
  const SeqLayout L = seq_layout(s->run_frames);
  if (poses) memcpy(poses, s->out.host() + L.poses.at, L.poses.bytes);
  if (npts) memcpy(npts, s->out.host() + L.npts.at, L.npts.bytes);
  if (iters) memcpy(iters, s->out.host() + L.iters.at, L.iters.bytes);
  return ICTR_OK;
}

extern "C" int ictr_sequence_selection_hashes(const ictr_sequence *s, uint64_t *out) {
  if (!s || !out) return fail(ICTR_ERR_INVALID, "sequence_selection_hashes: NULL argument");
  if (s->out.pending() || !s->out.ran()) return fail(ICTR_ERR_STATE, "sequence_selection_hashes: no completed run");
  const SeqLayout L = seq_layout(s->run_frames);
  memcpy(out, s->out.host() + L.hash.at, L.hash.bytes);
  return ICTR_OK;
}

// inspection: what the LAST pair's selection left on the device. d_ss (ms, varval, npts), d_sel and the engine's pt3d
// are written by k_seq_select_finish / k_seq_select_scatter only; the tracking reads pt3d and the tail launch writes
// ss->pose alone, so after the wait they still hold the last pair's selection. Plain copies behind a stream sync.
extern "C" int ictr_sequence_last_selection(const ictr_sequence *s, int32_t *npts, int32_t *sel, double *ms3,
                                            double *varval, float *pt3d) {
  if (!s) return fail(ICTR_ERR_INVALID, "sequence_last_selection: NULL argument");
  if (s->out.pending() || !s->out.ran()) return fail(ICTR_ERR_STATE, "sequence_last_selection: no completed run");
  HIPCHK(hipStreamSynchronize(s->stream));
  SeqState ss;
  HIPCHK(hipMemcpy(&ss, s->d_ss.get(), sizeof(ss), hipMemcpyDeviceToHost));
  const int M = s->b->M;
  if (ss.npts < 0 || ss.npts > M) return fail(ICTR_ERR_STATE, "sequence_last_selection: %d points selected, cap %d", ss.npts, M);
  if (npts) *npts = ss.npts;
  if (ms3) memcpy(ms3, ss.ms, sizeof(double) * 3);
  if (varval) *varval = ss.varval;
  if (sel && ss.npts > 0) HIPCHK(hipMemcpy(sel, s->d_sel.get(), sizeof(int) * (size_t)ss.npts, hipMemcpyDeviceToHost));
  if (pt3d) HIPCHK(hipMemcpy(pt3d, s->b->d_pt3d.get(), sizeof(float) * 3 * (size_t)M, hipMemcpyDeviceToHost));
  return ICTR_OK;
}

// workgroups per tracking launch of the last run (before the first run: the form the cap selects)
extern "C" int ictr_sequence_last_team(const ictr_sequence *s) { return s ? s->b->plan.team : 0; }
