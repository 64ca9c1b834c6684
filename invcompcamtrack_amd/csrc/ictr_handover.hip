// ictr_handover.hip -- the window hand-over (DESIGN.md §4 "Window hand-over"): the history [bsize][4][N] and the rows [M]
// of a counted stereo track window written, on the device, into the input buffers of the static split and of the camera
// fit, and the split's inlier words copied into the fit. The objects' structs stay in their own files; this file sees
// them through the views of ictr_launch.h.
//
//   k_ho_pairs   grid (chunks of kBlock survivors, frames): the frame's four words into its places among the view pairs
//                [2 npairs][4][M] of fsplit.pairs_from_stereo_tracks; the middle frame of an odd window returns at once
//   k_ho_obs     same grid: the two words of one side into the observations [bsize][2][M]
//   k_ho_points  one thread per survivor: ho_point of ictr_handover_hd.h on frame 0 into X [3][M]
//
// The adjuster (ictr_ba.hip) takes its points, both sides of its observations and its mask by the same kernels, and so
// does the window camera RANSAC (ictr_camransac.hip), whose winner's words in turn mask the fit and the adjuster.
//
// Every thread reads rows[m] once; rows is ascending, so neighbouring lanes read neighbouring (or the same cache line's)
// words of a history column, and every store is coalesced over m. No atomics, no LDS, plain vector stores. The three
// from-window entries enqueue on the null stream, like the window itself, and do not wait.
#include <stdint.h>
#include <string.h>

#include "ictr_dev.h"
#include "ictr_handover_hd.h"
#include "ictr_launch.h"

namespace ictr {

struct HoArgs {
  const double *hist;     // [bsize][4][n]
  const long long *rows;  // [m]
  int n, m, bsize;
};

__device__ __forceinline__ double ho_word(const HoArgs &a, int fr, int c, size_t r) {
  return a.hist[((size_t)fr * 4 + (size_t)c) * (size_t)a.n + r];
}

__global__ __launch_bounds__(kBlock) void k_ho_pairs(HoArgs a, double *__restrict__ pairs) {
  const int fr = blockIdx.y, np = ho_npairs(a.bsize), off = ho_offset(a.bsize);
  const bool first = fr < np, second = fr >= off;  // never both; neither: the middle frame of an odd window
  if (!first && !second) return;
  const int m = blockIdx.x * kBlock + threadIdx.x;
  if (m >= a.m) return;
  const size_t r = (size_t)a.rows[m], M = (size_t)a.m;
  const double xl = ho_word(a, fr, 0, r), yl = ho_word(a, fr, 1, r), xr = ho_word(a, fr, 2, r), yr = ho_word(a, fr, 3, r);
  // view pairs 2 g and 2 g + 1 of frame pair g: (left g -> right g + off) and (right g -> left g + off)
  double *p = pairs + (size_t)(2 * (first ? fr : fr - off)) * 4 * M + (size_t)m;
  if (first) {
    p[0] = xl;
    p[M] = yl;
    p[4 * M] = xr;
    p[5 * M] = yr;
  } else {
    p[2 * M] = xr;
    p[3 * M] = yr;
    p[6 * M] = xl;
    p[7 * M] = yl;
  }
}

__global__ __launch_bounds__(kBlock) void k_ho_obs(HoArgs a, int right, double *__restrict__ xy) {
  const int fr = blockIdx.y, m = blockIdx.x * kBlock + threadIdx.x;
  if (m >= a.m) return;
  const size_t r = (size_t)a.rows[m], M = (size_t)a.m;
  const int c = right ? 2 : 0;
  double *o = xy + (size_t)fr * 2 * M + (size_t)m;
  o[0] = ho_word(a, fr, c, r);
  o[M] = ho_word(a, fr, c + 1, r);
}

__global__ __launch_bounds__(kBlock) void k_ho_points(HoArgs a, double bf, HoCam cam, double *__restrict__ X) {
  const int m = blockIdx.x * kBlock + threadIdx.x;
  if (m >= a.m) return;
  const size_t r = (size_t)a.rows[m], M = (size_t)a.m;
  double p[3];
  ho_point(ho_word(a, 0, 0, r), ho_word(a, 0, 1, r), ho_word(a, 0, 2, r), bf, cam, p);
  X[m] = p[0];
  X[M + (size_t)m] = p[1];
  X[2 * M + (size_t)m] = p[2];
}

}  // namespace ictr

using namespace ictr;

namespace {

// the window as a kernel argument, for a destination made for n_dest points; what: the entry's name
int ho_window(const ictr_stereotrack *t, int n_dest, const char *what, HoArgs *a) {
  ictr_stereotrack_view v;
  if (int rc = ictr_stereotrack_view_(t, &v)) return rc;
  if (!v.counted) return fail(ICTR_ERR_STATE, "%s: the window is not counted; ictr_stereotrack_count comes first", what);
  if (v.bsize < 2) return fail(ICTR_ERR_INVALID, "%s: a window of %d frame has no frame pair (bsize 2 .. 65)", what, v.bsize);
  if (v.m != n_dest)
    return fail(ICTR_ERR_INVALID, "%s: the window kept %lld points, the object was made for %d", what, v.m, n_dest);
  a->hist = v.hist;
  a->rows = v.rows;
  a->n = v.n;
  a->m = (int)v.m;
  a->bsize = v.bsize;
  return ICTR_OK;
}

unsigned ho_chunks(int m) { return (unsigned)((m + kBlock - 1) / kBlock); }

int ho_in_flight(const char *what, const char *object) {
  return fail(ICTR_ERR_STATE, "%s: a run is in flight; call ictr_%s_wait first", what, object);
}

}  // namespace

extern "C" int ictr_fsplit_set_pairs_from_window(ictr_fsplit *r, const ictr_stereotrack *t) {
  const char *what = "fsplit_set_pairs_from_window";
  if (!r || !t) return fail(ICTR_ERR_INVALID, "%s: NULL argument", what);
  ictr_fsplit_view d;
  if (int rc = ictr_fsplit_view_(r, &d)) return rc;
  HoArgs a;
  if (int rc = ho_window(t, d.n, what, &a)) return rc;
  if (d.pending) return ho_in_flight(what, "fsplit");
  if (d.np != 2 * ho_npairs(a.bsize))
    return fail(ICTR_ERR_INVALID, "%s: a window of %d frames gives %d view pairs, the split was made for %d", what, a.bsize,
                2 * ho_npairs(a.bsize), d.np);
  hipLaunchKernelGGL(k_ho_pairs, dim3(ho_chunks(a.m), (unsigned)a.bsize), dim3(kBlock), 0, nullptr, a, d.xy);
  HIPCHK(hipGetLastError());
  ictr_fsplit_pairs_filled_(r);
  return ICTR_OK;
}

extern "C" int ictr_camfit_set_points_from_window(ictr_camfit *r, const ictr_stereotrack *t, double baseline) {
  const char *what = "camfit_set_points_from_window";
  if (!r || !t) return fail(ICTR_ERR_INVALID, "%s: NULL argument", what);
  ictr_camfit_view d;
  if (int rc = ictr_camfit_view_(r, &d)) return rc;
  HoArgs a;
  if (int rc = ho_window(t, d.n, what, &a)) return rc;
  if (d.pending) return ho_in_flight(what, "camfit");
  if (!d.cam_set) return fail(ICTR_ERR_STATE, "%s: ictr_camfit_set_camera comes first", what);
  const HoCam cam = {d.fc[0], d.fc[1], d.cc[0], d.cc[1]};
  hipLaunchKernelGGL(k_ho_points, dim3(ho_chunks(a.m)), dim3(kBlock), 0, nullptr, a, baseline * cam.fx, cam, d.X);
  HIPCHK(hipGetLastError());
  ictr_camfit_filled_(r, 1, 0, 0);
  return ICTR_OK;
}

extern "C" int ictr_camfit_set_observations_from_window(ictr_camfit *r, const ictr_stereotrack *t, int right) {
  const char *what = "camfit_set_observations_from_window";
  if (!r || !t) return fail(ICTR_ERR_INVALID, "%s: NULL argument", what);
  ictr_camfit_view d;
  if (int rc = ictr_camfit_view_(r, &d)) return rc;
  HoArgs a;
  if (int rc = ho_window(t, d.n, what, &a)) return rc;
  if (d.pending) return ho_in_flight(what, "camfit");
  if (d.nframes != a.bsize)
    return fail(ICTR_ERR_INVALID, "%s: the window has %d frames, the fit was made for %d", what, a.bsize, d.nframes);
  hipLaunchKernelGGL(k_ho_obs, dim3(ho_chunks(a.m), (unsigned)a.bsize), dim3(kBlock), 0, nullptr, a, right != 0 ? 1 : 0, d.xy);
  HIPCHK(hipGetLastError());
  ictr_camfit_filled_(r, 0, 1, 0);
  return ICTR_OK;
}

extern "C" int ictr_camfit_set_mask_from_fsplit(ictr_camfit *r, const ictr_fsplit *s, void *hip_stream) {
  const char *what = "camfit_set_mask_from_fsplit";
  if (!r || !s) return fail(ICTR_ERR_INVALID, "%s: NULL argument", what);
  ictr_camfit_view d;
  ictr_fsplit_view v;
  if (int rc = ictr_camfit_view_(r, &d)) return rc;
  if (int rc = ictr_fsplit_view_(s, &v)) return rc;
  if (d.pending) return ho_in_flight(what, "camfit");
  if (!v.ran) return fail(ICTR_ERR_STATE, "%s: the split has never run", what);
  if (v.n != d.n) return fail(ICTR_ERR_INVALID, "%s: the split has %d points, the fit %d", what, v.n, d.n);
  HIPCHK(hipMemcpyAsync(d.words, v.words, sizeof(unsigned long long) * (size_t)d.nwords, hipMemcpyDeviceToDevice,
                        (hipStream_t)hip_stream));
  ictr_camfit_filled_(r, 0, 0, 1);
  return ICTR_OK;
}

// the adjuster's inputs from the same window: ho_point into the points as set, k_ho_obs once per side
extern "C" int ictr_ba_set_points_from_window(ictr_ba *r, const ictr_stereotrack *t, double baseline) {
  const char *what = "ba_set_points_from_window";
  if (!r || !t) return fail(ICTR_ERR_INVALID, "%s: NULL argument", what);
  ictr_ba_view d;
  if (int rc = ictr_ba_view_(r, &d)) return rc;
  HoArgs a;
  if (int rc = ho_window(t, d.n, what, &a)) return rc;
  if (d.pending) return ho_in_flight(what, "ba");
  if (!d.cam_set) return fail(ICTR_ERR_STATE, "%s: ictr_ba_set_camera comes first", what);
  const HoCam cam = {d.fc[0], d.fc[1], d.cc[0], d.cc[1]};
  hipLaunchKernelGGL(k_ho_points, dim3(ho_chunks(a.m)), dim3(kBlock), 0, nullptr, a, baseline * cam.fx, cam, d.X);
  HIPCHK(hipGetLastError());
  ictr_ba_filled_(r, 1, 0, 0);
  return ICTR_OK;
}

extern "C" int ictr_ba_set_observations_from_window(ictr_ba *r, const ictr_stereotrack *t) {
  const char *what = "ba_set_observations_from_window";
  if (!r || !t) return fail(ICTR_ERR_INVALID, "%s: NULL argument", what);
  ictr_ba_view d;
  if (int rc = ictr_ba_view_(r, &d)) return rc;
  HoArgs a;
  if (int rc = ho_window(t, d.n, what, &a)) return rc;
  if (d.pending) return ho_in_flight(what, "ba");
  if (d.nframes != a.bsize)
    return fail(ICTR_ERR_INVALID, "%s: the window has %d frames, the adjuster was made for %d", what, a.bsize, d.nframes);
  for (int s = 0; s < d.nsides; ++s)
    hipLaunchKernelGGL(k_ho_obs, dim3(ho_chunks(a.m), (unsigned)a.bsize), dim3(kBlock), 0, nullptr, a, s,
                       d.xy + (size_t)s * (size_t)a.bsize * 2 * (size_t)a.m);
  HIPCHK(hipGetLastError());
  ictr_ba_filled_(r, 0, 1, 0);
  return ICTR_OK;
}

extern "C" int ictr_ba_set_mask_from_fsplit(ictr_ba *r, const ictr_fsplit *s, void *hip_stream) {
  const char *what = "ba_set_mask_from_fsplit";
  if (!r || !s) return fail(ICTR_ERR_INVALID, "%s: NULL argument", what);
  ictr_ba_view d;
  ictr_fsplit_view v;
  if (int rc = ictr_ba_view_(r, &d)) return rc;
  if (int rc = ictr_fsplit_view_(s, &v)) return rc;
  if (d.pending) return ho_in_flight(what, "ba");
  if (!v.ran) return fail(ICTR_ERR_STATE, "%s: the split has never run", what);
  if (v.n != d.n) return fail(ICTR_ERR_INVALID, "%s: the split has %d points, the adjuster %d", what, v.n, d.n);
  HIPCHK(hipMemcpyAsync(d.words, v.words, sizeof(unsigned long long) * (size_t)d.nwords, hipMemcpyDeviceToDevice,
                        (hipStream_t)hip_stream));
  ictr_ba_filled_(r, 0, 0, 1);
  return ICTR_OK;
}

// the window camera RANSAC's inputs from the same window, by the same kernels; its winner's words as a mask
extern "C" int ictr_camransac_set_points_from_window(ictr_camransac *r, const ictr_stereotrack *t, double baseline) {
  const char *what = "camransac_set_points_from_window";
  if (!r || !t) return fail(ICTR_ERR_INVALID, "%s: NULL argument", what);
  ictr_camransac_view d;
  if (int rc = ictr_camransac_view_(r, &d)) return rc;
  HoArgs a;
  if (int rc = ho_window(t, d.n, what, &a)) return rc;
  if (d.pending) return ho_in_flight(what, "camransac");
  if (!d.cam_set) return fail(ICTR_ERR_STATE, "%s: ictr_camransac_set_camera comes first", what);
  const HoCam cam = {d.fc[0], d.fc[1], d.cc[0], d.cc[1]};
  hipLaunchKernelGGL(k_ho_points, dim3(ho_chunks(a.m)), dim3(kBlock), 0, nullptr, a, baseline * cam.fx, cam, d.X);
  HIPCHK(hipGetLastError());
  ictr_camransac_filled_(r, 1, 0);
  return ICTR_OK;
}

extern "C" int ictr_camransac_set_observations_from_window(ictr_camransac *r, const ictr_stereotrack *t) {
  const char *what = "camransac_set_observations_from_window";
  if (!r || !t) return fail(ICTR_ERR_INVALID, "%s: NULL argument", what);
  ictr_camransac_view d;
  if (int rc = ictr_camransac_view_(r, &d)) return rc;
  HoArgs a;
  if (int rc = ho_window(t, d.n, what, &a)) return rc;
  if (d.pending) return ho_in_flight(what, "camransac");
  if (d.nframes != a.bsize)
    return fail(ICTR_ERR_INVALID, "%s: the window has %d frames, the RANSAC was made for %d", what, a.bsize, d.nframes);
  for (int s = 0; s < d.nsides; ++s)
    hipLaunchKernelGGL(k_ho_obs, dim3(ho_chunks(a.m), (unsigned)a.bsize), dim3(kBlock), 0, nullptr, a, s,
                       d.xy + (size_t)s * (size_t)a.bsize * 2 * (size_t)a.m);
  HIPCHK(hipGetLastError());
  ictr_camransac_filled_(r, 0, 1);
  return ICTR_OK;
}

extern "C" int ictr_camfit_set_mask_from_camransac(ictr_camfit *r, const ictr_camransac *s, void *hip_stream) {
  const char *what = "camfit_set_mask_from_camransac";
  if (!r || !s) return fail(ICTR_ERR_INVALID, "%s: NULL argument", what);
  ictr_camfit_view d;
  ictr_camransac_view v;
  if (int rc = ictr_camfit_view_(r, &d)) return rc;
  if (int rc = ictr_camransac_view_(s, &v)) return rc;
  if (d.pending) return ho_in_flight(what, "camfit");
  if (!v.ran) return fail(ICTR_ERR_STATE, "%s: the RANSAC has never run", what);
  if (v.n != d.n) return fail(ICTR_ERR_INVALID, "%s: the RANSAC has %d points, the fit %d", what, v.n, d.n);
  HIPCHK(hipMemcpyAsync(d.words, v.words, sizeof(unsigned long long) * (size_t)d.nwords, hipMemcpyDeviceToDevice,
                        (hipStream_t)hip_stream));
  ictr_camfit_filled_(r, 0, 0, 1);
  return ICTR_OK;
}

extern "C" int ictr_ba_set_mask_from_camransac(ictr_ba *r, const ictr_camransac *s, void *hip_stream) {
  const char *what = "ba_set_mask_from_camransac";
  if (!r || !s) return fail(ICTR_ERR_INVALID, "%s: NULL argument", what);
  ictr_ba_view d;
  ictr_camransac_view v;
  if (int rc = ictr_ba_view_(r, &d)) return rc;
  if (int rc = ictr_camransac_view_(s, &v)) return rc;
  if (d.pending) return ho_in_flight(what, "ba");
  if (!v.ran) return fail(ICTR_ERR_STATE, "%s: the RANSAC has never run", what);
  if (v.n != d.n) return fail(ICTR_ERR_INVALID, "%s: the RANSAC has %d points, the adjuster %d", what, v.n, d.n);
  HIPCHK(hipMemcpyAsync(d.words, v.words, sizeof(unsigned long long) * (size_t)d.nwords, hipMemcpyDeviceToDevice,
                        (hipStream_t)hip_stream));
  ictr_ba_filled_(r, 0, 0, 1);
  return ICTR_OK;
}

extern "C" int ictr_debug_camransac_inputs(const ictr_camransac *r, double *X, double *xy, uint64_t *words) {
  if (!r) return fail(ICTR_ERR_INVALID, "debug_camransac_inputs: camransac is NULL");
  ictr_camransac_view v;
  if (int rc = ictr_camransac_view_(r, &v)) return rc;
  HIPCHK(hipDeviceSynchronize());
  const size_t n = (size_t)v.n;
  if (X) HIPCHK(hipMemcpy(X, v.X, sizeof(double) * 3 * n, hipMemcpyDeviceToHost));
  if (xy) HIPCHK(hipMemcpy(xy, v.xy, sizeof(double) * 2 * (size_t)v.nsides * (size_t)v.nframes * n, hipMemcpyDeviceToHost));
  if (words) {  // the mask in effect: every point where none is in use (bits past n clear)
    if (v.use_mask) {
      HIPCHK(hipMemcpy(words, v.mask, sizeof(uint64_t) * (size_t)v.nwords, hipMemcpyDeviceToHost));
    } else {
      for (int w = 0; w < v.nwords; ++w) words[w] = ~0ull;
      if (v.n & 63) words[v.nwords - 1] = (1ull << (v.n & 63)) - 1ull;
    }
  }
  return ICTR_OK;
}

extern "C" int ictr_debug_ba_inputs(const ictr_ba *r, double *X, double *xy, uint64_t *words) {
  if (!r) return fail(ICTR_ERR_INVALID, "debug_ba_inputs: ba is NULL");
  ictr_ba_view v;
  if (int rc = ictr_ba_view_(r, &v)) return rc;
  HIPCHK(hipDeviceSynchronize());
  const size_t n = (size_t)v.n;
  if (X) HIPCHK(hipMemcpy(X, v.X, sizeof(double) * 3 * n, hipMemcpyDeviceToHost));
  if (xy) HIPCHK(hipMemcpy(xy, v.xy, sizeof(double) * 2 * (size_t)v.nsides * (size_t)v.nframes * n, hipMemcpyDeviceToHost));
  if (words) HIPCHK(hipMemcpy(words, v.words, sizeof(uint64_t) * (size_t)v.nwords, hipMemcpyDeviceToHost));
  return ICTR_OK;
}

// inspection: the device buffers as they stand, after everything enqueued so far on any stream
extern "C" int ictr_debug_fsplit_pairs(const ictr_fsplit *r, double *xy) {
  if (!r || !xy) return fail(ICTR_ERR_INVALID, "debug_fsplit_pairs: NULL argument");
  ictr_fsplit_view v;
  if (int rc = ictr_fsplit_view_(r, &v)) return rc;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(xy, v.xy, sizeof(double) * 4 * (size_t)v.np * (size_t)v.n, hipMemcpyDeviceToHost));
  return ICTR_OK;
}

extern "C" int ictr_debug_camfit_inputs(const ictr_camfit *r, double *X, double *xy, uint64_t *words) {
  if (!r) return fail(ICTR_ERR_INVALID, "debug_camfit_inputs: camfit is NULL");
  ictr_camfit_view v;
  if (int rc = ictr_camfit_view_(r, &v)) return rc;
  HIPCHK(hipDeviceSynchronize());
  const size_t n = (size_t)v.n;
  if (X) HIPCHK(hipMemcpy(X, v.X, sizeof(double) * 3 * n, hipMemcpyDeviceToHost));
  if (xy) HIPCHK(hipMemcpy(xy, v.xy, sizeof(double) * 2 * (size_t)v.nframes * n, hipMemcpyDeviceToHost));
  if (words) HIPCHK(hipMemcpy(words, v.words, sizeof(uint64_t) * (size_t)v.nwords, hipMemcpyDeviceToHost));
  return ICTR_OK;
}
