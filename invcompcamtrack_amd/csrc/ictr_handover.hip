// ictr_handover.hip -- the window hand-over (DESIGN.md §4 "Window hand-over"): the history [bsize][4][N] and the rows [M]
// of a counted stereo track window written, on the device, into the input buffers of the stages that follow, and one
// stage's inlier words copied into the mask of another. The objects' structs stay in their own files. The split's pairs
// are seen through ictr_fsplit_view; the fit, the adjuster and the window camera RANSAC each hand out their one input
// block (ictr_wininputs.h) as a WinDest (ictr_launch.h), so each hand-over is written once: ho_points, ho_obs, ho_mask,
// ho_debug_inputs. The public entries name the object and pass it on.
//
//   k_ho_pairs   grid (chunks of kBlock survivors, frames): the frame's four words into its places among the view pairs
//                [2 npairs][4][M] of fsplit.pairs_from_stereo_tracks; the middle frame of an odd window returns at once
//   k_ho_obs     same grid: the two words of one side into that side's observations [bsize][2][M]
//   k_ho_points  one thread per survivor: ho_point of ictr_handover_hd.h on frame 0 into X [3][M]
//
// Every thread reads rows[m] once; rows is ascending, so neighbouring lanes read neighbouring (or the same cache line's)
// words of a history column, and every store is coalesced over m. No atomics, no LDS, plain vector stores. The
// from-window entries enqueue on the null stream, like the window itself, and do not wait. They refuse in one order:
// NULL, window not counted, bsize < 2, size mismatch, run in flight, then camera not set or frame count; a refused call
// launches nothing and sets no flag.
#include <stdint.h>
#include <string.h>

#include "ictr_dev.h"
#include "ictr_handover_hd.h"
#include "ictr_launch.h"
#include "ictr_wininputs.h"

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

// a public entry's object as a destination (V = WinDest) or a mask source (WinMaskSrc) through its accessor `get`; all
// zero for a NULL object, which the helpers refuse
template <class T, class V>
V ho_of(T *r, int (*get)(T *, V *)) {
  V v = {};
  if (r) get(r, &v);
  return v;
}

// ho_point of frame 0 into the points, with the camera of the destination's set_camera
int ho_points(const WinDest &d, const ictr_stereotrack *t, double baseline, const char *what) {
  if (!d.in || !t) return null_object(what);
  HoArgs a;
  if (int rc = ho_window(t, d.in->n, what, &a)) return rc;
  if (int rc = d.out->refuse(what, d.object)) return rc;
  if (!d.in->cam_set) return fail(ICTR_ERR_STATE, "%s: ictr_%s_set_camera comes first", what, d.object);
  const HoCam cam = {d.in->cam.fx, d.in->cam.fy, d.in->cam.cx, d.in->cam.cy};
  hipLaunchKernelGGL(k_ho_points, dim3(ho_chunks(a.m)), dim3(kBlock), 0, nullptr, a, baseline * cam.fx, cam, d.in->X.get());
  HIPCHK(hipGetLastError());
  d.in->filled(true, false, false);
  return ICTR_OK;
}

// sides first_side .. first_side + nsides - 1 of the window into sides 0 .. nsides - 1 of the observations
int ho_obs(const WinDest &d, const ictr_stereotrack *t, int first_side, int nsides, const char *what) {
  if (!d.in || !t) return null_object(what);
  HoArgs a;
  if (int rc = ho_window(t, d.in->n, what, &a)) return rc;
  if (int rc = d.out->refuse(what, d.object)) return rc;
  if (d.in->nframes != a.bsize)
    return fail(ICTR_ERR_INVALID, "%s: the window has %d frames, the %s was made for %d", what, a.bsize, d.noun,
                d.in->nframes);
  for (int s = 0; s < nsides; ++s)
    hipLaunchKernelGGL(k_ho_obs, dim3(ho_chunks(a.m), (unsigned)a.bsize), dim3(kBlock), 0, nullptr, a, first_side + s,
                       d.in->xy.get() + (size_t)s * (size_t)a.bsize * 2 * (size_t)a.m);
  HIPCHK(hipGetLastError());
  d.in->filled(false, true, false);
  return ICTR_OK;
}

// the inlier words of the source's last run, waited for or in flight, into the mask words, on the device on `stream`
int ho_mask(const WinDest &d, const WinMaskSrc &src, void *stream, const char *what) {
  if (!d.in || !src.noun) return null_object(what);
  if (int rc = d.out->refuse(what, d.object)) return rc;
  if (!src.ran) return fail(ICTR_ERR_STATE, "%s: the %s has never run", what, src.noun);
  if (src.n != d.in->n)
    return fail(ICTR_ERR_INVALID, "%s: the %s has %d points, the %s %d", what, src.noun, src.n, d.noun, d.in->n);
  HIPCHK(hipMemcpyAsync(d.in->words.get(), src.words, sizeof(unsigned long long) * (size_t)d.in->nwords,
                        hipMemcpyDeviceToDevice, (hipStream_t)stream));
  d.in->filled(false, false, true);
  return ICTR_OK;
}

// inspection: the device buffers as they stand, after everything enqueued so far on any stream. in_effect: where no mask
// is in use the words answer every point's bit (bits past n clear), not the buffer
int ho_debug_inputs(const WinDest &d, double *X, double *xy, uint64_t *words, bool in_effect = false) {
  const WinInputs &in = *d.in;
  HIPCHK(hipDeviceSynchronize());
  if (X) HIPCHK(hipMemcpy(X, in.X.get(), sizeof(double) * 3 * (size_t)in.n, hipMemcpyDeviceToHost));
  if (xy) HIPCHK(hipMemcpy(xy, in.xy.get(), sizeof(double) * in.obs_count(), hipMemcpyDeviceToHost));
  if (words && in_effect && !in.use_mask) {
    for (int w = 0; w < in.nwords; ++w) words[w] = ~0ull;
    if (in.n & 63) words[in.nwords - 1] = (1ull << (in.n & 63)) - 1ull;
  } else if (words) {
    HIPCHK(hipMemcpy(words, in.words.get(), sizeof(uint64_t) * (size_t)in.nwords, hipMemcpyDeviceToHost));
  }
  return ICTR_OK;
}

}  // namespace

// ---------------------------------------------------------------- the split's pairs
extern "C" int ictr_fsplit_set_pairs_from_window(ictr_fsplit *r, const ictr_stereotrack *t) {
  const char *what = "fsplit_set_pairs_from_window";
  if (!r || !t) return null_object(what);
  ictr_fsplit_view d;
  if (int rc = ictr_fsplit_view_(r, &d)) return rc;
  HoArgs a;
  if (int rc = ho_window(t, d.n, what, &a)) return rc;
  if (d.pending) return fail(ICTR_ERR_STATE, "%s: a run is in flight; call ictr_fsplit_wait first", what);
  if (d.np != 2 * ho_npairs(a.bsize))
    return fail(ICTR_ERR_INVALID, "%s: a window of %d frames gives %d view pairs, the split was made for %d", what, a.bsize,
                2 * ho_npairs(a.bsize), d.np);
  hipLaunchKernelGGL(k_ho_pairs, dim3(ho_chunks(a.m), (unsigned)a.bsize), dim3(kBlock), 0, nullptr, a, d.xy);
  HIPCHK(hipGetLastError());
  ictr_fsplit_pairs_filled_(r);
  return ICTR_OK;
}

extern "C" int ictr_debug_fsplit_pairs(const ictr_fsplit *r, double *xy) {
  if (!r || !xy) return null_object("debug_fsplit_pairs");
  ictr_fsplit_view v;
  if (int rc = ictr_fsplit_view_(r, &v)) return rc;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(xy, v.xy, sizeof(double) * 4 * (size_t)v.np * (size_t)v.n, hipMemcpyDeviceToHost));
  return ICTR_OK;
}

// ---------------------------------------------------------------- the camera fit (one side: left, or with `right` the right)
extern "C" int ictr_camfit_set_points_from_window(ictr_camfit *r, const ictr_stereotrack *t, double baseline) {
  return ho_points(ho_of(r, ictr_camfit_inputs_), t, baseline, "camfit_set_points_from_window");
}
extern "C" int ictr_camfit_set_observations_from_window(ictr_camfit *r, const ictr_stereotrack *t, int right) {
  return ho_obs(ho_of(r, ictr_camfit_inputs_), t, right != 0 ? 1 : 0, 1, "camfit_set_observations_from_window");
}
extern "C" int ictr_camfit_set_mask_from_fsplit(ictr_camfit *r, const ictr_fsplit *s, void *hip_stream) {
  return ho_mask(ho_of(r, ictr_camfit_inputs_), ho_of(s, ictr_fsplit_mask_), hip_stream, "camfit_set_mask_from_fsplit");
}
extern "C" int ictr_camfit_set_mask_from_camransac(ictr_camfit *r, const ictr_camransac *s, void *hip_stream) {
  return ho_mask(ho_of(r, ictr_camfit_inputs_), ho_of(s, ictr_camransac_mask_), hip_stream,
                 "camfit_set_mask_from_camransac");
}
extern "C" int ictr_debug_camfit_inputs(const ictr_camfit *r, double *X, double *xy, uint64_t *words) {
  if (!r) return fail(ICTR_ERR_INVALID, "debug_camfit_inputs: camfit is NULL");
  return ho_debug_inputs(ho_of(const_cast<ictr_camfit *>(r), ictr_camfit_inputs_), X, xy, words);
}

// ---------------------------------------------------------------- the bundle adjuster (every side it was made for)
extern "C" int ictr_ba_set_points_from_window(ictr_ba *r, const ictr_stereotrack *t, double baseline) {
  return ho_points(ho_of(r, ictr_ba_inputs_), t, baseline, "ba_set_points_from_window");
}
extern "C" int ictr_ba_set_observations_from_window(ictr_ba *r, const ictr_stereotrack *t) {
  const WinDest d = ho_of(r, ictr_ba_inputs_);
  return ho_obs(d, t, 0, d.in ? d.in->nsides : 0, "ba_set_observations_from_window");
}
extern "C" int ictr_ba_set_mask_from_fsplit(ictr_ba *r, const ictr_fsplit *s, void *hip_stream) {
  return ho_mask(ho_of(r, ictr_ba_inputs_), ho_of(s, ictr_fsplit_mask_), hip_stream, "ba_set_mask_from_fsplit");
}
extern "C" int ictr_ba_set_mask_from_camransac(ictr_ba *r, const ictr_camransac *s, void *hip_stream) {
  return ho_mask(ho_of(r, ictr_ba_inputs_), ho_of(s, ictr_camransac_mask_), hip_stream, "ba_set_mask_from_camransac");
}
extern "C" int ictr_debug_ba_inputs(const ictr_ba *r, double *X, double *xy, uint64_t *words) {
  if (!r) return fail(ICTR_ERR_INVALID, "debug_ba_inputs: ba is NULL");
  return ho_debug_inputs(ho_of(const_cast<ictr_ba *>(r), ictr_ba_inputs_), X, xy, words);
}

// ---------------------------------------------------------------- the window camera RANSAC (every side it was made for)
extern "C" int ictr_camransac_set_points_from_window(ictr_camransac *r, const ictr_stereotrack *t, double baseline) {
  return ho_points(ho_of(r, ictr_camransac_inputs_), t, baseline, "camransac_set_points_from_window");
}
extern "C" int ictr_camransac_set_observations_from_window(ictr_camransac *r, const ictr_stereotrack *t) {
  const WinDest d = ho_of(r, ictr_camransac_inputs_);
  return ho_obs(d, t, 0, d.in ? d.in->nsides : 0, "camransac_set_observations_from_window");
}
extern "C" int ictr_debug_camransac_inputs(const ictr_camransac *r, double *X, double *xy, uint64_t *words) {
  if (!r) return fail(ICTR_ERR_INVALID, "debug_camransac_inputs: camransac is NULL");
  return ho_debug_inputs(ho_of(const_cast<ictr_camransac *>(r), ictr_camransac_inputs_), X, xy, words, true);  // in effect
}
