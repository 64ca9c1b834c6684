/*
 * ictr.h -- C-ABI of the MI355X-native Gauss-Newton photometric tracker.
 *
 * Drop-in boundary for the per-frame tracking hot path of catree/InvCompCamTrack. The reference
 * has NO C-ABI for this path: its boundary is the C++ class API in namespace CTR
 * (camera.h:19-31, pose.h:18-40, odometer.h:21-30, utilities.h:46-82) that the two CLI drivers
 * link statically (run_io_reprojection_test.cpp:189-223, run_track_nposes.cpp:185-259). This header
 * mirrors those classes one method per function, with opaque handles, plain pointers and sizes,
 * following the conventions of the reference's only real FFI (misc_src/triang.c + its ctypes
 * callers, func_util_geom.py:582-606): caller-owned C-contiguous float32/float64 buffers, results
 * written into caller-allocated outputs. Differences, all deliberate:
 *   - every function returns an int status (0 = ok) instead of void; nothing throws across the ABI;
 *     ictr_last_error() gives the message. (The reference ignores all errors.)
 *   - counts are int64_t (the reference's ctypes callers pass c_longlong against C int).
 *   - image pyramids are device-resident handles (ictr_pyramid) built by HIP kernels, replacing the
 *     cv::Mat-typed util_constructpyramide (utilities.h:63-64); ictr_odometer_setpose_host keeps the
 *     reference's literal "const float** level pointer" signature for callers that own host planes.
 *   - ictr_batch_* runs B independent tracking problems per launch (the run_track_nposes pose-sample
 *     axis, run_track_nposes.cpp:193); an ictr_odometer is a batch of one.
 *
 * include/ctr_shim.hpp re-creates namespace CTR {CamClass, PoseClass, OdometerClass} on top of
 * these functions; INTEGRATION.md shows the ctypes binding.
 *
 * All hot-path arithmetic runs in hand-written HIP kernels for gfx950; there is no CPU fallback:
 * every entry point that needs the GPU fails with ICTR_ERR_NO_DEVICE when none is usable.
 */
#ifndef ICTR_H
#define ICTR_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ICTR_OK 0
#define ICTR_ERR_INVALID 1   /* bad argument */
#define ICTR_ERR_NO_DEVICE 2 /* no usable HIP device */
#define ICTR_ERR_HIP 3       /* a HIP runtime call failed */
#define ICTR_ERR_STATE 4     /* call order violated (e.g. TrackPose before SetPose) */

/* optparam, utilities.h:46-61 -- field order and types preserved verbatim */
typedef struct ictr_optparam {
  int maxpttrack;   /* SoA stride M of all point arrays; drivers round it up to a multiple of 4 */
  int psz;          /* patch size P */
  int pszd2;        /* P/2 */
  int pszd2m3;      /* P + P/2 - 1 */
  int novals;       /* P*P */
  int lv_f;         /* coarsest pyramid level (first processed) */
  int lv_l;         /* finest pyramid level (last processed) */
  bool donorm;      /* point cloud + pose normalisation */
  bool dopatchnorm; /* patch mean subtraction */
  int maxiter;
  float normdp_ratio;
  int verbosity;
} ictr_optparam;

/* fills the derived fields exactly as run_io_reprojection_test.cpp:112-126 does */
int ictr_optparam_init(ictr_optparam *op, int lv_f, int lv_l, int psz, int maxiter, float normdp_ratio,
                       int donorm, int dopatchnorm, int maxpttrack, int verbosity);

const char *ictr_last_error(void);
int ictr_version(void);
/* number of usable HIP devices (0 when none); never fails */
int ictr_device_count(void);
int ictr_set_device(int device);
/* measured streaming-read bandwidth of the current GPU in GB/s (bytes >= 1 MiB read reps times with wide loads):
 * the practical HBM ceiling to quote next to the vendor peak in roofline reports */
int ictr_stream_read_bandwidth(size_t bytes, int reps, double *gbps_out);
/* inspection: the transposing wave reduction of the resident-iteration kernel alone, on caller data.
 * vals[64 lanes][64 values], value index = 2 * patch + kind -> out[lane] = sum over the 64 lanes of value
 * 2 * patch_of_lane[lane] + kind_of_lane[lane] (all host arrays; 64 entries each) */
int ictr_debug_transpose_reduce(const float *vals, float *out, int *patch_of_lane, int *kind_of_lane,
                                int patches_per_wave /* 16 or 32: the kernel's two instantiations; 16 uses values 0..31 */);
/* inspection: the half-window fetch path of the resident-iteration kernel alone, one wave, eight 9x9 windows of a
 * caller plane[rows][sw] (all host arrays). top_left[8] = texel index of each window's top-left texel; the windows must
 * lie in the plane. out[8][64][4]: for window g and lane = pixel (row lane / 8, column lane % 8) the four bilinear taps
 * a, b, c, d = window texels (row + 1, col + 1), (row + 1, col), (row, col + 1), (row, col) */
int ictr_debug_half_window(const float *plane, int rows, int sw, const int *top_left, float *out);
/* inspection: the solver turn's 6x6 full-pivot LU on the device (one wave per system, n systems, all host arrays):
 * H36[n][36] symmetric (the kernel reads the upper triangle), b6[n][6] -> x6[n][6], rank[n], nonzero[n] (non-zero
 * pivots), the composed permutations rowmap6 / colmap6 [n][6] (c[i] = b[rowmap[i]], x[i] = c[colmap[i]]) and the
 * factors lu36[n][36]. through_state = 0: factor and substitute in registers; 1: the factors are stored to a
 * device problem record and a second launch reloads them and substitutes (the per-iteration launch forms). */
int ictr_debug_wave_solve(const float *H36, const float *b6, int64_t n, int through_state, float *x6, int *rank,
                          int *nonzero, int *rowmap6, int *colmap6, float *lu36);
/* inspection: the device builds of the f32 exponential / logarithm, one thread per input.
 * log_not_exp = 0: in p[n][6] -> out G[n][12]; 1: in G[n][12] -> out p[n][6] */
int ictr_debug_se3(const float *in, int64_t n, int log_not_exp, float *out);

/* ------------------------------------------------------------------ CamClass (camera.h:19-31, camera.cpp:14-45) */
typedef struct ictr_cam ictr_cam;
int ictr_cam_create(ictr_cam **out, int noscales, const float *fc, const float *cc, const int *wh, int padding);
void ictr_cam_destroy(ictr_cam *cam);
float ictr_cam_getfx(const ictr_cam *cam, int sc);
float ictr_cam_getfy(const ictr_cam *cam, int sc);
float ictr_cam_getcx(const ictr_cam *cam, int sc);
float ictr_cam_getcy(const ictr_cam *cam, int sc);
float ictr_cam_getswo(const ictr_cam *cam, int sc);
float ictr_cam_getsho(const ictr_cam *cam, int sc);
float ictr_cam_getsw(const ictr_cam *cam, int sc);
float ictr_cam_getsh(const ictr_cam *cam, int sc);

/* ------------------------------------------------------------------ utilities.h:84-241 (SE(3) exp / log, host) */
void ictr_se3_coeff_to_group_f(float *G12, const float *p6);
void ictr_se3_coeff_to_group_d(double *G12, const double *p6);
void ictr_se3_group_to_coeff_f(float *p6, const float *G12);
void ictr_se3_group_to_coeff_d(double *p6, const double *G12);
/* Hes.fullPivLu().solve(sumsd), odometer.cpp:509-515 (host copy of the device routine, for callers/tests) */
void ictr_solve6(const float *H36, const float *b6, float *x6);

/* ------------------------------------------------------------------ util_constructpyramide (utilities.cpp:14-52) */
typedef struct ictr_pyramid ictr_pyramid;
/* img: host, row-major f32, w x h. Builds lv_f+1 levels on the device: 2x2 box down-sampling, [-1 0 1]
 * gradients with reflect-101 border, replicate (image) / zero (gradient) padding by `pad` pixels.
 * getgrad: 0 image levels only (a "new" frame); 1 image + gradient planes (the reference's getgrad = true); 2 image
 * levels only, to be used as a REFERENCE frame: the tracker's 8x8 setup kernel forms the gradient patches on the fly
 * from the image plane (same subtraction, same blend, same bits as with the planes) -- a quarter of the memory and of
 * the build's bytes; accepted by trackings with psz 8 and no robustness option (they run the 8x8 per-iteration /
 * resident forms; small problems lose the one-launch tracker), refused with ICTR_ERR_STATE elsewhere. */
int ictr_pyramid_create(ictr_pyramid **out, const float *img, int w, int h, int lv_f, int getgrad, int pad);
/* same, img already in device memory (stays caller-owned; only read during the call) */
int ictr_pyramid_create_device(ictr_pyramid **out, const float *img_dev, int w, int h, int lv_f, int getgrad,
                               int pad, void *hip_stream);
/* Refill an existing pyramid from a new frame of the same size (the per-frame util_constructpyramide of a video loop,
 * run_track_nposes.cpp:180 once per image of a sequence): no allocation, the planes keep their addresses. img_dev: device memory, read by kernels
 * enqueued on hip_stream; img: host memory, copied to a device staging buffer first (has left `img` on return). */
int ictr_pyramid_rebuild_device(ictr_pyramid *pyr, const float *img_dev, void *hip_stream);
int ictr_pyramid_rebuild(ictr_pyramid *pyr, const float *img, void *hip_stream);
/* adopts caller-built host planes (the reference's img_pyr / dx_pyr / dy_pyr arrays); dx/dy may be NULL */
int ictr_pyramid_create_from_host_planes(ictr_pyramid **out, const float **img_pyr, const float **dx_pyr,
                                         const float **dy_pyr, int w, int h, int lv_f, int pad);
void ictr_pyramid_destroy(ictr_pyramid *pyr);
int ictr_pyramid_levels(const ictr_pyramid *pyr);
/* padded plane size of one level */
int ictr_pyramid_level_dims(const ictr_pyramid *pyr, int level, int *sw, int *sh);
/* which: 0 image, 1 dx, 2 dy */
int ictr_pyramid_download(const ictr_pyramid *pyr, int level, int which, float *host_out);
const float *ictr_pyramid_device_plane(const ictr_pyramid *pyr, int level, int which);

/* util_getPatch / util_getPatch_grad (utilities.cpp:55-113, 115-189), batched over K centres.
 * mids: host SoA x[K] then y[K]; outputs host, K*psz*psz each, patch-major. */
int ictr_get_patch(const ictr_pyramid *pyr, int level, const float *mids, int64_t K, int psz, int dopatchnorm,
                   float *out);
int ictr_get_patch_grad(const ictr_pyramid *pyr, int level, const float *mids, int64_t K, int psz, int dopatchnorm,
                        float *out, float *out_dx, float *out_dy);
/* run_track_nposes.cpp:271-355 -- the per-point patch correlation that scores a pose sample, on the device.
 * For each of K points: patches around its position in the backward-most, the reference and the forward-most frame
 * (util_getPatch with mean subtraction, :281), each divided by its norm; corr = max(0, (max(0, <b,r>) w_back +
 * max(0, <r,f>) w_fwd) / (w_back + w_fwd)) with the reference's strict validity tests (:290-305): -1 when the
 * reference position is outside, a term dropped (weight 0) when its frame's position is outside, 0 for NaN.
 * mids: host SoA x_back[K] y_back[K] x_ref[K] y_ref[K] x_fwd[K] y_fwd[K] at `level`; out_corr: K floats. */
int ictr_ncc_score(const ictr_pyramid *pyr_back, const ictr_pyramid *pyr_ref, const ictr_pyramid *pyr_fwd, int level,
                   const float *mids, int64_t K, int psz, float w_back, float w_fwd, float *out_corr);

/* ------------------------------------------------------------------ PoseClass (pose.h:18-40) */
typedef struct ictr_pose ictr_pose;
/* cam and op are held by pointer for the object's lifetime, like the reference (pose.cpp:14-18);
 * run_track_nposes.cpp:281 relies on that aliasing when it flips op.dopatchnorm. */
int ictr_pose_create(ictr_pose **out, const ictr_cam *cam, const ictr_optparam *op);
void ictr_pose_destroy(ictr_pose *pose);
int ictr_pose_setpose_se3(ictr_pose *pose, const double *p_in, const double *meanshift3, double varval);
int ictr_pose_addpose_se3(ictr_pose *pose, const float *dp6);
int ictr_pose_subpose_se3(ictr_pose *pose, const float *dp6);
int ictr_pose_getpose_se3(const ictr_pose *pose, double *p_out6);
/* host SoA buffers with stride op->maxpttrack: pt3d X[M] Y[M] Z[M] -> pt2d x[M] y[M] */
int ictr_pose_project_pt(const ictr_pose *pose, const float *pt3d, float *pt2d, int64_t nopoints, int sc);
int ictr_pose_project_pt_save_rotated(const ictr_pose *pose, const float *pt3d, float *pt3d_rot, float *pt2d,
                                      int64_t nopoints, int sc);
/* current cpos_p[6] / cpos_G[12] (host copies) */
int ictr_pose_get_state(const ictr_pose *pose, float *p6, float *G12);

/* ------------------------------------------------------------------ OdometerClass (odometer.h:21-30) */
typedef struct ictr_odometer ictr_odometer;
int ictr_odometer_create(ictr_odometer **out, ictr_pose *pose, const ictr_optparam *op);
void ictr_odometer_destroy(ictr_odometer *odo);
/* Set3Dpoints (odometer.cpp:171-239). pt_in: host f64 SoA X[n] Y[n] Z[n] (stride nopoints_in).
 * MUTATES pt_in when op->donorm, exactly like the reference (odometer.cpp:207-212). */
int ictr_odometer_set3dpoints(ictr_odometer *odo, double *pt_in, int64_t nopoints_in);
/* SetPose (odometer.cpp:241-255) with device pyramids; both are borrowed until the next SetPose */
int ictr_odometer_setpose(ictr_odometer *odo, const double *p_in, const ictr_pyramid *pyr_ref,
                          const ictr_pyramid *pyr_new);
/* the reference's literal signature: host level-pointer arrays (uploaded on every call: PCIe-bound) */
int ictr_odometer_setpose_host(ictr_odometer *odo, const double *p_in, const float **img_ref,
                               const float **img_ref_dx, const float **img_ref_dy, const float **img_new);
/* TrackPose (odometer.cpp:257-426): coarse-to-fine Gauss-Newton on the device, result in p_out[6] */
int ictr_odometer_trackpose(ictr_odometer *odo, double *p_out);
/* Get2DPoints (odometer.h:30): host SoA x[M] y[M] at level lv_l, valid after SetPose; owned by odo */
const float *ictr_odometer_get2dpoints(ictr_odometer *odo);
/* stream all of this odometer's kernels are enqueued on (hipStream_t); NULL = default stream */
int ictr_odometer_set_stream(ictr_odometer *odo, void *hip_stream);

/* ---- inspection (parity tests, profiling); not part of the reference surface ---- */
typedef struct ictr_trace_rec {
  int level;
  int iter;
  float H[36];
  float b[6];
  float dp[6];
  float p[6];
} ictr_trace_rec;
/* enable before trackpose; records every executed (level, iteration) of problem 0 */
int ictr_odometer_enable_trace(ictr_odometer *odo, int enable);
int ictr_odometer_trace(ictr_odometer *odo, ictr_trace_rec *out, int64_t capacity, int64_t *count);
/* which: 0 pat_ref 1 pat_ref_dx 2 pat_ref_dy (novals*M floats) 4 pt3d 5 pt3d_ref (3*M) 7 sd coefficients (16*M);
 * 100+l: pt2d of level l (2*M). Copies device state to host_out. */
int ictr_odometer_read_buffer(ictr_odometer *odo, int which, float *host_out, int64_t count);
/* normalisation parameters of the last Set3Dpoints */
int ictr_odometer_get_norm(const ictr_odometer *odo, double *meanshift3, double *varval);
/* Launch-form and kernel-selection bits, for cross-checks, tests and measurements (0 = the default; results are the same
 * up to summation order unless noted). Any other bit is refused with ICTR_ERR_INVALID.
 * The default form of a tracking, in this order (see ictr_batch_last_path):
 *   - 8x8 patches, no robustness option, no patch normalisation, problems of >= 8193 points (or >= 500 points with
 *     >= 48 000 in the batch, or a peer exchange set): the resident-iteration form (4) -- per level the setup launch and
 *     ONE launch for all iterations, templates in registers;
 *   - problems of up to 192 8x8 patches' worth of pixels (384 with >= 16 problems), or 8x8 problems of 129..8192 points
 *     in the team form (ictr_batch_set_team): the one-launch tracker (1; 3 when it also carries the begin phase) --
 *     not for sharded batches, with event timing on, or with image-only reference pyramids;
 *   - up to 65 536 points in the batch: the per-iteration launches replayed as one hipGraph (2);
 *   - otherwise the per-iteration launches (0). */
#define ICTR_VARIANT_ANY_SIZE 0x2              /* bit 1: any-size kernels for P = 8 instead of the 8x8 fast path, in
                                                  the per-iteration launches and in the one-launch tracker (one
                                                  workgroup per problem: the team form is an 8x8 form) */
#define ICTR_VARIANT_H_BY_SETUP 0x100          /* bit 8: H reduced by the level's setup tail, not by the first iteration */
#define ICTR_VARIANT_LAUNCHES 0x2000           /* bit 13: per-iteration launches whatever the problem size */
#define ICTR_VARIANT_ONE_LAUNCH 0x4000         /* bit 14: the one-launch tracker wherever its point records fit */
#define ICTR_VARIANT_NO_GRAPH 0x8000           /* bit 15: plain launches instead of the hipGraph replay */
#define ICTR_VARIANT_SEPARATE_BEGIN 0x40000    /* bit 18: the begin phase as separate operations */
#define ICTR_VARIANT_NO_TEAMS 0x80000          /* bit 19: one workgroup per problem in the one-launch tracker */
#define ICTR_VARIANT_NO_RESIDENT 0x200000      /* bit 21: never the resident-iteration form */
#define ICTR_VARIANT_DEBUG_MUTE 0x2000000      /* bit 25: debug, one workgroup of every problem skips its exchange store
                                                  (tests of the time-out path: the tracking FAILS) */
#define ICTR_VARIANT_GRAD_PLANES 0x8000000     /* bit 27: the 8x8 setup kernel reads the gradient planes instead of
                                                  forming the gradients from the image plane (builder-made pyramids;
                                                  bit-identical patches either way) */
#define ICTR_VARIANT_DYNAMIC_LOOP 0x10000000   /* bit 28: the 8x8 setup kernel's dynamic patch loop instead of the
                                                  static 16-patch groups (bit-identical patches) */
#define ICTR_VARIANT_ALL                                                                                            \
  (ICTR_VARIANT_ANY_SIZE | ICTR_VARIANT_H_BY_SETUP | ICTR_VARIANT_LAUNCHES | ICTR_VARIANT_ONE_LAUNCH |              \
   ICTR_VARIANT_NO_GRAPH | ICTR_VARIANT_SEPARATE_BEGIN | ICTR_VARIANT_NO_TEAMS | ICTR_VARIANT_NO_RESIDENT |         \
   ICTR_VARIANT_DEBUG_MUTE | ICTR_VARIANT_GRAD_PLANES | ICTR_VARIANT_DYNAMIC_LOOP)
/* A kernel-form bit of the same word, accepted beside the ICTR_VARIANT_* bits (a family of its own: it selects inside
 * one kernel, not a launch form). Bit 29: the 8x8 setup kernel's static groups read the reference image with direct
 * taps and line touches at every level, never through the per-wave LDS tile (bit-identical patches, sums and poses). */
#define ICTR_REF8_DIRECT_TAPS 0x20000000
#define ICTR_SELECT_ALL (ICTR_VARIANT_ALL | ICTR_REF8_DIRECT_TAPS)
int ictr_odometer_set_variant(ictr_odometer *odo, int variant);
/* one-launch tracker, team form (see ictr_batch_set_team) */
int ictr_odometer_set_team(ictr_odometer *odo, int target_points, int min_points, int max_points);
int ictr_odometer_set_robust(ictr_odometer *odo, int flags, float huber_k); /* see ictr_batch_set_robust */
/* launch form and workgroups per problem of the last TrackPose (see ictr_batch_last_path / ictr_batch_last_team) */
int ictr_odometer_last_path(const ictr_odometer *odo);
int ictr_odometer_last_team(const ictr_odometer *odo);

/* ------------------------------------------------------------------ batched engine (B independent problems) */
typedef struct ictr_batch ictr_batch;
/* All problems share cam and op; each has its own point set (<= op->maxpttrack), pose and frame pair. */
int ictr_batch_create(ictr_batch **out, const ictr_cam *cam, const ictr_optparam *op, int64_t nproblems);
void ictr_batch_destroy(ictr_batch *b);
int ictr_batch_set_stream(ictr_batch *b, void *hip_stream);
int ictr_batch_set3dpoints(ictr_batch *b, int64_t problem, double *pt_in, int64_t nopoints_in);
/* same, with the cloud normalisation supplied by the caller (sharded runs: every rank must use the mean /
 * mean-squared-radius of ALL points, not of its own slice). Ignored unless op->donorm. */
int ictr_batch_set3dpoints_norm(ictr_batch *b, int64_t problem, double *pt_in, int64_t nopoints_in,
                                const double *meanshift3, double varval);
int ictr_batch_get_norm(const ictr_batch *b, int64_t problem, double *meanshift3, double *varval);
int ictr_batch_setpose(ictr_batch *b, int64_t problem, const double *p_in, const ictr_pyramid *pyr_ref,
                       const ictr_pyramid *pyr_new);
/* SetPose of every problem in one call: p_all[6*nproblems], all problems on the same frame pair (pose samples) */
int ictr_batch_setpose_all(ictr_batch *b, const double *p_all, const ictr_pyramid *pyr_ref,
                           const ictr_pyramid *pyr_new);
/* enqueue SetPose's projection + the whole coarse-to-fine loop for every problem; asynchronous */
int ictr_batch_track_async(ictr_batch *b);
/* wait and fetch all poses: p_out[6*nproblems] */
int ictr_batch_get_poses(ictr_batch *b, double *p_out);
/* number of GN iterations each problem executed in the last track, per level summed: iters[nproblems] */
int ictr_batch_get_iterations(ictr_batch *b, int *iters);
int ictr_batch_get2dpoints(ictr_batch *b, int64_t problem, float *host_out /* 2*M */);
int ictr_batch_set_variant(ictr_batch *b, int variant); /* bits: see ictr_odometer_set_variant */
/* One-launch tracker, team form: a problem of min_points < nopoints <= max_points 8x8 patches is shared by several
 * workgroups (at most 64) that all-gather their partial sums inside the launch. target_points > 0: ceil(nopoints /
 * target_points) workgroups, a function of the problem's point count only; 0: automatic (shares of 40-128 points for a
 * lone problem, a batch sized so that its workgroups are resident together; depends on the batch size too); < 0: never.
 * Defaults 0 / 128 / 8192 (environment: ICTR_TEAM_TARGET / ICTR_TEAM_MINPTS / ICTR_TEAM_MAXPTS); tests use small
 * targets to exercise many, ragged and empty shares. Results equal the other launch forms up to summation order. */
int ictr_batch_set_team(ictr_batch *b, int target_points, int min_points, int max_points);
/* Behaviour-changing robustness options, all OFF by default (the default reproduces the reference, quirks included).
 * flags: ICTR_ROBUST_CLEAN  points outside the reference view at a level contribute nothing (the reference reuses
 *                           their stale patches and sd coefficients, odometer.cpp:304);
 *        ICTR_ROBUST_COMPOSE left-compositional update G <- exp(dp) G instead of p += dp (pose.cpp:118-123); a step of
 *                           exactly zero leaves p as it is;
 *        ICTR_ROBUST_HUBER  residuals weighted min(1, huber_k / |r|) in J^T r (H stays the precomputed one).
 * With any flag set the 8x8 fast path is bypassed (any-size kernels). Oracle: oracle/np_oracle.py (same options). */
#define ICTR_ROBUST_CLEAN 1
#define ICTR_ROBUST_COMPOSE 2
#define ICTR_ROBUST_HUBER 4
int ictr_batch_set_robust(ictr_batch *b, int flags, float huber_k);
/* inspection, like ictr_odometer_read_buffer; additionally which = 8: the problem's device state as floats */
int ictr_batch_read_buffer(ictr_batch *b, int64_t problem, int which, float *host_out, int64_t count);
/* HIP-event timing on the batch's own stream: when enabled, ictr_batch_track_async brackets, per level, the
 * setup kernel (steps 4-6) and the block of maxiter iteration launches (steps 7-10) with events.
 * After the track has completed: ms_setup[l], ms_iters[l] for l in 0..lv_f (0 for levels not run). */
int ictr_batch_set_timing(ictr_batch *b, int enable);
int ictr_batch_get_level_times(ictr_batch *b, float *ms_setup, float *ms_iters);
/* ms_kernel[l]: summed duration of the level's maxiter accumulate-kernel launches ALONE (events around each launch,
 * excluding the tail kernels and the gaps) -- the figure comparable with rocprofv3 --kernel-trace --stats */
int ictr_batch_get_kernel_times(ictr_batch *b, float *ms_kernel);
/* ms per level of the level's FIRST accumulate launch alone (8x8 fast path: the instantiation that also sums H) */
int ictr_batch_get_first_iter_times(ictr_batch *b, float *ms_first);
/* For callers that run several engines concurrently on different streams: ictr_timebase_mark() sets a process-wide
 * time base (synchronises the device); ictr_batch_get_kernel_intervals returns, for the last completed tracking,
 * start and end of every accumulate launch in ms since that base, indexed [level * max(1, maxiter) + iteration]
 * (0, 0 for launches that did not run). Overlapping intervals of different engines = launches that shared the GPU. */
int ictr_timebase_mark(void);
int ictr_batch_get_kernel_intervals(ictr_batch *b, float *start_ms, float *end_ms);
int ictr_batch_get_setup_intervals(ictr_batch *b, float *start_ms, float *end_ms); /* [level]: the setup launches */
/* which launch form the last tracking used: 0 = per-iteration launches (plain), 1 = the one-launch tracker (whole
 * odometer.cpp:257-426 loop in one kernel; one workgroup or a team of workgroups per problem, see ictr_batch_last_team),
 * 2 = per-iteration launches replayed as one hipGraph, 3 = the one-launch tracker with the begin phase and the state
 * read-back inside the launch, 4 = the resident-iteration form (one setup launch + one k_level_resident launch per
 * level: dense problems of >= 8193 8x8 patches) */
int ictr_batch_last_path(const ictr_batch *b);
/* workgroups per problem of that launch when it was the one-launch tracker (1 otherwise): problems of a few hundred to a
 * few thousand 8x8 patches are shared by a team of workgroups that all-gather their partial sums inside the launch */
int ictr_batch_last_team(const ictr_batch *b);

/* ---- distributed (points sharded over ranks): split phases so the caller can all-reduce ----
 * The normal-equation block lives in a caller-visible device buffer: per problem 21 floats of H
 * (upper triangle, row-major) + 6 floats of b  => red[nproblems][27]. With sharding enabled the
 * accumulate kernels leave rank-local sums there and the *_finish kernels consume the reduced values. */
int ictr_batch_enable_sharding(ictr_batch *b, int enable);
float *ictr_batch_reduction_buffer(ictr_batch *b); /* device pointer, nproblems*27 floats */
/* use a caller-owned device buffer (e.g. a torch tensor handed to torch.distributed) instead; NULL = internal */
int ictr_batch_set_reduction_buffer(ictr_batch *b, float *dev_ptr);
int ictr_batch_begin(ictr_batch *b);                  /* SetPose projection, all problems */
/* 1 if the caller must all-reduce red[] between level_accumulate and level_finish; 0 on the 8x8 fast path, where H
 * is accumulated by the level's first iteration launch and travels with that iteration's b (27 floats, one message) */
int ictr_batch_level_allreduce_needed(ictr_batch *b);
int ictr_batch_level_accumulate(ictr_batch *b, int level);  /* steps 4-6 -> local H in red[] (unless deferred) */
int ictr_batch_level_finish(ictr_batch *b, int level);      /* adopt (reduced) H, reset iteration state */
int ictr_batch_iter_accumulate(ictr_batch *b, int level);   /* steps 7-9a -> local b in red[] */
int ictr_batch_iter_finish(ictr_batch *b, int level);       /* steps 9b-10 on the (reduced) b */

/* ------------------------------------------------------------------ Python flow-tracking surface on the device
 * misc_src/classoftrack.py:4-34 func_get_transf_position: K points (x, y) moved by a displacement field sampled
 * bilinearly at the points; float64 arithmetic in NumPy's operation order (bit-identical to the NumPy restatement and
 * to the goldens generated from the reference); NaN for points whose four taps are not all inside the field.
 * disp_u / disp_v: (H, W) planes, float32 (is_f64 = 0) or float64, host or device pointers (fields_on_device);
 * disp_v may be NULL (x only). xy and out: host (K, 2) float64. */
int ictr_flow_gather(const void *disp_u, const void *disp_v, int is_f64, int fields_on_device, int H, int W,
                     const double *xy, int64_t K, double *out);
/* misc_src/func_OF_util.py:87-129 func_extract_bil_patch, batched and without the post-processing options: K raw
 * bilinear patches (side x side x C, side = 2 (pz / 2): Python-2 integer division) of a host (H, W, C) float64 image
 * around host points (K, 2) float64; out: host (K, side, side, C) float64. Windows must lie inside the image. */
int ictr_extract_bil_patches(const double *img, int H, int W, int C, const double *pts, int64_t K, int pz, double *out);

/* ---- one-shot peer-to-peer all-reduce of the reduction buffer (latency-optimal on point-to-point xGMI) ----
 * Each rank stores its nproblems*27 floats straight into a mailbox slot in every peer's device memory (mapped with
 * hipIpc) and adds the world slots of its own mailbox in rank order: one hop instead of a ring's 2(N-1), one small
 * kernel on the compute stream, identical bits on every rank. Set-up: create -> exchange the local handles through any
 * host channel (torch.distributed all_gather) -> connect. See csrc/ictr_p2p.hip for the protocol. */
typedef struct ictr_p2p ictr_p2p;
int ictr_p2p_create(ictr_p2p **out, int rank, int world, int64_t count /* floats per exchange */);
int ictr_p2p_handle_bytes(void);                                  /* sizeof(hipIpcMemHandle_t) */
int ictr_p2p_local_handle(ictr_p2p *p, void *handle_out);          /* this rank's mailbox handle */
int ictr_p2p_connect(ictr_p2p *p, const void *all_handles);        /* world handles, rank order */
int ictr_p2p_allreduce(ictr_p2p *p, float *dev_buf, int64_t count, void *hip_stream); /* in place, asynchronous */
int ictr_p2p_error(ictr_p2p *p); /* 1 if an exchange timed out (a peer never arrived); synchronises the device */
void ictr_p2p_destroy(ictr_p2p *p);
/* Sharded RESIDENT form (r03): the batch holds this rank's shard of every problem's points, and its resident-iteration
 * launches (one per level, all iterations inside) add H -- once per level -- and b -- once per iteration -- over the ranks
 * THEMSELVES: a frame pair's solver workgroup writes its sums into every rank's mailbox and polls its own (the protocol
 * above, inside the launch: no kernel boundary, no host call, no communicator between two iterations). p: a connected
 * ictr_p2p with count >= 64 * nproblems, created alike on every rank; NULL switches the exchange off again. Every rank
 * must run the same trackings (same problems, levels, iteration limits); their loop decisions stay in lockstep because
 * every rank solves on identical sums. A tracking that cannot run in the resident form (see ictr_odometer_set_variant)
 * fails with ICTR_ERR_STATE instead of running unsynchronised; a peer that never arrives ends the launch after
 * ICTR_TEAM_TIMEOUT_S and the wait returns ICTR_ERR_HIP. */
int ictr_batch_set_peer_exchange(ictr_batch *b, ictr_p2p *p);

/* ------------------------------------------------------------------ flow producer for the misc_src/run_*OF* drivers
 * Those drivers shell out to an external optical-flow binary that is not in the reference repository
 * (misc_src/run_test_OF_track.py:90-108). ictr_patchflow is the in-tree replacement: K independent psz x psz patches
 * (psz <= 32), each with its own 2-parameter translation, pyramidal inverse-compositional Lucas-Kanade with
 * util_getPatch's sampling convention; one wave64 per patch runs every level and iteration inside one launch.
 * pts: host SoA x[K] y[K] at level 0 in frame A; out: host SoA positions in frame B (NaN when lost);
 * status (optional) 1/0; iters (optional) executed iterations. Build-defined algorithm: no reference pins it. */
int ictr_patchflow(const ictr_pyramid *pyr_a, const ictr_pyramid *pyr_b, const float *pts, int64_t K, int psz, int lv_f,
                   int lv_l, int maxiter, float eps, float *out, int *status, int *iters);
/* duration in ms of the k_patchflow launch of this thread's last ictr_patchflow call (HIP events), < 0 if unknown */
float ictr_patchflow_last_kernel_ms(void);
/* kernel form of this thread's last k_patchflow launch (ictr_patchflow or a flow grid): pixels per lane * 10 + waves per
 * patch, one of 11, 41, 161, 82; 0 before the first launch. ICTR_PF_WPP=1 / 2 (read once per process) forces one / two
 * waves per patch; unset, patches of more than 256 pixels take two. */
int ictr_patchflow_last_form(void);

/* The disparity of a rectified stereo pair: the same patches, layouts, refusals and pyramid walk as ictr_patchflow with
 * ONE parameter per patch. The patch moves along x only (p += sum Gx (T - I) / sum Gx^2), y never moves and comes back
 * with its input bits. A patch is lost iff its gradients vanish or sum Gx^2 <= 0.01 (sum Gx^2 + sum Gy^2): horizontal
 * edges alone carry no disparity; vertical edges alone, which the 2-D call refuses, are kept. psz 1..32 (psz 1 is a
 * legal 1-D patch). K = 0 is accepted. Build-defined: the statement of record is tests/patchdisp_np.py. */
int ictr_patchdisp(const ictr_pyramid *pyr_a, const ictr_pyramid *pyr_b, const float *pts, int64_t K, int psz, int lv_f,
                   int lv_l, int maxiter, float eps, float *out, int *status, int *iters);
/* duration in ms of the k_patchdisp launch of this thread's last ictr_patchdisp call (HIP events), < 0 if unknown */
float ictr_patchdisp_last_kernel_ms(void);
/* kernel form of this thread's last k_patchdisp launch (ictr_patchdisp or ictr_flowgrid_compute_x): pixels per lane * 10
 * + waves per patch, one of 11, 41, 82, chosen by the patch size alone; 0 before the first launch */
int ictr_patchdisp_last_form(void);

/* ------------------------------------------------------------------ full-frame parametric alignment (extension)
 * Inverse-compositional Gauss-Newton alignment of a whole template region under one parametric warp:
 * model 0 translation (2), 1 SE(2) (3), 2 affine (6), 3 homography (8). These are the warp models BASELINE.json's
 * configs 1, 2, 3 and 5 name; the reference itself has no such warp (its only warp is the SE(3) reprojection of
 * 3-D points, odometer.cpp:193-300), so this engine is build-defined: same Gauss-Newton skeleton (template
 * gradients + Hessian once per level, residual + J^T r per iteration, coarse-to-fine), Baker-Matthews update
 * M <- M * W(dp)^-1; oracle = oracle/np_icgn.py. nproblems independent frame pairs run in every launch.
 * Warps cross the boundary as row-major 3x3 matrices in level-0 pixel coordinates (template pixel -> current pixel). */
typedef struct ictr_icgn ictr_icgn;
#define ICTR_WARP_TRANSLATION 0
#define ICTR_WARP_SE2 1
#define ICTR_WARP_AFFINE 2
#define ICTR_WARP_HOMOGRAPHY 3
/* region_xywh: template rectangle at level 0, NULL = the frame minus a 2-pixel rim; eps: stop when |dp| <= eps */
int ictr_icgn_create(ictr_icgn **out, int model, int w, int h, int lv_f, int lv_l, int maxiter, float eps,
                     const int *region_xywh, int64_t nproblems);
void ictr_icgn_destroy(ictr_icgn *g);
int ictr_icgn_set_stream(ictr_icgn *g, void *hip_stream);
/* pyramids: lv_f+1 levels, gradients on the template, padding >= 2; borrowed, must outlive the run */
int ictr_icgn_set_frames(ictr_icgn *g, int64_t problem, const ictr_pyramid *tmpl, const ictr_pyramid *cur);
int ictr_icgn_set_warp(ictr_icgn *g, int64_t problem, const double *M9); /* initial warp, NULL = identity */
int ictr_icgn_set_timing(ictr_icgn *g, int enable);
int ictr_icgn_run_async(ictr_icgn *g); /* all levels, all iterations, no host synchronisation */
/* M9_out: nproblems*9; iters: nproblems; last_dp: nproblems*8 (any may be NULL). Synchronises the stream. */
int ictr_icgn_get_results(ictr_icgn *g, double *M9_out, int *iters, float *last_dp);
int ictr_icgn_get_kernel_times(ictr_icgn *g, float *ms_per_level); /* summed k_icgn_iter time per level */
/* row-band sharding (BASELINE config 5): each rank owns template rows [row_lo, row_hi) at level 0 and all-reduces
 * the 44-float record per problem (36 upper-triangle H + 8 b) between the accumulate and finish phases. */
int ictr_icgn_set_rows(ictr_icgn *g, int row_lo, int row_hi);
int ictr_icgn_enable_sharding(ictr_icgn *g, int enable, float *red_dev /* nproblems*44 floats or NULL */);
int ictr_icgn_begin(ictr_icgn *g);
int ictr_icgn_hess_accumulate(ictr_icgn *g, int level);
int ictr_icgn_hess_finish(ictr_icgn *g, int level);
int ictr_icgn_iter_accumulate(ictr_icgn *g, int level);
int ictr_icgn_iter_finish(ictr_icgn *g, int level);

/* ------------------------------------------------------------------ frame-to-frame sequence (run_odometer_test.m:172-250)
 * Tracks frame t -> t+1 for every t of a video, each pair from the pose just found for frame t, with the step between
 * two pairs on the device: no host synchronisation and no copy between pairs, one read-back at the end.
 * Per pair t -> t+1, with p_t the tracked pose of frame t (p_0 given):
 *   1. cull: every world point X projected at level 0 in f64, Xc = G(p_t) X (se3_exp<double>),
 *      u = fx Xc / Zc + cx, v = fy Yc / Zc + cy; kept iff 1 <= u <= w and 1 <= v <= h (the script's bounds literally,
 *      w, h the camera's unpadded size; NO depth test, as in the script);
 *   2. subsample: the survivors of ranks 0, s, 2s, ... in world-index order, then Set3Dpoints' cap: the first
 *      min(count, maxpttrack). The script passes the selected count itself as maxpttrack; here the cap is fixed at
 *      creation, and npts == cap in the output shows where it bit;
 *   3. Set3Dpoints (f64 meanshift / varval, patch and coefficient state reset), SetPose(p_t, pyr_t, pyr_t+1),
 *      TrackPose -> p_t+1, as a fresh run_io_reprojection_test process would;
 *   4. no point selected (deviation: the reference would divide by zero): p_t+1 = p_t, npts = iters = 0, continue.
 * The launch form follows the cap: the team form where it serves the cap (psz 8), otherwise one workgroup per tracking
 * (at most 2048 points); a cap neither serves is refused by ictr_sequence_create. nworld: 1 .. 2^24, stride >= 1. */
typedef struct ictr_sequence ictr_sequence;
int ictr_sequence_create(ictr_sequence **out, const ictr_cam *cam, const ictr_optparam *op, int64_t nworld, int stride);
void ictr_sequence_destroy(ictr_sequence *s);
/* The setters below are refused (ICTR_ERR_STATE) while a run is in flight: call ictr_sequence_wait first.
 * world points, f64 SoA X[nworld] Y[nworld] Z[nworld]; copied to the device once (never modified) */
int ictr_sequence_set_points(ictr_sequence *s, const double *pt3d);
/* frames [N][h][w] f32 of the camera's unpadded size (w, h are checked against it), N >= 2. Host frames are copied to
 * the device once; on_device frames are borrowed until ictr_sequence_wait. */
int ictr_sequence_set_frames(ictr_sequence *s, const float *frames, int64_t nframes, int w, int h, int on_device);
int ictr_sequence_set_stream(ictr_sequence *s, void *hip_stream);
/* a sequence runs the plain one-launch forms only: any robustness flag is refused (ICTR_ERR_INVALID) */
int ictr_sequence_set_robust(ictr_sequence *s, int flags, float huber_k);
/* enqueues the whole sequence from p0 (6 f64) and returns */
int ictr_sequence_track_async(ictr_sequence *s, const double *p0);
/* waits for the last run: poses [N][6] (poses[0] = p0), npts / iters [N-1] per pair (any may be NULL) */
int ictr_sequence_wait(ictr_sequence *s, double *poses, int32_t *npts, int32_t *iters);
/* inspection, after wait: per pair an order-aware 64-bit hash of the selected world indices,
 * sum over k < npts of splitmix64((k << 32) | index_k) modulo 2^64 */
int ictr_sequence_selection_hashes(const ictr_sequence *s, uint64_t *out);
/* inspection, after wait (ICTR_ERR_STATE without a completed run): what the LAST pair's selection left on the device.
 * npts; sel[0 .. npts) the selected world indices in order (room for maxpttrack entries, the rest is not written);
 * ms3 / varval the f64 normalisation of the selected points (0, 0, 0 and 1 without donorm); pt3d the engine's
 * normalised f32 points, SoA X[M] Y[M] Z[M] with M = maxpttrack, zero behind npts. Neither the tracking nor the last
 * frame's bookkeeping writes any of them. Any output may be NULL. Synchronous copies; no kernel runs. */
int ictr_sequence_last_selection(const ictr_sequence *s, int32_t *npts, int32_t *sel, double *ms3, double *varval,
                                 float *pt3d);
/* workgroups per tracking launch of the last run (before the first run: the form the cap selects):
 * 1 = the single-workgroup form, > 1 = the team form */
int ictr_sequence_last_team(const ictr_sequence *s);

/* ------------------------------------------------------------------ RANSAC pose sampling (func_ransac_fitcameras_odom.m:17-87)
 * From N 2-D/3-D matches, pose samples as the script draws them, with these deviations:
 *   - trial t (0-based) draws from a counter-based stream, u_k = mix(mix(seed) ^ ((t << 32) | k)), k = 0, 1, ...,
 *     mix = splitmix64; index ((u_k >> 32) * N) >> 32; repeats skipped; the first 4 distinct indices in draw order.
 *     Not reproducible against MATLAB's randsample; every run is bit-reproducible.
 *   - 2-D points are undistorted for the solver with one radial coefficient kc (x_d = x_n (1 + kc |x_n|^2), 20
 *     fixed-point steps); the same model distorts the reprojections. kc = 0: the plain pinhole.
 *   - degenfn_P literally (|dot(cross(p1, p2), p3)| < 2^-52 over every triple, 3-D points and homogeneous undistorted
 *     2-D points), then P3P (Lambda Twist) on the first three matches; of its solutions the one that reprojects the
 *     fourth match nearest (first on ties). None: the trial fails.
 *   - a match is an inlier when |reproj(R (X - t)) - pt2d| <= inlthresh (f64, no depth test); a trial succeeds with
 *     >= 4 inliers. The first nsamples successes among trials 0 .. maxtrials-1 are accepted.
 *   - post-filter: inl_cnt[j] = accepted samples that have match j as an inlier; sample s is dropped when s < N and
 *     inl_cnt[s] <= 4 (the script's logical index over matches applied to samples); inl_cnt loses its entries <= 4.
 * Inputs N: 4 .. 2^24, max_samples: 1 .. 2^24. */
typedef struct ictr_ransac ictr_ransac;
int ictr_ransac_create(ictr_ransac **out, int64_t n, int64_t max_samples);
void ictr_ransac_destroy(ictr_ransac *r);
/* pt2d f64 SoA x[N] y[N] (pixels, distorted), pt3d f64 SoA X[N] Y[N] Z[N]; refused (ICTR_ERR_STATE) while a run is in
 * flight */
int ictr_ransac_set_points(ictr_ransac *r, const double *pt2d, const double *pt3d);
/* enqueues the trials on hip_stream (NULL: the null stream) and returns; fc, cc: 2 f64 each. nsamples: 1 .. max_samples,
 * maxtrials: 1 .. 2^40, inlthresh finite. Runs of more than 64 chunks read a 4-byte flag between groups of 64 chunks
 * (a host wait) and stop enqueueing once the samples are found. */
int ictr_ransac_run(ictr_ransac *r, const double *fc, const double *cc, double kc, int64_t nsamples, int64_t maxtrials,
                    double inlthresh, uint64_t seed, void *hip_stream);
/* waits for the last run. counts[4]: samples after the post-filter (S), accepted samples before it, trials the script
 * would have used, entries of the filtered inl_cnt. Per kept sample (any pointer may be NULL): R [S][9] row-major,
 * camera centre t [S][3], p = se3_log([R | -R t]) [S][6], inlier bits [S][ceil(N / 64)] (bit j % 64 of word j / 64 =
 * match j); inl_cnt [counts[3]] (at most N entries). */
int ictr_ransac_wait(ictr_ransac *r, int64_t *counts, double *R, double *t, double *p, uint64_t *inl_words,
                     int32_t *inl_cnt);
/* inspection, after wait: per kept sample its trial index and its 4 drawn match indices (draw order) */
int ictr_ransac_samples(const ictr_ransac *r, int64_t *trial, int32_t *draws);
/* trials per chunk of this object (ICTR_RANSAC_CHUNK overrides the choice made from N) */
int ictr_ransac_chunk_size(const ictr_ransac *r);
/* inspection: k_ransac_hyp and k_ransac_score<tile> alone over trials first_trial .. first_trial + count - 1 (count:
 * 1 .. 2^20, trials below 2^40), in the object's own chunks and tile, on the null stream; no selection, so every trial
 * of the range is computed whatever came before it. Needs set_points; refused (ICTR_ERR_STATE) while a run is in
 * flight. Per trial (host arrays): status[count] (1 = not degenerate and a P3P root chosen), draws[count][4] (draw
 * order, -1 = not drawn), hyp[count][12] (R row-major, then the camera centre), cnt[count] inliers,
 * words[count][ceil(N / 64)] inlier bits. hyp, cnt and words of a trial with status 0 are undefined. */
int ictr_debug_ransac_trials(ictr_ransac *r, const double *fc, const double *cc, double kc, double inlthresh,
                             uint64_t seed, int64_t first_trial, int64_t count, int32_t *status, int32_t *draws,
                             double *hyp, uint32_t *cnt, uint64_t *words);

/* ------------------------------------------------------------------ static split (misc_src/run_test_OF_track.py:309-343)
 * "Divide points in static and dynamic using the fundamental matrix": RANSAC over 8-point fundamental matrices of P view
 * pairs of the same N points (DESIGN.md §4 "Static split"):
 *   - trial t (0-based) draws 8 distinct point indices from the counter-based stream of the pose sampling above
 *     (u_k = mix(mix(seed) ^ ((t << 32) | k)), index ((u_k >> 32) N) >> 32, repeats skipped, at most 1024 draws); the
 *     same 8 serve every pair;
 *   - per (trial, pair) the fundamental matrix F, xb^T F xa = 0, of the 8 correspondences: Hartley normalisation, null
 *     vector of the 8x9 design matrix by Gaussian elimination with full pivoting, rank 2 by a one-sided Jacobi SVD,
 *     denormalisation, unit Frobenius norm; all f64 in a fixed order. A fit fails (F = NaN) when a mean distance is 0, a
 *     pivot is exactly 0 or an entry of F is not finite; a trial with a failed fit has no inliers;
 *   - per point and pair the distance of xb to the line F xa (func_F_transfer_points), per point the maximum over the
 *     pairs (a NaN stays); inlier iff that maximum < thresh;
 *   - the trial with the most inliers wins, the lowest trial on ties; no inlier anywhere is a normal result
 *     (best_count 0, best_trial the lowest trial).
 * Inputs N: 8 .. 2^22, npairs: 1 .. 64, ntrials: 1 .. 2^20. Coordinates that are not finite are admitted: such a point
 * is never an inlier, and a trial that draws it fails. */
typedef struct ictr_fsplit ictr_fsplit;
int ictr_fsplit_create(ictr_fsplit **out, int64_t n, int64_t npairs);
void ictr_fsplit_destroy(ictr_fsplit *r);
/* xy: f64 [npairs][4][N], per pair the rows xa, ya, xb, yb; refused (ICTR_ERR_STATE) while a run is in flight */
int ictr_fsplit_set_pairs(ictr_fsplit *r, const double *xy);
/* enqueues the trials on hip_stream (NULL: the null stream) and returns; thresh must not be NaN */
int ictr_fsplit_run(ictr_fsplit *r, int64_t ntrials, double thresh, uint64_t seed, void *hip_stream);
/* waits for the last run; any output may be NULL. draws[8]: the winner's point indices (draw order, -1 = not drawn),
 * F [npairs][9] row-major (nine NaN where a fit failed), inl_words [ceil(N / 64)] (bit j % 64 of word j / 64 = point
 * j), dd [N]: every point's largest distance under the winner. */
int ictr_fsplit_wait(ictr_fsplit *r, int64_t *best_trial, int64_t *best_count, int32_t *draws, double *F,
                     uint64_t *inl_words, double *dd);
/* on: the next runs record device time stamps between their stages; get: ms[4] of the last waited run spent in
 * k_fsplit_fit, k_fsplit_score, k_fsplit_select (summed over the chunks) and k_fsplit_mask */
int ictr_fsplit_set_timing(ictr_fsplit *r, int on);
int ictr_fsplit_get_kernel_times(const ictr_fsplit *r, float *ms);
/* inspection: k_fsplit_fit and k_fsplit_score<tile> alone over trials first_trial .. first_trial + count - 1 (within
 * 0 .. 2^20), through the launch helper of the run, in the object's own chunks (ICTR_FSPLIT_CHUNK, default 4096
 * trials) and tile (ICTR_FSPLIT_TILE = 16 / 32 / 64, default 32), on the null stream. Per trial (host arrays):
 * status[count] (1 = every pair's fit succeeded), draws[count][8], F[count][npairs][9], cnt[count] inliers (0 for a
 * trial with status 0). */
int ictr_debug_fsplit_trials(ictr_fsplit *r, double thresh, uint64_t seed, int64_t first_trial, int64_t count,
                             int32_t *status, int32_t *draws, double *F, uint32_t *cnt);

/* ------------------------------------------------------------------ camera fit (misc_src/run_test_OF_track.py:374-411)
 * "Fit cameras": one pose per frame of a track window, each by Levenberg-Marquardt on the mean squared reprojection
 * residual of the same N points (DESIGN.md §4 "Camera fit"); nframes independent fits run side by side:
 *   - x_cam = R X + t, pinhole fc, cc without distortion; an observation counts in a frame iff its mask bit is set and
 *     its three point and two pixel coordinates are finite (no depth test); c = sum(rx^2 + ry^2) / n;
 *   - per pass H (21), b (6), s summed in an order that is a function of N alone (csrc/ictr_camfit_hd.h);
 *     (H + damp diag(H)) d = b by LDL^T without pivoting; the pose moves by the Cayley retraction of d;
 *   - schedule of triang.c:327 (noiter 20, damp_init 2, damp_fct 10, minres 1e-5, maxdamp 1e10): a trial pose is
 *     accepted iff its cost is finite and smaller; stops, tested in this order: cost <= minres or an accepted improvement
 *     <= minres (converged), noiter iterations, damp >= maxdamp.
 * All f64 in a fixed order: the same bits on every run. N: 1 .. 2^22, nframes: 1 .. 4096, noiter: 0 .. 1000. */
#define ICTR_CAMFIT_CONVERGED 0
#define ICTR_CAMFIT_NOITER 1
#define ICTR_CAMFIT_MAXDAMP 2
#define ICTR_CAMFIT_FEW_OBS 3          /* fewer than 3 counted observations: G = G0 */
#define ICTR_CAMFIT_START_NOT_FINITE 4 /* the cost at G0 is not finite: G = G0 */
typedef struct ictr_camfit ictr_camfit;
int ictr_camfit_create(ictr_camfit **out, int64_t n, int64_t nframes);
void ictr_camfit_destroy(ictr_camfit *r);
/* X: f64 [3][N]; xy: f64 [nframes][2][N] (pixels); words: the inlier words of ictr_fsplit_wait (bit j % 64 of word j / 64
 * = point j), NULL: every point; fc[2] (finite, not 0), cc[2]. All refused (ICTR_ERR_STATE) while a run is in flight. */
int ictr_camfit_set_points(ictr_camfit *r, const double *X);
int ictr_camfit_set_observations(ictr_camfit *r, const double *xy);
int ictr_camfit_set_mask(ictr_camfit *r, const uint64_t *words);
int ictr_camfit_set_camera(ictr_camfit *r, const double *fc, const double *cc);
/* enqueues 2 + 2 noiter launches on hip_stream (NULL: the null stream) and returns. G0 [nframes][12]: row-major [R | t]
 * start poses (finite). Needs damp_init > 0, damp_fct > 1, minres >= 0, all finite, and maxdamp > 0. */
int ictr_camfit_run(ictr_camfit *r, const double *G0, int32_t noiter, double damp_init, double damp_fct, double minres,
                    double maxdamp, void *hip_stream);
/* waits for the last run; any output may be NULL. Per frame: G [12], cost, damp, iters (solves tried), status
 * (ICTR_CAMFIT_*), n (counted observations). */
int ictr_camfit_wait(ictr_camfit *r, double *G, double *cost, double *damp, int32_t *iters, int32_t *status, int64_t *n);
/* per frame the mean of sqrt(rx^2 + ry^2) over the counted observations at the poses G [nframes][12], with dt[3] (NULL:
 * zero) added to every translation, and their number n (may be NULL); NaN where n is 0. Synchronous, null stream. */
int ictr_camfit_reproj(ictr_camfit *r, const double *G, const double *dt, double *mean_err, int64_t *n);
/* on: the next runs record device time stamps around their launches; get: ms[2] of the last waited run spent in
 * k_camfit_pass and k_camfit_step */
int ictr_camfit_set_timing(ictr_camfit *r, int on);
int ictr_camfit_get_kernel_times(const ictr_camfit *r, float *ms);
/* inspection: k_camfit_pass at the poses G [nframes][12] and the ordered sum of k_camfit_step alone, on the null stream.
 * Per frame: n, s, H [21] (upper triangle, row-major), b [6]. */
int ictr_debug_camfit_pass(ictr_camfit *r, const double *G, int64_t *n, double *s, double *H, double *b);

/* ------------------------------------------------------------------ window bundle adjustment (run_test_OF_track.py, TODO 3)
 * "BA Adjust cameras and static points": the poses of frames 1 .. F - 1 and the adjusted points of a track window moved
 * together by Levenberg-Marquardt on the reprojection residuals of nsides = 1 or 2 cameras per frame (DESIGN.md §4 "Window
 * bundle adjustment"):
 *   - side s of frame f sees x_cam = R_f X + t_f + o_s, o_0 = 0, o_1 = the offset; a point is adjusted iff its mask bit
 *     is set and its 3 coordinates and all its 2 S F observation coordinates are finite; any other point adds exact zeros
 *     and comes back unchanged; c = sum(rx^2 + ry^2) / (n S F) over the n adjusted points; frame 0 keeps its start pose;
 *   - one step: the damped normal equations through the Schur complement of the points, a 3 x 3 LDL^T per point and a
 *     dense 6 (F - 1) LDL^T for the cameras, both without pivoting, every sum over points in the order of
 *     csrc/ictr_camfit_hd.h (csrc/ictr_ba_hd.h); a pivot that is not finite or not > 0 fails the solve;
 *   - the schedule, the accept test, the stops and the status codes of the camera fit (ICTR_CAMFIT_*); status 3: fewer
 *     than 3 adjusted points; a failed solve raises the damping, counts an iteration and is tried again.
 * All f64 in a fixed order: the same bits on every run. N: 8 .. 2^22, nframes: 2 .. 32, nsides: 1 or 2, noiter: 0 .. 1000. */
typedef struct ictr_ba ictr_ba;
int ictr_ba_create(ictr_ba **out, int64_t n, int64_t nframes, int64_t nsides);
void ictr_ba_destroy(ictr_ba *r);
/* X: f64 [3][N]; xy: f64 [nsides][nframes][2][N] (pixels); words, fc, cc as ictr_camfit_*; offset[3] finite (needed with
 * two sides). All refused (ICTR_ERR_STATE) while a run is in flight. */
int ictr_ba_set_points(ictr_ba *r, const double *X);
int ictr_ba_set_observations(ictr_ba *r, const double *xy);
int ictr_ba_set_mask(ictr_ba *r, const uint64_t *words);
int ictr_ba_set_camera(ictr_ba *r, const double *fc, const double *cc);
int ictr_ba_set_offset(ictr_ba *r, const double *offset);
/* enqueues 2 + 7 (noiter + 1) launches on hip_stream (NULL: the null stream) and returns. G0 [nframes][12]: the start
 * poses (finite); the schedule as ictr_camfit_run. */
int ictr_ba_run(ictr_ba *r, const double *G0, int32_t noiter, double damp_init, double damp_fct, double minres,
                double maxdamp, void *hip_stream);
/* waits for the last run; any output may be NULL. G [nframes][12], X [3][N] (24 bytes per point, copied only when asked
 * for), cost, damp, iters, status (ICTR_CAMFIT_*), n (adjusted points). */
int ictr_ba_wait(ictr_ba *r, double *G, double *X, double *cost, double *damp, int32_t *iters, int32_t *status, int64_t *n);
/* on: the next runs record device time stamps around their launches; get: ms[7] of the last waited run spent in
 * k_ba_point, k_ba_frames, k_ba_decide, k_ba_schur, k_ba_gather, k_ba_solve, k_ba_back */
int ictr_ba_set_timing(ictr_ba *r, int on);
int ictr_ba_get_kernel_times(const ictr_ba *r, float *ms);
/* inspection: the passes, the Schur pass and the assembly alone at the poses G [nframes][12], the points X [3][N] (NULL:
 * the set ones) and the damping damp, on the null stream. n, cost, A [dim (dim + 1) / 2] the reduced system's upper
 * triangle (row-major, packed, dim = 6 (nframes - 1)), rhs [dim], V [6][N], gp [3][N], nfail: the adjusted points whose
 * 3 x 3 factorisation failed. */
int ictr_debug_ba_system(ictr_ba *r, const double *G, const double *X, double damp, int64_t *n, double *cost, double *A,
                         double *rhs, double *V, double *gp, int64_t *nfail);

/* ------------------------------------------------------------------ multi-view point triangulation (misc_src/triang.c)
 * A track set (10^4 .. 10^5 points, 2 .. 30 views each) triangulated in one launch, one lane per point, with the
 * arithmetic of the reference routine of each mode: every product and sum in f32, in its order and grouping, so the
 * results carry the bits of the reference binary built without contraction (DESIGN.md §4 "Triangulation").
 *   DLT    triangulate_DLT: normal equations of the rows x P2 - P0, y P2 - P1; cov = inverse of A^T A
 *   GN     triangulate_full3D: Gauss-Newton on the reprojection error; cov = (J^T J)^-1 of the last iteration
 *   LM     triangulate_full3D_LM: Levenberg-Marquardt, diagonal damping; cov = the last damped inverse
 *   DEPTH  triangulate_depthonly: Gauss-Newton on the depth along a ray from a centre; cov[0] = 1 / sum j^2
 * The reference prints a line per iteration; here the count comes back per point. */
#define ICTR_TRIANG_DLT 0
#define ICTR_TRIANG_GN 1
#define ICTR_TRIANG_LM 2
#define ICTR_TRIANG_DEPTH 3
/* status word of a point (it changes no value) */
#define ICTR_TRIANG_NONFINITE 1 /* bit 0: a non-finite word in the point or its covariance */
#define ICTR_TRIANG_BEHIND 2    /* bit 1: not in front of its first view's camera (P2 . X <= 0) */
typedef struct ictr_triang_params {
  int32_t noiter;                      /* iterations at most (0: the start point comes back, covariance 0) */
  float minres;                        /* stop once the mean squared residual is <= minres */
  float damp_init, damp_fct, maxdamp;  /* LM: first damping, its factor, stop once damp >= maxdamp */
} ictr_triang_params;
typedef struct ictr_triang ictr_triang;
/* caps: max_points 1 .. 2^24, max_obs 2 * max_points .. 2^28 (observations of all tracks), max_frames 1 .. 2^20 */
int ictr_triang_create(ictr_triang **out, int64_t max_points, int64_t max_obs, int64_t max_frames);
void ictr_triang_destroy(ictr_triang *t);
/* P [nframes][12]: row-major 3x4 camera matrices, f32. The setters are refused (ICTR_ERR_STATE) while a run is in flight. */
int ictr_triang_set_cameras(ictr_triang *t, const float *P, int64_t nframes);
/* the ragged track list: point i owns observations offsets[i] .. offsets[i+1]-1 (offsets[0] = 0, n + 1 entries) of
 * view[] (frame index), x[], y[] (pixels). ICTR_ERR_INVALID for a track of fewer than 2 views or a view >= nframes.
 * Repacks the list for the kernel on the device and waits for that (the null stream). */
int ictr_triang_set_tracks(ictr_triang *t, int64_t n, const int64_t *offsets, const int32_t *view, const float *x,
                           const float *y);
/* enqueues upload, kernel and read-back on hip_stream (NULL: the null stream) and returns. params: NULL allowed for DLT.
 * init_pts [n][3]: the start points of GN / LM / DEPTH (required there); campos, ptdir [n][3]: centre and unit ray of
 * DEPTH (required there). The arrays are copied before the call returns. */
int ictr_triang_run(ictr_triang *t, int mode, const ictr_triang_params *params, const float *init_pts,
                    const float *campos, const float *ptdir, void *hip_stream);
/* waits for the last run; any pointer may be NULL. pts [n][3], cov [n][9] (row-major 3x3; DEPTH: the scalar in word 0,
 * zeros beyond), iters [n], status [n] (ICTR_TRIANG_NONFINITE | ICTR_TRIANG_BEHIND) */
int ictr_triang_wait(ictr_triang *t, float *pts, float *cov, int32_t *iters, int32_t *status);
/* The reference library's four entry points with its parameter lists and layouts (P [12][noviews], pt2d [2][noviews],
 * pt3d in place, cov 9 floats or, for the depth, 1): the same kernels on a batch of one point. Unlike the reference
 * they return a status. */
int ictr_triangulate_DLT(float *pt3d, float *AtAinv, const float *pt2d, const float *P, const int noviews);
int ictr_triangulate_full3D(float *pt3d, float *pt3d_cov, const float *pt2d, const float *P, const int noviews,
                            const int noiter, const float minres);
int ictr_triangulate_full3D_LM(float *pt3d, float *pt3d_cov, const float *pt2d, const float *P, const int noviews,
                               const int noiter, const float damp_init, const float damp_fct, const float minres,
                               const float maxdamp);
int ictr_triangulate_depthonly(float *pt3d, float *depth_cov, const float *campos, const float *ptdir, const float *pt2d,
                               const float *P, const int noviews, const int noiter, const float minres);

/* ---------------------------------------------------------------- point-track front end (ictr_frontend.hip)
 * The stage in front of the device code, on the device: corners, forward / backward flow on a node grid, the sliding
 * window of tracks. Each part equals host code of the Python package bit for bit (DESIGN.md §4 "Point-track front end"):
 * patchflow.good_features, patchflow.dense_flow, classoftrack.func_get_transf_position, classoftrack.oftrack.addframe. */

/* patchflow.good_features(img, maxcorners, quality, mindist, win): the plane is level 0 of pyr, or, with pyr NULL, the
 * host image img [h][w] f32 (w, h are read from the pyramid otherwise). mindist >= 1, 0 <= win <= 8, maxcorners >= 1.
 * out_xy [maxcorners][2] (x, y) strongest first, *out_count of them are written. */
int ictr_good_features(const ictr_pyramid *pyr, const float *img, int w, int h, int maxcorners, double quality,
                       int mindist, int win, float *out_xy, int *out_count);

/* one direction of one frame pair on a `step` grid: nodes x = step/2 + i step < w, likewise y */
typedef struct ictr_flowgrid ictr_flowgrid;
int ictr_flowgrid_create(ictr_flowgrid **out, int w, int h, int step);
void ictr_flowgrid_destroy(ictr_flowgrid *g);
int ictr_flowgrid_dims(const ictr_flowgrid *g, int *nx, int *ny);
/* tracks the nodes from pyr_a to pyr_b (the kernel and arguments of ictr_patchflow, lv_l = 0), forms d = out - pts and
 * fills the lost nodes (dense_flow's rule); enqueued on hip_stream (NULL: the null stream), no host wait */
int ictr_flowgrid_compute(ictr_flowgrid *g, const ictr_pyramid *pyr_a, const ictr_pyramid *pyr_b, int psz, int lv_f,
                          int maxiter, float eps, void *hip_stream);
/* the same with the 1-D kernel of ictr_patchdisp (a rectified stereo pair): same grid object, fill, gather and dense
 * field; after the fill every y displacement of the grid is exactly +0.0 */
int ictr_flowgrid_compute_x(ictr_flowgrid *g, const ictr_pyramid *pyr_a, const ictr_pyramid *pyr_b, int psz, int lv_f,
                            int maxiter, float eps, void *hip_stream);
/* injects node displacements d [ny][nx][2] and the lost mask [ny][nx] (1 = lost, its d is ignored) and fills */
int ictr_flowgrid_set_nodes(ictr_flowgrid *g, const float *d, const uint8_t *lost);
/* d after the fill and the lost mask; either may be NULL */
int ictr_flowgrid_nodes(const ictr_flowgrid *g, float *d, uint8_t *lost);
/* func_get_transf_position(xy, F[:,:,0], F[:,:,1]) with F = the dense field, which is not formed. xy, out [K][2] f64 */
int ictr_flowgrid_gather(const ictr_flowgrid *g, const double *xy, int64_t K, double *out);
/* the dense field [h][w][2] f32 of dense_flow into out (a device pointer when on_device != 0) */
int ictr_flowgrid_dense(const ictr_flowgrid *g, float *out, int on_device);

/* the loop of patchflow.run_OF_point_track with a ring of bsize block slots on the device: device memory does not grow
 * with the sequence, a block that leaves the window is copied to a host store of the object */
typedef struct ictr_pointtrack ictr_pointtrack;
int ictr_pointtrack_create(ictr_pointtrack **out, int w, int h, int bsize, int maxcorners, int lv_f, int psz, int step,
                           int maxiter, float eps, double quality, int mindist, int win, double th_ratio, double th_abs);
void ictr_pointtrack_destroy(ictr_pointtrack *t);
/* img [h][w] f32 in host memory (copied before the call returns). From the second frame on: the pair's two grids, the
 * corners of its first frame, oftrack.addframe. Everything is enqueued; the host reads nothing back. */
int ictr_pointtrack_push_frame(ictr_pointtrack *t, const float *img);
/* oftrack.frcounter: frame pairs so far = blocks */
int ictr_pointtrack_frcounter(const ictr_pointtrack *t, int64_t *frcounter);
/* block `block` as addframe holds it before any compaction: *count rows (0: the frame had no corner) of tracks
 * [count][2][bsize] f32, valid [count], absmovement [count] f64; buffers sized for maxcorners rows, any but count may be
 * NULL. A block b <= frcounter - bsize has left the window (oftrack keeps its valid rows only). Waits for the device. */
int ictr_pointtrack_read_block(ictr_pointtrack *t, int64_t block, float *tracks, uint8_t *valid, double *absmovement,
                               int *count);

/* ---------------------------------------------------------------- stereo track window (ictr_stereotrack.hip)
 * misc_src/run_test_OF_track.py:170-223 on the device, equal to stereotrack.stereo_track_window_host bit for bit
 * (DESIGN.md §4 "Stereo track window"): start points are sent to the right frame through the disparity and checked back
 * (open), then carried through the left and right flows of one frame pair per advance with the script's eight tests; a
 * point that fails once is dead. count / read compact the survivors in start order into xy_t [M][4][bsize]. One step's
 * fields are resident at a time: device memory is the window state [bsize][4][N] f64 and does not grow with the sequence.
 * Everything is enqueued on the null stream; the host waits in count (for M) and in read (for the M rows) only. */

/* a displacement field: a kind, an exact sign (+1 or -1; the script's -imgs_d is sign -1) and where it lives */
#define ICTR_FIELD_PLANE 0 /* float32 [h][w], moves x only (a disparity) */
#define ICTR_FIELD_FLOW 1  /* float32 [h][w][2] interleaved (u, v) */
#define ICTR_FIELD_GRID 2  /* an ictr_flowgrid* of the window's size that holds a field; its dense field is not formed */
typedef struct ictr_field {
  int32_t kind;      /* ICTR_FIELD_* */
  int32_t sign;      /* +1 or -1 */
  int32_t on_device; /* plane, flow: data is device memory (read when the step runs) instead of host memory (copied
                        before the call returns) */
  int32_t x_only;    /* flow, grid: the first component alone moves the point (the stereo pair); a plane always is */
  const void *data;
} ictr_field;
/* float64 fields have no kind: a caller that holds them converts exactly or not at all. */

typedef struct ictr_stereotrack ictr_stereotrack;
/* 2 <= w, h; 1 <= bsize <= 256 */
int ictr_stereotrack_create(ictr_stereotrack **out, int w, int h, int bsize, double th_ratio, double th_abs);
void ictr_stereotrack_destroy(ictr_stereotrack *t);
/* frame 0. xy0: f64 [n][2] start points in host memory, or NULL: every pixel in the script's meshgrid order (n = w h, or
 * 0). 1 <= n <= 2^24. lr, rl: the x-only fields left -> right and right -> left of frame 0. Starts a new window. */
int ictr_stereotrack_open(ictr_stereotrack *t, const double *xy0, int64_t n, const ictr_field *lr, const ictr_field *rl);
/* frame fr = 1 .. bsize-1, in order: the four two-component flows of the pair fr-1 -> fr and the x-only fields of frame
 * fr; ICTR_ERR_STATE before open and after bsize-1 calls */
int ictr_stereotrack_advance(ictr_stereotrack *t, const ictr_field *l_fwd, const ictr_field *l_bwd,
                             const ictr_field *r_fwd, const ictr_field *r_bwd, const ictr_field *lr_next,
                             const ictr_field *rl_next);
/* after the last advance: the ordered compaction (counts per workgroup, a scan, the rows); *m = survivors */
int ictr_stereotrack_count(ictr_stereotrack *t, int64_t *m);
/* after count: xy_t f64 [m][4][bsize] and rows int64 [m] (start indices, ascending); either may be NULL */
int ictr_stereotrack_read(ictr_stereotrack *t, double *xy_t, int64_t *rows);
/* per-launch timing with HIP events; ms[2] of the window completed by read: the open and advance kernels, the
 * compaction kernels. Both refused (ICTR_ERR_STATE) while a window is open and not read. */
int ictr_stereotrack_set_timing(ictr_stereotrack *t, int on);
int ictr_stereotrack_get_kernel_times(const ictr_stereotrack *t, float *ms);

/* ---------------------------------------------------------------- window camera RANSAC (ictr_camransac.hip)
 * "RANSAC camera estimation ... for whole sequence, check right for consistency" (misc_src/run_test_OF_track.py, TODO 1;
 * DESIGN.md §4 "Window camera RANSAC"): ntrials trials over the N points of a track window seen in nframes frames from
 * nsides = 1 (left) or 2 (left, right) cameras. Trial g draws 4 points once (the pose sampler's stream over all N) and
 * fits one pose per frame by P3P from their left observations; a point is an inlier of the trial iff it counts (mask bit
 * set, its 3 coordinates and its 2 nsides nframes observation coordinates finite) and reprojects within thresh (strictly)
 * in every frame and on every side, the right camera at t_f + offset. The largest count wins, the lowest trial on ties.
 * X: f64 [3][N] in the first view's frame; xy: f64 [nsides][nframes][2][N] (the bundle adjuster's layout); words: bit
 * j % 64 of word j / 64 is point j, NULL: every point. 4 <= N <= 2^22, 1 <= nframes <= 64, 1 <= ntrials <= 2^20.
 * run enqueues on hip_stream (NULL: the null stream) and returns; wait blocks and copies out: best_trial (-1: no trial
 * succeeded; then best_count 0, G NaN, words 0, dd NaN, draws -1), best_count, draws [4], G [nframes][12] row-major
 * [R | t], p [nframes][6] = se3_log(G) taken on the host, inl_words [ceil(N / 64)], dd [N] each point's largest
 * reprojection distance under the winner (any may be NULL). The setters, run and the debug entry return ICTR_ERR_STATE
 * while a run is in flight; run needs points, observations and the camera, and with two sides the offset. */
typedef struct ictr_camransac ictr_camransac;
int ictr_camransac_create(ictr_camransac **out, int64_t n, int64_t nframes, int64_t nsides);
void ictr_camransac_destroy(ictr_camransac *r);
int ictr_camransac_set_camera(ictr_camransac *r, const double *fc, const double *cc);
int ictr_camransac_set_offset(ictr_camransac *r, const double *offset);
int ictr_camransac_set_points(ictr_camransac *r, const double *X);
int ictr_camransac_set_observations(ictr_camransac *r, const double *xy);
int ictr_camransac_set_mask(ictr_camransac *r, const uint64_t *words);
int ictr_camransac_run(ictr_camransac *r, int64_t ntrials, double thresh, uint64_t seed, void *hip_stream);
int ictr_camransac_wait(ictr_camransac *r, int64_t *best_trial, int64_t *best_count, int32_t *draws, double *G, double *p,
                        uint64_t *inl_words, double *dd);
/* per-kernel timing with HIP events around the launches of the next runs; ms[4] of the last waited run: k_cr_hyp,
 * k_cr_score, k_cr_select (summed over the chunks) and k_cr_flags + k_cr_mask */
int ictr_camransac_set_timing(ictr_camransac *r, int on);
int ictr_camransac_get_kernel_times(const ictr_camransac *r, float *ms);
int ictr_camransac_chunk_size(const ictr_camransac *r);
/* inspection: k_cr_hyp and k_cr_score<tile> alone over trials first_trial .. first_trial + count - 1 (below 2^20), in the
 * object's own chunks and tile, on the null stream; no selection. status [count], draws [count][4],
 * G [count][nframes][12], cnt [count] (0 for a failed trial) */
int ictr_debug_camransac_trials(ictr_camransac *r, double thresh, uint64_t seed, int64_t first_trial, int64_t count,
                                int32_t *status, int32_t *draws, double *G, uint32_t *cnt);

/* ---------------------------------------------------------------- window hand-over (ictr_handover.hip)
 * A counted window (ictr_stereotrack_count has run; before or after ictr_stereotrack_read) handed to the static split and
 * the camera fit on the device (DESIGN.md §4 "Window hand-over"): the history and the rows stay where they are, kernels
 * write the split's view pairs (fsplit.pairs_from_stereo_tracks), the fit's points (camfit.depth_from_disparity and
 * points_from_first_view) and observations (camfit.observations_from_stereo_tracks) from them, bit for bit what the host
 * functions make of the xy_t that read returns. The window is not changed: read afterwards returns the same xy_t.
 * The split and the fit are made for exactly n = M points (the fit's summation order is a function of n), so after count;
 * an object is reused when the next window keeps the same M. Limits: 2 <= bsize <= 65 (the split's 64 view pairs),
 * 8 <= M <= 2^22.
 * The three from-window entries enqueue on the null stream, like the window, and return without waiting; a run on the
 * null stream or on a blocking stream follows in order, a run on a non-blocking stream is the caller's to order behind
 * them. Each returns ICTR_ERR_STATE when the window is not counted or a run of r is in flight, ICTR_ERR_INVALID when r
 * was not made for the window's M (and the frames named below); nothing is launched then. */
/* needs r made for n = M, npairs = 2 (bsize / 2); pair 2 g = (left g, right g + ceil(bsize / 2)), pair 2 g + 1 = (right g,
 * left g + ceil(bsize / 2)); the middle frame of an odd window is in no pair */
int ictr_fsplit_set_pairs_from_window(ictr_fsplit *r, const ictr_stereotrack *t);
/* X = ((xl - cx) / fx d, (yl - cy) / fy d, d), d = baseline fx / (xr - xl) on frame 0 (baseline: P1[0, 3] of the script,
 * signed like the disparity), with the camera of ictr_camfit_set_camera, which comes first (ICTR_ERR_STATE). A zero
 * disparity gives a point that is not finite, which the fit leaves out. */
int ictr_camfit_set_points_from_window(ictr_camfit *r, const ictr_stereotrack *t, double baseline);
/* the left (right = 0) or right (right != 0) x, y of every frame; needs r made for nframes = bsize */
int ictr_camfit_set_observations_from_window(ictr_camfit *r, const ictr_stereotrack *t, int right);
/* the inlier words of the last run of s, waited for or still in flight, copied device to device on hip_stream, which is
 * to be the stream of that run (NULL: the null stream). ICTR_ERR_STATE when s has never run or a run of r is in flight,
 * ICTR_ERR_INVALID when the point counts differ. */
int ictr_camfit_set_mask_from_fsplit(ictr_camfit *r, const ictr_fsplit *s, void *hip_stream);
/* inspection: the input buffers as they stand on the device, after everything enqueued so far: xy [npairs][4][N];
 * X [3][N], xy [nframes][2][N], words [ceil(N / 64)] (any of the three may be NULL) */
int ictr_debug_fsplit_pairs(const ictr_fsplit *r, double *xy);
int ictr_debug_camfit_inputs(const ictr_camfit *r, double *X, double *xy, uint64_t *words);
/* The same for the bundle adjustment: the points as ictr_camfit_set_points_from_window (ictr_ba_set_camera comes first),
 * the left observations into side 0 and, with two sides, the right ones into side 1, the split's words as the mask; and
 * the adjuster's device inputs read back (any of X [3][N], xy [nsides][nframes][2][N], words may be NULL). */
int ictr_ba_set_points_from_window(ictr_ba *r, const ictr_stereotrack *t, double baseline);
int ictr_ba_set_observations_from_window(ictr_ba *r, const ictr_stereotrack *t);
int ictr_ba_set_mask_from_fsplit(ictr_ba *r, const ictr_fsplit *s, void *hip_stream);
int ictr_debug_ba_inputs(const ictr_ba *r, double *X, double *xy, uint64_t *words);

/* The same for the window camera RANSAC (ictr_camransac_set_camera comes first for the points; both sides of an object of
 * two sides are written), its winner's inlier words, of a run waited for or still in flight, copied on hip_stream into
 * the fit's or the adjuster's mask, and its device inputs read back. As for ictr_camfit_set_mask_from_fsplit, hip_stream
 * is to be the stream of that run (NULL: the null stream): the copy is ordered behind the run by the stream alone, and on
 * another non-blocking stream it is the caller's to order. ictr_debug_camransac_inputs returns in words the mask in
 * effect: the words of the last ictr_camransac_set_mask, or every point's bit (bits past N clear) where that was NULL or
 * never called. */
int ictr_camransac_set_points_from_window(ictr_camransac *r, const ictr_stereotrack *t, double baseline);
int ictr_camransac_set_observations_from_window(ictr_camransac *r, const ictr_stereotrack *t);
int ictr_camfit_set_mask_from_camransac(ictr_camfit *r, const ictr_camransac *s, void *hip_stream);
int ictr_ba_set_mask_from_camransac(ictr_ba *r, const ictr_camransac *s, void *hip_stream);
int ictr_debug_camransac_inputs(const ictr_camransac *r, double *X, double *xy, uint64_t *words);

/* ---------------------------------------------------------------- variational refinement (ictr_flowrefine.hip)
 * A dense flow A -> B refined per pixel at level 0 (DESIGN.md §4 "Variational refinement of a dense field"): n_outer
 * times warp B by the field, linearise brightness and gradient constancy with robust weights, and solve for an increment
 * with n_sor red-black SOR sweeps under a robust smoothness term. The rule is patchflow.refine_flow_host's, in f32.
 * Planes are [h][w] f32, fields [h][w][2] f32 interleaved (u, v). */
typedef struct ictr_flowrefine ictr_flowrefine;
/* 4 <= w, h <= 32768 */
int ictr_flowrefine_create(ictr_flowrefine **out, int w, int h);
void ictr_flowrefine_destroy(ictr_flowrefine *r);
/* defaults 16, 13, 4.5, 8, 5, 1.6. Refused: a negative or non-finite value, alpha = 0 (no coupling: 0 / 0 at every pixel
 * without data), n_outer or n_sor above 1024, omega outside (0, 2). n_outer = 0 returns the source's bits. */
int ictr_flowrefine_set_params(ictr_flowrefine *r, float alpha, float gamma, float delta, int n_outer, int n_sor,
                               float omega);
/* src: an ICTR_FIELD_FLOW in host memory (checked for finiteness and copied before the call returns; a value that is not
 * finite is refused) or in device memory (read when the run executes; not checked), or an ICTR_FIELD_GRID, whose dense
 * field is formed into the refiner's own buffer. sign must be +1; the descriptor's x_only is not read. x_only != 0 (a
 * stereo pair): only u moves, v comes back with its input bits. Both pyramids and the field are of the refiner's size
 * (ICTR_ERR_INVALID otherwise); only the level-0 image planes are read, with any padding. Everything is enqueued on
 * hip_stream (NULL: the null stream); the call waits for nothing but the copy of a host field. */
int ictr_flowrefine_run(ictr_flowrefine *r, const ictr_pyramid *pyr_a, const ictr_pyramid *pyr_b, const ictr_field *src,
                        int x_only, void *hip_stream);
/* waits for the last run and copies its field [h][w][2] to out (a device pointer when on_device != 0) */
int ictr_flowrefine_result(ictr_flowrefine *r, float *out, int on_device);
/* the result buffer on the device (a device ICTR_FIELD_FLOW for the stereo track window), valid behind the run's stream */
const float *ictr_flowrefine_device_ptr(const ictr_flowrefine *r);
/* HIP events around the launches of the next runs; ms[4] of the last run (waits for it): k_fr_warp, k_fr_coef, k_fr_sor
 * summed over the outer iterations, and k_fr_init + k_fr_final. All 0 when timing was off. */
int ictr_flowrefine_set_timing(ictr_flowrefine *r, int on);
int ictr_flowrefine_get_kernel_times(ictr_flowrefine *r, float *ms);
/* the planes of the last outer iteration (waits for the run): which = 0 Bw, 1..5 a11 a12 a22 b1 b2, 6 7 the right and
 * down edge weights, 8 9 du dv after the last sweep, 10 11 the u, v that the iteration started from */
#define ICTR_FLOWREFINE_STAGES 12
int ictr_flowrefine_read_stage(ictr_flowrefine *r, int which, float *out);
/* inspection: a plane written from host memory, and one half-sweep k_fr_sor<colour> on the planes as they stand (null
 * stream, waited for) */
int ictr_debug_flowrefine_write_stage(ictr_flowrefine *r, int which, const float *in);
int ictr_debug_flowrefine_half_sweep(ictr_flowrefine *r, int colour, int x_only);

/* ---------------------------------------------------------------- densification of a flow grid (ictr_densify.hip)
 * The dense field of a flow grid at level 0 by photometric voting (DESIGN.md §4 "Densification of a flow grid"): every
 * pixel takes the weighted mean of the displacements of all nodes that are not lost and whose psz x psz patch covers it,
 * in ascending node row, then column; a node's vote is dropped when it moves the pixel out of the frame, and weighs
 * 1 / max(|B(x + d) - A(x)|, minerr)^power otherwise. A pixel without a vote takes the grid's up-sampled value
 * (ictr_flowgrid_dense). The rule is patchflow.densify_flow_host's, in f32. The object owns its [h][w][2] f32 result. */
typedef struct ictr_flowdensify ictr_flowdensify;
/* 2 <= w, h <= 32768 */
int ictr_flowdensify_create(ictr_flowdensify **out, int w, int h);
void ictr_flowdensify_destroy(ictr_flowdensify *z);
/* defaults 2.0, 1. Refused: a minerr that is not finite or not positive, a power outside 1..4. */
int ictr_flowdensify_set_params(ictr_flowdensify *z, float minerr, int power);
/* grid: holds a field of the object's size, tracked with patches of psz (1 .. 32); both pyramids are of that size
 * (ICTR_ERR_INVALID otherwise; ICTR_ERR_STATE for a grid without a field). A step and psz whose node table does not fit
 * a workgroup's LDS are refused (ICTR_ERR_INVALID). Only the level-0 image planes are read, with any padding. One launch,
 * enqueued on hip_stream (NULL: the null stream); the call does not wait. */
int ictr_flowdensify_run(ictr_flowdensify *z, const ictr_flowgrid *grid, const ictr_pyramid *pyr_a,
                         const ictr_pyramid *pyr_b, int psz, void *hip_stream);
/* waits for the last run and copies its field [h][w][2] to out (a device pointer when on_device != 0) */
int ictr_flowdensify_result(ictr_flowdensify *z, float *out, int on_device);
/* the result buffer on the device (a device ICTR_FIELD_FLOW for the refinement and for the stereo track window), valid
 * behind the run's stream */
const float *ictr_flowdensify_device_ptr(const ictr_flowdensify *z);
/* HIP events around the launch of the next runs; *ms of the last run's k_densify (waits for it), 0 when timing was off */
int ictr_flowdensify_set_timing(ictr_flowdensify *z, int on);
int ictr_flowdensify_get_kernel_ms(ictr_flowdensify *z, float *ms);
/* planes [h][w] f32 of the last run (waits for it): which = 0 the votes a pixel took, 1 their summed weight */
#define ICTR_FLOWDENSIFY_STAGES 2
int ictr_flowdensify_read_stage(ictr_flowdensify *z, int which, float *out);

/* ---------------------------------------------------------------- coarse-to-fine dense flow (ictr_c2fflow.hip)
 * The dense field A -> B built level by level (DESIGN.md §4 "Coarse-to-fine dense flow"): for l = lv_f .. 0 a grid of
 * nodes at step / 2 + k step of the level's own size is searched at that level alone, every node started from twice the
 * coarser level's dense field at (min(X >> 1, w' - 1), min(Y >> 1, h' - 1)) ((0, 0) at lv_f); the node displacements are
 * filled (the flow grid's fill), densified (ictr_flowdensify's rule) and, when switched on, refined (ictr_flowrefine's
 * rule) on the level's planes. The result is level 0's field. The rule is patchflow.c2f_flow_host's, in f32.
 * Status of a node: 0 lost (its start is out of view, or not finite: no vote, filled from its neighbours), 1 tracked,
 * 2 held by the conditioning test, 3 held because it left the view while iterating, 4 held because it ended further than
 * psz from its start (or not finite). A held node keeps its start's bits and votes. */
typedef struct ictr_c2fflow ictr_c2fflow;
#define ICTR_C2F_LOST 0
#define ICTR_C2F_TRACKED 1
#define ICTR_C2F_HELD_COND 2
#define ICTR_C2F_HELD_VIEW 3
#define ICTR_C2F_HELD_FAR 4
/* w x h frames, levels lv_f .. 0 (0 <= lv_f <= 15), step >= 1, psz 1 .. 32. Refused with a message: a level smaller than
 * 2 x 2, a level without a node (step / 2 >= its width or height). */
int ictr_c2fflow_create(ictr_c2fflow **out, int w, int h, int lv_f, int step, int psz);
void ictr_c2fflow_destroy(ictr_c2fflow *c);
/* defaults 10, 0.01, 2.0, 1: the search's iterations per level and stop (|step| < eps), the densifier's parameters */
int ictr_c2fflow_set_params(ictr_c2fflow *c, int maxiter, float eps, float minerr, int power);
/* on != 0: refine every level with these parameters (ictr_flowrefine_set_params' rules; every level must be at least
 * 4 x 4, refused otherwise). Default off. */
int ictr_c2fflow_set_refine(ictr_c2fflow *c, int on, float alpha, float gamma, float delta, int n_outer, int n_sor,
                            float omega);
/* Both pyramids: levels 0 .. lv_f of the object's level sizes (refused otherwise), padding >= psz, the first with
 * gradient planes. A step and psz whose node table does not fit the densifier's LDS are refused (ictr_flowdensify_run). Everything is enqueued on hip_stream (NULL: the null stream); the call does not wait. */
int ictr_c2fflow_run(ictr_c2fflow *c, const ictr_pyramid *pyr_a, const ictr_pyramid *pyr_b, void *hip_stream);
/* waits for the last run and copies level 0's field [h][w][2] to out (a device pointer when on_device != 0) */
int ictr_c2fflow_result(ictr_c2fflow *c, float *out, int on_device);
/* the result buffer on the device (a device ICTR_FIELD_FLOW), valid behind the run's stream */
const float *ictr_c2fflow_device_ptr(const ictr_c2fflow *c);
/* size and node counts of a level; any pointer may be NULL */
int ictr_c2fflow_level_dims(const ictr_c2fflow *c, int level, int *w, int *h, int *nx, int *ny);
/* of the last run (waits for it): the level's field [h_l][w_l][2], its node displacements after the fill [ny][nx][2] and
 * the status bytes [ny][nx]; any pointer may be NULL */
int ictr_c2fflow_read_level(ictr_c2fflow *c, int level, float *field, float *d, unsigned char *status);
/* HIP events around the stages of the next runs; ms[3 (lv_f + 1)] of the last run (waits for it): per level from 0 the
 * search (k_c2f_level and the fill), the densification and the refinement, zeros when timing was off */
int ictr_c2fflow_set_timing(ictr_c2fflow *c, int on);
int ictr_c2fflow_get_kernel_ms(ictr_c2fflow *c, float *ms);
/* -- patch-mean normalisation (DESIGN.md §4 "Patch-mean normalisation"): its switch and the reader of the node bias */
/* on != 0: patch-mean normalisation for the next runs, for frames whose brightness differs by a locally constant offset
 * (the two cameras of a rig, auto-exposure). The search removes the mean of the template and of every frame window;
 * every node that votes from inside the view gets its brightness offset beta = mean(B at its final position) -
 * mean(A at the node), any other node +0.0; a node's vote in the densification weighs |Bw - A - beta|. The refinement is
 * unchanged: its brightness term still sees the offset. Default off: the runs are then, bit for bit and kernel for
 * kernel, those of an object that never had this call. */
int ictr_c2fflow_set_patnorm(ictr_c2fflow *c, int on);
/* of the last run (waits for it), which had patnorm on (refused otherwise): the level's node bias [ny][nx] */
int ictr_c2fflow_read_level_bias(ictr_c2fflow *c, int level, float *bias);
/* -- the 1-D (x only) form for rectified stereo pairs (DESIGN.md §4 "The 1-D form"): its switch */
/* on != 0: the next runs search along x only. A node starts from the x component of the coarser field alone, the search is
 * k_patchdisp's rule at the level (hxx and hyy; held by conditioning iff !(tr > 0) or !(hxx > 1e-2 tr); p += bx / hxx),
 * the rejection is (p - init)^2 > psz^2, the refinement (when on) moves u alone, and the y component of every node and of
 * every level's field is +0.0 to the bit. It combines with patch-mean normalisation. Default off: the runs are then, bit
 * for bit, those of an object that never had this call. */
int ictr_c2fflow_set_x_only(ictr_c2fflow *c, int on);
int ictr_c2fflow_get_x_only(const ictr_c2fflow *c, int *on);
/* -- a finest level above 0, and the up-sampling that finishes such a run (DESIGN.md §4 "A finest level above 0").
 * The rule (patchflow.upsample_flow_host states it in f64): with s = 2^lv and a field F of level lv's size w_l x h_l, output
 * pixel (x, y) of the w x h frame takes fx = clamp((x + 0.5) / s - 0.5, 0, w_l - 1), x0 = floor(fx), x1 = min(x0 + 1,
 * w_l - 1), rx = fx - x0 (fy, y0, y1, ry alike with h_l) and, per component, top = (1 - rx) F[y0][x0] + rx F[y0][x1],
 * bot = (1 - rx) F[y1][x0] + rx F[y1][x1], val = (1 - ry) top + ry bot; the output is s val. The device takes the six
 * products and three sums in f32 in that order, each rounded. */
/* ictr_c2fflow_create with a finest level lv_l (0 <= lv_l <= lv_f, refused otherwise): the runs search, densify and refine
 * the levels lv_f .. lv_l alone, and only those get a grid, a densifier, events, status and bias rows and a refiner; their
 * results are, bit for bit, those of the same levels of an object with lv_l = 0. With lv_l > 0 the object owns one
 * w x h x 2 result plane: a run ends with ONE launch of k_flow_upsample from level lv_l's field (the refiner's when the run
 * refined; with x_only set the y component is not read and is written as +0.0), and ictr_c2fflow_result and
 * ictr_c2fflow_device_ptr hand out that plane. The size rules of ictr_c2fflow_create hold for the levels lv_l .. lv_f;
 * ictr_c2fflow_level_dims, _read_level and _read_level_bias refuse a level below lv_l; ictr_c2fflow_get_kernel_ms keeps
 * its 3 (lv_f + 1) values, zeros below lv_l. lv_l = 0 is ictr_c2fflow_create. */
int ictr_c2fflow_create_lvl(ictr_c2fflow **out, int w, int h, int lv_f, int lv_l, int step, int psz);
int ictr_c2fflow_get_lv_l(const ictr_c2fflow *c, int *lv_l);
/* *ms of k_flow_upsample in the last run (waits for it); 0 when timing was off or lv_l = 0 */
int ictr_c2fflow_get_upsample_ms(ictr_c2fflow *c, float *ms);
/* The rule on a caller's field: src [h_l][w_l][2], out [h][w][2], 1 <= lv <= 15, and (w_l, h_l) must be the size of level lv
 * of a w x h pyramid (round-half-even halving), refused otherwise. x_only != 0: the y component of src is not read and the
 * y component of out is +0.0. on_device = 0: both are host arrays, staged by the call, which waits. on_device != 0: both are
 * device pointers and the kernel is enqueued on hip_stream (NULL: the null stream); the call does not wait. */
int ictr_flow_upsample(const float *src, int w_l, int h_l, int lv, float *out, int w, int h, int x_only, int on_device,
                       void *hip_stream);
/* -- colour (three-channel) frames (DESIGN.md §4 "Colour").
 * A colour frame is THREE pyramids, one per channel, built by ictr_pyramid_create as any other and equal in size, levels
 * and padding. The rule (patchflow.c2f_flow_host on triples states it in f64): the nodes, the starts, the view tests, the
 * stop, the rejection, the status values, the fill and the up-sampling are those of one channel; the search sums
 * H = sum_c sum_px G_c G_c^T and b = sum_c sum_px G_c (T_c - I_c) and takes one conditioning decision and one step per
 * node; with patnorm every channel loses its own patch mean and a node has one brightness offset per channel; a
 * densifier's vote weighs the channel mean e = (1/3) sum_c |Bw_c - A_c - beta_c|; the refinement warps and differentiates
 * per channel, takes its two robust weights jointly over the channels on the channel mean,
 * q0 = delta inside / 2 / sqrt((1/3) sum_c n0_c Iz_c^2 + eps^2) and qg likewise, and its coefficients as channel means.
 * Three equal channels give the grey rule in real arithmetic. The number of channels is 1 or 3. */
/* n = 1 (the object as created) or 3; anything else is refused. To be called before the first run (refused after one): it
 * sizes the node bias block, [ny][nx][n] floats per level; if that allocation fails the object keeps its channel count.
 * (The refinement's two more warp planes are made by the first refined run of a 3-channel object.) */
int ictr_c2fflow_set_channels(ictr_c2fflow *c, int n);
int ictr_c2fflow_get_channels(const ictr_c2fflow *c, int *n);
/* ictr_c2fflow_run of a 3-channel object: pyr_a[ch], pyr_b[ch] are channel ch of frames A and B. Refused with a message:
 * on a 1-channel object (and ictr_c2fflow_run on a 3-channel one), and when the three pyramids of a frame differ in
 * geometry (size, levels' strides or padding). Every other check is ictr_c2fflow_run's, per channel. The result plane, the
 * levels' fields, node displacements and status bytes are read as after ictr_c2fflow_run. */
int ictr_c2fflow_run_rgb(ictr_c2fflow *c, const ictr_pyramid *const pyr_a[3], const ictr_pyramid *const pyr_b[3],
                         void *hip_stream);
/* of the last run, which had patnorm on, of a 3-channel object (waits for it): the node bias [ny][nx][3] of a level;
 * ictr_c2fflow_read_level_bias refuses such an object */
int ictr_c2fflow_read_level_bias_rgb(ictr_c2fflow *c, int level, float *bias);
/* -- the patch cost of the search (DESIGN.md §4 "Robust patch cost"): ictr_c2fflow_set_cost, ictr_c2fflow_get_cost,
 * ICTR_C2F_COST_L2, ICTR_C2F_COST_HUBER */
#include "ictr_c2f_cost.h"
/* -- a lockstep set of coarse-to-fine flows, one launch per stage for all members (DESIGN.md §4 "Lockstep sets"):
 * ictr_c2fset_create, _destroy, _run, _run_rgb, _size, _last_operations, _set_timing, _get_kernel_ms */
#include "ictr_c2f_set.h"

#ifdef __cplusplus
}
#endif
#endif /* ICTR_H */
