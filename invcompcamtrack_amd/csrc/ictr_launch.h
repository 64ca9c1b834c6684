// ictr_launch.h -- host-side interface between the translation units of the library: every function that one .hip file
// defines and another calls, the argument bundles of the launchers, the error helper and the HIP-check macro. Included by
// every .hip file, the defining one too, so that a definition that drifts from its declaration does not compile or link.
// Nothing here is seen by a kernel: kernel arguments are the structs of ictr_dev.h (and Exchange of ictr_xchg.h), which the
// launchers fill.
#pragma once

#include <stddef.h>

#include "ictr_dev.h"
#include "ictr_own.h"

struct ictr_pyramid;
struct ictr_p2p;

// what ictr_host.hip, the only file that sees inside ictr_pyramid, exposes about one (ictr_icgn.hip, ictr_patchflow.hip,
// ictr_frontend.hip)
struct ictr_pyramid_view {
  int nlev, pad;
  const int *w, *h, *sw;
  float *const *img, *const *dx, *const *dy;
  int getgrad;  // 1: the gradient planes exist (image-only pyramids of the tracker's on-the-fly path have none)
};
extern "C" int ictr_pyramid_view_(const ictr_pyramid *p, ictr_pyramid_view *v);  // ictr_host.hip
// A level of a pyramid (level 0 unless the caller names another) as a kernel reads a frame: the plane at pixel (0, 0),
// inside the padding, and its row stride. The one place that forms this address; `who` opens the message about a NULL or
// empty pyramid, or one without the level. Size checks are the caller's.
struct ictr_level0 {
  const float *img;
  int stride, w, h;
};
inline int ictr_pyramid_level0(const ictr_pyramid *p, const char *who, ictr_level0 *l, int level = 0) {
  ictr_pyramid_view v;
  if (!p || ictr_pyramid_view_(p, &v) || v.nlev < 1) return ictr::fail(ICTR_ERR_INVALID, "%s: a pyramid is NULL", who);
  if (level < 0 || level >= v.nlev) return ictr::fail(ICTR_ERR_INVALID, "%s: a pyramid has no level %d", who, level);
  *l = ictr_level0{v.img[level] + (size_t)v.pad * v.sw[level] + v.pad, v.sw[level], v.w[level], v.h[level]};
  return ICTR_OK;
}
// The stages that the coarse-to-fine flow (ictr_c2fflow.hip) runs per level, on n (1 .. kSetMax) objects of the level's
// size and of one set of parameters at once, one launch per stage for all of them (DESIGN.md §4 "Lockstep sets"; a single
// object is n = 1): the node buffers of a flow grid that its search kernel writes (raw displacements [K][2] and the lost
// bytes [K]) and the grids' fill on a stream; the densifiers' and the refiners' run reading level `level` of `channels`
// (1 or 3) pyramids per member and frame, pyr_a[m * channels + c] and pyr_b[m * channels + c], which the caller has
// checked to agree in geometry. No object's own event is recorded: the event the caller records behind the run stands
// for them.
struct ictr_flowgrid;
struct ictr_flowdensify;
struct ictr_flowrefine;
extern "C" int ictr_flowgrid_node_buffers_(ictr_flowgrid *g, float **draw, unsigned char **lost);  // ictr_frontend.hip
// rowhas: the caller's block of n * ny ints, cleared by the one memset (NULL with n = 1: the grid's own)
extern "C" int ictr_flowgrid_fill_(ictr_flowgrid *const *g, int n, int *rowhas, void *hip_stream);  // ictr_frontend.hip
// bias[m]: grid m's node bias [ny][nx][channels] on the device, as patch-mean normalisation has it (all NULL: none)
extern "C" int ictr_flowdensify_run_level_(ictr_flowdensify *const *z, const ictr_flowgrid *const *grid,
                                           const ictr_pyramid *const *pyr_a, const ictr_pyramid *const *pyr_b, int n,
                                           int channels, int psz, int level, const float *const *bias, void *hip_stream);
// field[m]: a device field [h][w][2]; bw12[m]: two more Bw planes [2][h][w] of the caller's on the device (3 channels
// alone); *ops: the launches (with n_outer = 0 the copies, one per member) enqueued
extern "C" int ictr_flowrefine_run_level_(ictr_flowrefine *const *r, const ictr_pyramid *const *pyr_a,
                                          const ictr_pyramid *const *pyr_b, int n, int channels, const float *const *field,
                                          int x_only, int level, float *const *bw12, int *ops, void *hip_stream);
// what a set compares its members' stages by: minerr and power; alpha, gamma, delta, omega and n_outer, n_sor
extern "C" int ictr_flowdensify_get_params_(const ictr_flowdensify *z, float *minerr, int *power);
extern "C" int ictr_flowrefine_get_params_(const ictr_flowrefine *r, float *p4, int *n2);
// the mailboxes of a connected p2p object as a kernel argument of the resident launch; non-zero: not connected (ictr_p2p.hip)
extern "C" int ictr_p2p_fill_xchg_(const ictr_p2p *p, ictr::ResXchg *x);
extern "C" const char *ictr_last_error(void);

// The window hand-over (ictr_handover.hip, DESIGN.md §4 "Window hand-over"): what the files that see inside their objects
// expose so that a counted window's history can be written into the next stages' input buffers without leaving the
// device. The split's pairs buffer has a layout of its own (ictr_fsplit_view). The fit, the adjuster and the window
// camera RANSAC each embed one ictr::WinInputs (ictr_wininputs.h) and hand it out as a WinDest; the split and the RANSAC
// hand out the inlier words of their last run as a WinMaskSrc.
struct ictr_stereotrack;
struct ictr_fsplit;
struct ictr_camfit;
struct ictr_ba;
struct ictr_camransac;
struct ictr_stereotrack_view {
  const double *hist;     // [bsize][4][n]
  const long long *rows;  // [m] start indices of the survivors, ascending
  int n, bsize, counted;  // counted: ictr_stereotrack_count has run on this window (hist and rows are final)
  long long m;
};
struct ictr_fsplit_view {
  double *xy;  // [np][4][n]
  int n, np;
  int pending;  // a run is in flight
};
namespace ictr {
struct WinInputs;
struct WinDest {
  WinInputs *in;
  const Readback *out;  // of the object: a run in flight fixes its inputs
  const char *object;   // "camfit", "ba", "camransac": ictr_<object>_wait, ictr_<object>_set_camera in the messages
  const char *noun;     // "fit", "adjuster", "RANSAC"
};
struct WinMaskSrc {
  const unsigned long long *words;  // [ceil(n / 64)] inlier bits of the last run, in the result block on the device
  int n;
  bool ran;          // a run was ever enqueued
  const char *noun;  // "split", "RANSAC"
};
}  // namespace ictr
extern "C" int ictr_stereotrack_view_(const ictr_stereotrack *t, ictr_stereotrack_view *v);  // ictr_stereotrack.hip
extern "C" int ictr_fsplit_view_(const ictr_fsplit *r, ictr_fsplit_view *v);                // ictr_fsplit.hip
extern "C" void ictr_fsplit_pairs_filled_(ictr_fsplit *r);  // the pairs a hand-over has filled count as set
extern "C" int ictr_fsplit_mask_(const ictr_fsplit *r, ictr::WinMaskSrc *m);
extern "C" int ictr_camfit_inputs_(ictr_camfit *r, ictr::WinDest *d);        // ictr_camfit.hip
extern "C" int ictr_ba_inputs_(ictr_ba *r, ictr::WinDest *d);                // ictr_ba.hip
extern "C" int ictr_camransac_inputs_(ictr_camransac *r, ictr::WinDest *d);  // ictr_camransac.hip
extern "C" int ictr_camransac_mask_(const ictr_camransac *r, ictr::WinMaskSrc *m);

namespace ictr {

// ---------------------------------------------------------------- errors, device, environment (ictr_host.hip)
// records the message for ictr_last_error (per thread) and returns `code`
int fail(int code, const char *fmt, ...);  // and HIPCHK(expr), which returns through it: ictr_own.h
int need_device();                          // ICTR_OK, or ICTR_ERR_NO_DEVICE with its message: there is no CPU fallback
int env_int(const char *name, int dflt);    // integer value of an environment variable, dflt when unset
int cu_count();                             // CUs of the calling thread's current device, queried once per device
void pyramid_level_size(int w, int h, int level, int *wl, int *hl);  // the size of a pyramid's level (round-half-even halving)

// the two RANSAC stages: trials per score workgroup from an environment variable, 16, 64 or (anything else) 32 ...
inline int ran_tile_env(const char *name) {
  const int tile = env_int(name, 32);
  return (tile == 16 || tile == 64) ? tile : 32;
}
// ... and the workgroups of `block` threads that give each of nwords 64-item words one wave
inline int ran_segs(int nwords, int block) { return (nwords + block / 64 - 1) / (block / 64); }
// the per-pixel kernels of the flow stages: a wave per 64 consecutive columns of a row, kWaves rows per workgroup
inline dim3 pixel_rows_grid(int cols, int rows) { return dim3((cols + 63) / 64, (rows + kWaves - 1) / kWaves); }

// ---------------------------------------------------------------- argument bundles of the launchers (host side only)
// launch geometry of one pyramid level's kernels
struct LevelLaunch {
  int level;
  int variant;  // selection bits as the launchers see them (ICTR_VARIANT_*)
  int gridx;    // workgroups per problem of the any-size kernels
  int cpw;      // wave64 fast paths (8x8, 4x4): points per wave chunk ...
  int gridx8;   // ... and workgroups per problem
};
// workgroups of a resident-iteration launch (ictr_resident.hip)
struct ResidentGeom {
  int parts, slots, np;  // worker workgroups per frame pair, pairs in flight, patches per wave (16 or 32)
};
// team form of the one-launch tracker (ictr_track1.hip, "Teams"): several workgroups per problem
struct T1Team {
  int team, q;  // workgroups per problem, points per workgroup
  Exchange x;   // ictr_xchg.h; the mailbox in the team layout
};

// ---------------------------------------------------------------- ictr_kernels.hip
// plain streaming read of nfloats floats (ictr_stream_read_bandwidth); sink: 8192 * kBlock floats, never written
void launch_stream_read(const float *src, size_t nfloats, float *sink, hipStream_t s);
// interleave a finished level into {img, dx, dy, 0} texels (read by k_ref8's packed taps)
void launch_pyr_pack(const float *img, const float *dx, const float *dy, float *pack, size_t n, hipStream_t s);
// one pyramid level. src: the input frame (first, unpadded, stride w) or the previous level's padded image plane
// (pw x ph, stride psw)
void launch_pyr_level(const float *src, int first, int pw, int ph, int psw, float *img, float *dx, float *dy, float *pack,
                      int w, int h, int pad, int sw, int sh, int getgrad, hipStream_t s);
// K patches of P x P (and their gradient patches) around mids[2K]
void launch_getpatch(const float *img, const float *dx, const float *dy, const float *mids, int K, int P, int sw,
                     int dopatchnorm, float *out, float *out_dx, float *out_dy, hipStream_t s);
// weighted NCC of the patches of frame r against frames b (back) and f (forward) at mids[2K]
void launch_ncc(const float *img_b, const float *img_r, const float *img_f, const float *mids, int K, int P, int sw,
                float swo, float sho, float w_back, float w_fwd, float *out, hipStream_t s);
// func_get_transf_position: K points moved by a displacement field (H x W, f32 or f64) sampled bilinearly, in f64
void launch_flow_gather(const void *du, const void *dv, int is_f64, int H, int W, const double *xy, int K, double *out,
                        hipStream_t s);
// func_extract_bil_patch, batched: K raw (2 half x 2 half x C) bilinear patches of an (H, W, C) f64 image
void launch_bil_patches(const double *img, int H, int W, int C, const double *pts, int K, int half, double *out,
                        hipStream_t s);
// n points of a cloud of capacity M through the pose G[12] and the level camera; pt3d_rot (may be NULL): the rotated points
void launch_project_generic(const float *pt3d, float *pt3d_rot, float *pt2d, int n, int M, const float *G, LevelCam lc,
                            hipStream_t s);
// step 3 for every problem and level (and clears the trace counter); cams[e.nlev]
void launch_project_ref(const EngineDev &e, const LevelCam *cams, int maxpts, hipStream_t s);
// deferred H: the level's H partials are reduced and factored by the level's first iteration tail, not by the level tail
bool defer_h(const EngineDev &e, int variant);
// partials per problem that the tail behind an accumulate launch of this geometry adds
int tail_partials(const EngineDev &e, const LevelLaunch &ll);
// steps 4-6 of one level for every problem: accumulate kernel + per-problem tail. tail = false (the resident form on the
// 8x8 fast path): no tail, the resident-iteration launch that follows reduces and factors H itself
void launch_ref_level(const EngineDev &e, const LevelCam &lc, const LevelLaunch &ll, bool tail, hipStream_t s);
// sharded phase API: the level's solve on the summed record
void launch_level_finish(const EngineDev &e, const LevelLaunch &ll, hipStream_t s);
// steps 7-9a of one Gauss-Newton iteration for every problem (the accumulate kernel). first: the level's first iteration;
// ev0 / ev1 (optional, timing runs): HIP events that take the kernel's own start and end time stamps
void launch_iter_main(const EngineDev &e, const LevelCam &lc, const LevelLaunch &ll, int first, hipStream_t s,
                      hipEvent_t ev0, hipEvent_t ev1);
// ... and steps 9b-10 (one workgroup per problem)
void launch_iter_tail(const EngineDev &e, const LevelLaunch &ll, int first, hipStream_t s);
// sharded phase API: the iteration's solve and update on the summed record
void launch_iter_finish(const EngineDev &e, const LevelLaunch &ll, int first, hipStream_t s);
// inspection: WaveSolver on n systems, one wave each; through_state: factors stored in st by one launch, reloaded by a second
hipError_t launch_debug_wave_solve(const float *H, const float *b, int n, ProbState *st, int through_state, float *x,
                                   int *rank, int *nonzero, int *rowmap, int *colmap, float *lu, hipStream_t s);
// inspection: the device builds of se3_exp<float> / se3_log<float> on n inputs
hipError_t launch_debug_se3(const float *in, float *out, long long n, int log_not_exp, hipStream_t s);

// ---------------------------------------------------------------- ictr_track1.hip
// dynamic LDS bytes of a k_track1 workgroup; *tmpl_lds: 0 when the templates do not fit and stay in device memory
size_t track1_plan(int npts_cap, int n, int p8, int waves, int *tmpl_lds);
// bytes of initial state + plane table a launch can carry in its arguments (fused begin)
size_t track1_blob_bytes(void);
// points per workgroup of the team form for a problem of maxpts points, and with it the team size: functions of the
// point count alone
int track1_team_q(int maxpts, int target);
int track1_team_size(int maxpts, int target);
// ONE launch for the whole tracking of every problem. blob (may be NULL): [ProbState x B][PlaneSet x B x nlev] for the
// fused begin; host_st (may be NULL): pinned mirror of the final records; project_here (without a blob): the records and
// the plane table have been uploaded, the launch projects (step 3) itself; tm (may be NULL): team form; any_size:
// ICTR_VARIANT_ANY_SIZE, 8x8 patches in the any-size form k_track1 too (a robustness option takes them there anyway)
hipError_t launch_track1(const EngineDev &e, const LevelCam *cams, int maxpts, int waves, const void *blob,
                         ProbState *host_st, hipStream_t s, const T1Team *tm, bool project_here = false,
                         bool any_size = false);

// ---------------------------------------------------------------- ictr_resident.hip
int resident_points_per_workgroup(int np);
int resident_blocks_per_cu(int np);  // workgroups of the kernel that one CU holds at once (0: the kernel cannot run)
// all iterations of one level in ONE launch, (g.parts + 1) * g.slots workgroups that must all be resident. nblk: H partials
// per problem left by the level's setup launch (tail_partials); xchg (may be NULL): sums over the ranks inside the launch
hipError_t launch_level_resident(const EngineDev &e, const LevelCam &lc, int level, const ResidentGeom &g, int nblk,
                                 const Exchange &x, const ResXchg *xchg, hipStream_t s);
// inspection: the transposing wave reduction alone, np = 16 or 32 patches per wave
hipError_t launch_debug_transpose_reduce(const float *vals, float *out, int *patch_of_lane, int *kind_of_lane, int np,
                                         hipStream_t s);
// inspection: the half-window fetch path alone (one wave, eight windows of a plane of ntexels floats, row stride sw)
hipError_t launch_debug_half_window(const float *plane, int ntexels, int sw, const int *top_left, float *out, hipStream_t s);

// ---------------------------------------------------------------- ictr_sequence.hip, ictr_ransac.hip, ictr_fsplit.hip, ictr_patchflow.hip
// the between-pairs step (three launches), or with a.tail the last frame's bookkeeping (one)
void launch_seq_select(const SeqArgs &a, hipStream_t s);
// one chunk of a.k trials: hypotheses and scoring (tile = 16 / 32 / 64 hypotheses per workgroup) ...
void launch_ransac_hyp_score(const RansacArgs &a, int tile, hipStream_t s);
// ... and the same followed by the ordered selection
void launch_ransac_chunk(const RansacArgs &a, int tile, hipStream_t s);
// after the last chunk: inl_cnt and the post-filter
void launch_ransac_finish(const RansacArgs &a, hipStream_t s);
// one chunk of a.k trials of the static split: fits and scoring (tile = 16 / 32 / 64 trials per workgroup) ...
void launch_fsplit_fit_score(const FsplitArgs &a, int tile, hipStream_t s, hipEvent_t after_fit = nullptr);
// ... the chunk's best trial against the best so far ...
void launch_fsplit_select(const FsplitArgs &a, hipStream_t s);
// ... and after the last chunk the distances and inlier bits of the winner
void launch_fsplit_mask(const FsplitArgs &a, hipStream_t s);
// per-patch translation IC-LK, all levels, a.K points
void launch_patchflow(const PFArgs &a, hipStream_t s);
// NPL * 10 + WPP of this thread's last launch_patchflow (11, 41, 161 or 82), 0 before the first
int patchflow_last_form();
// the 1-D (x only) search of a rectified stereo pair on the same arguments; its form (11, 41 or 82) likewise
void launch_patchdisp(const PFArgs &a, hipStream_t s);
int patchdisp_last_form();
// the argument checks of a patch tracking and its level table; the point buffers and a->K stay the caller's
int patchflow_args(const ictr_pyramid *pa, const ictr_pyramid *pb, int psz, int lv_f, int lv_l, int maxiter, float eps,
                   PFArgs *a);

}  // namespace ictr
