// ictr_dev.h -- structures shared by the HIP kernels and the host-side ABI implementation.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ictr.h"
#include "ictr_xchg.h"

namespace ictr {

constexpr int kBlock = 256;        // threads per workgroup = 4 wave64
constexpr int kWaves = kBlock / 64;
constexpr int kCoefStride = 16;    // 12 steepest-descent coefficients per point, padded to one 64-B line
constexpr int kHUnique = 21;       // upper triangle of the 6x6 normal matrix
constexpr int kRedStride = 27;     // per problem: 21 (H) + 6 (b) in the reduction buffer
constexpr int kPartHStride = 32;   // per block partial of H (21 padded to 32)
constexpr int kPartBStride = 8;    // per block partial of b (6 padded)
constexpr int kMaxGridX = 2048;    // 256 CUs x 8 resident workgroups: cap, then grid-stride

// per pyramid level camera constants (camera.cpp:31-42), passed by value to the kernels
struct LevelCam {
  float fx, fy, cx, cy, swo, sho;
  int sw;  // padded row stride, (int)getsw(level) as the reference passes it (odometer.cpp:286)
};

// device pointers of the four planes one problem reads at one level
struct PlaneSet {
  const float *ref, *dx, *dy, *cur;
  const float *pack;  // optional: the reference level as one interleaved plane {img, dx, dy, 0} per pixel (k_ref8)
};

// per-problem state living in device memory for the whole coarse-to-fine loop
struct ProbState {
  float p[6];    // cpos_p  (pose.h:54)
  float G[12];   // cpos_G  (pose.h:53)
  float H[36];   // Hes     (odometer.h:62)
  float LU[36];  // full-pivot LU factors of H, computed once per level (H is constant across its iterations)
  int piv[12];   // 6 row + 6 column transpositions
  int luinfo[2]; // non-zero pivots, rank
  float b[6];    // sumsd
  float dp[6];   // delta_p
  float normdp;
  float normdp_init;
  int it;           // iteration counter of the current level
  int active;       // loop condition of odometer.cpp:344-346, evaluated on the device
  int total_iters;  // executed GN iterations, all levels
  int npts;         // nopoints of this problem
  unsigned reserved_;
  int pad_;
};

// Cross-GPU exchange inside the resident-iteration launch (ictr_resident.hip, "sharded resident form"): the mailboxes of
// an ictr_p2p object (ictr_p2p.hip: one per rank, hipIpc-mapped into every peer) as the kernel sees them. world == 1: off.
constexpr int kXchgMaxWorld = 16;
constexpr int kXchgPerPair = 64;  // granules per frame pair and rank: [0, 12) b as (hi, lo) pairs, [12, 33) H
struct ResXchg {
  unsigned long long *peer[kXchgMaxWorld];  // every rank's mailbox as mapped into this process (own rank: the local one)
  unsigned long long *local;
  int rank, world;
  long long cap;     // granules per (parity, rank) slot of a mailbox
  unsigned *xseq;    // [B] exchanges done so far per frame pair (device memory; every rank counts alike)
};

struct DevTrace {
  ictr_trace_rec *rec;
  int *count;
  int capacity;
  int reserved_;  // (explicit padding: EngineDev has none, the host's graph key compares its bytes)
};

// everything a kernel needs, passed by value (kernarg segment)
struct EngineDev {
  int B, M, P, n, nlev;  // nlev = lv_f+1
  int lv_f, lv_l, maxiter;
  float ratio;
  int dopatchnorm;
  int sharded;  // 1: accumulate kernels stop after writing rank-local sums to red[]
  int otf;      // every reference pyramid is builder-made (its gradients ARE the central differences of its image plane):
                // 1 = the 8x8 setup kernel may form them on the fly from the image plane; 2 = it must (some reference
                // pyramid is image-only: no dx / dy / packed planes exist); 0 = caller-supplied gradient planes.
                // Every reference pyramid carries the interleaved {img, dx, dy, 0} planes exactly when otf != 2.
  // behaviour-changing options, all off by default; any of them routes P = 8 through the
  // any-size kernels. ICTR_ROBUST_CLEAN: a point outside the reference view at a level contributes nothing (its
  // stale patches / gradients are zeroed instead of reused, cf. odometer.cpp:304); ICTR_ROBUST_COMPOSE: G <- exp(dp) G
  // instead of p += dp (pose.cpp:118-123); ICTR_ROBUST_HUBER: residuals weighted min(1, k / |r|) in J^T r.
  int robust;
  float huber_k;
  float *pt3d;      // [B][3M]  X..Y..Z..
  float *pt3d_ref;  // [B][3M]  camera-frame points at the reference pose
  float *pt2d;      // [B][nlev][2M]
  float *T, *Gx, *Gy;  // [B][M*n] patch-major, the reference's pat_ref_all / _dx_all / _dy_all
  float *coef;         // [B][M][16]
  ProbState *st;       // [B]
  const PlaneSet *planes;  // [B][nlev]
  float *partH;  // [B][gridx][32]
  float *partb;  // [B][gridx][8]
  float *red;    // [B][27]
  DevTrace trace;
};

// frame-to-frame sequence (ictr_sequence.hip): the between-pairs step on the device
constexpr int kSeqBlock = 256;                 // threads of the count / scatter workgroups
constexpr int kSeqPPT = 16;                    // world points per thread there
constexpr int kSeqChunk = kSeqBlock * kSeqPPT; // world points per workgroup (64 survivor masks)
constexpr int kSeqFinish = 256;                // threads of the one-workgroup finish
struct SeqState {       // carried from one pair to the next
  double pose[6];       // p_t of the pair being prepared (f64, as TrackPose returns it)
  double G[12];         // se3_exp<double>(p_t): the camera of the cull
  double ms[3], varval; // normalisation of the pair's selected points (Set3Dpoints)
  int npts;             // selected points of the pair (0: the pair is lost, its pose is carried)
  int pad_[3];
};
struct SeqArgs {
  const double *X;   // world points, SoA X[nw] Y[nw] Z[nw]
  long long nw;
  int nblk;          // workgroups of the count / scatter launches (kSeqChunk points each)
  int stride, cap, M, n, donorm;
  int t;             // pair t -> t+1 being prepared; t = N-1: finish-only (the last pose and pair N-2's iterations)
  int tail;
  double fx, fy, cx, cy, w, h;  // level-0 camera (f32 values) and the unpadded frame size
  double p0[6];      // pose of frame 0
  ProbState *st;     // the engine's record (B = 1): the previous pair's final state on entry, the next initial state out
  SeqState *ss;
  unsigned long long *mask;  // [nblk][kSeqChunk / 64] survivor bits, one word per wave and step
  unsigned *cnt;             // [nblk] survivors per workgroup
  int *sel;                  // [cap] world indices of the selected points
  double *poses;             // [N][6]
  unsigned long long *hash;  // [N-1] order-aware hash of each pair's selected indices
  int *npts_out, *iters_out; // [N-1]
  float *pt3d, *T, *Gx, *Gy, *coef;  // the engine's buffers (problem 0)
};

// RANSAC pose sampling from 2-D/3-D matches (ictr_ransac.hip)
constexpr int kRanHypBlock = 64;     // one lane per trial
constexpr int kRanScoreBlock = 256;  // four waves, one 64-match block each
constexpr int kRanSelBlock = 1024;   // the one-workgroup select / finish
struct RansacState {
  long long held;         // accepted samples so far (the script's successes, trial order)
  long long trials_used;  // trials the script would have consumed
  long long kept;         // samples after the post-filter
  long long n_ic;         // entries of the filtered inl_cnt
  int done;               // nsamples held or maxtrials reached: later chunks exit at once
  int pad_[3];
};
struct RansacArgs {
  const double *pts;      // SoA u[n] v[n] X[n] Y[n] Z[n] (f64)
  int n, nwords;          // matches, 64-bit inlier words per sample
  double fx, fy, cx, cy, kc, thr;
  unsigned long long seedmix;  // mix(seed)
  long long base;         // global index of the chunk's first trial
  int k;                  // trials of this chunk
  long long nsamples, maxtrials;
  double *hyp;            // [K][12]: R row-major, camera centre t
  int *draws;             // [K][4] drawn match indices, draw order
  int *status;            // [K] 1 = not degenerate and a P3P root chosen
  unsigned *cnt;          // [K] inliers
  unsigned long long *words;  // [K][nwords] inlier bits
  RansacState *st;
  long long *o_trial;     // [S] accepted trial indices
  int *o_draws;           // [S][4]
  double *o_R, *o_t;     // [S][9], [S][3]
  unsigned long long *o_words;  // [S][nwords]
  int *o_cnt;             // [n] inl_cnt: times each match is an inlier of an accepted sample
  int *o_keep;            // [S] accepted samples kept by the post-filter (ascending)
  int *o_cntf;            // [n] inl_cnt without the entries <= 4
};

// static / moving split of a track window by fundamental-matrix RANSAC (ictr_fsplit.hip)
constexpr int kFsFitBlock = 64;     // one lane per (trial, pair)
constexpr int kFsScoreBlock = 256;  // four waves, one 64-point block each
constexpr int kFsSelBlock = 1024;   // the one-workgroup select
constexpr int kFsTileMats = 320;    // matrices of a score workgroup's LDS tile (23040 B): 320 / T pairs of T trials
constexpr int kFsMaxPairs = 64;
struct FsplitState {
  long long best_trial, best_count;
  int draws[8];
};
struct FsplitArgs {
  const double *xy;     // [P][4][n]: xa, ya, xb, yb per pair (f64)
  int n, nwords, np;    // points, 64-bit inlier words, pairs
  double thr;
  unsigned long long seedmix;
  long long base;       // first trial of this chunk
  int k;                // trials in this chunk
  double *F;            // [K][np][9]; nine NaN where the fit failed
  int *draws;           // [K][8], -1 = not drawn
  int *pst;             // [K][np] 1 = the fit of this pair succeeded
  unsigned *cnt;        // [K] inliers
  FsplitState *st;      // the best trial so far ...
  double *o_F;          // ... its matrices [np][9]
  unsigned long long *o_words;  // [nwords] its inlier bits
  double *o_dd;         // [n] its distances
};

// per-patch translation IC-LK (ictr_patchflow.hip)
struct PFLevel {
  const float *a, *ax, *ay, *b;  // frame A image + gradients, frame B image (padded planes)
  int sw;
  int shift;  // (pad - P) * (sw + 1): pf_taps' base is the patch's corner in a plane padded by exactly P
  float swo, sho, scale;  // unpadded size, 0.5^level
};
struct PFArgs {
  PFLevel lv[16];
  int lv_f, lv_l, P, maxiter, K;
  float eps2;        // stop when |dp|^2 < eps2
  float min_det;     // relative conditioning threshold of the 2x2 system
  const float *pts;  // SoA x[K] y[K] at level 0
  float *out;        // SoA x'[K] y'[K] at level 0 (NaN when lost)
  int *status;       // 1 tracked, 0 lost
  int *iters;        // executed iterations (all levels)
  float min_hx;      // k_patchdisp: the patch is kept iff hxx > min_hx * (hxx + hyy)
};

// The argument block of a kernel of the coarse-to-fine flow (DESIGN.md §4 "Lockstep sets"): a stage's arguments once per
// member of a set of flows (a single object is a set of one), by value in the kernel arguments. A workgroup takes item
// m = its block index along the grid dimension the stage does not use: the index is uniform, so the item's fields come by
// scalar loads at a computed offset.
constexpr int kSetMax = 8;
constexpr size_t kKernargLimit = 4096;  // bytes of kernel arguments a launch may carry
template <class A>
struct SetArgs {
  A m[kSetMax];
};

}  // namespace ictr
