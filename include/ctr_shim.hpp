// ctr_shim.hpp -- header-only C++ facade: namespace CTR { optparam, CamClass, PoseClass, OdometerClass, util_* } with the
// reference's method names and argument order (camera.h:19-31, pose.h:18-40, odometer.h:21-30), implemented on the
// C-ABI of include/ictr.h. A driver written against the reference's classes (run_io_reprojection_test.cpp:189-223,
// run_track_nposes.cpp:185-259) compiles against this header after two mechanical edits that the missing OpenCV
// types force:
//   * util_constructpyramide(img, w, h, lv_f, getgrad, pad) returns a CTR::Pyramid (device resident) instead of
//     filling cv::Mat arrays (utilities.h:63-64);
//   * OdometerClass::SetPose takes (p_in, const Pyramid& ref, const Pyramid& cur); the literal
//     (p_in, img_ref, img_ref_dx, img_ref_dy, img_new) overload with host level-pointer arrays is kept as well.
// Errors: the reference ignores all of them; here a failing call throws std::runtime_error with ictr_last_error().
#pragma once

#include <stdexcept>
#include <string>

#include "ictr.h"

namespace CTR {

typedef ictr_optparam optparam;  // utilities.h:46-61, same fields

inline void check(int rc, const char *what) {
  if (rc != ICTR_OK) throw std::runtime_error(std::string(what) + ": " + ictr_last_error());
}

class Pyramid {
 public:
  Pyramid(const float *img, int w, int h, int lv_f, bool getgrad, int imgpadding) : h_(nullptr) {
    check(ictr_pyramid_create(&h_, img, w, h, lv_f, getgrad ? 1 : 0, imgpadding), "util_constructpyramide");
  }
  ~Pyramid() { ictr_pyramid_destroy(h_); }
  // the next frame of a sequence into the same planes (no allocation)
  void rebuild(const float *img) { check(ictr_pyramid_rebuild(h_, img, nullptr), "util_constructpyramide (rebuild)"); }
  Pyramid(const Pyramid &) = delete;
  Pyramid &operator=(const Pyramid &) = delete;
  const ictr_pyramid *handle() const { return h_; }

 private:
  ictr_pyramid *h_;
};

// utilities.cpp:14-52
inline Pyramid *util_constructpyramide(const float *img, int w, int h, int lv_f, bool getgrad, int imgpadding) {
  return new Pyramid(img, w, h, lv_f, getgrad, imgpadding);
}
// utilities.cpp:55-113 / 115-189: one psz x psz patch around mid = (x, y) of a pyramid level (bilinear, patch-constant
// weights; mean subtracted when op->dopatchnorm). The reference takes the level's padded plane and its row stride
// (`img_ao_pyr[i][level]`, `camobj.getsw(level)`); the device-resident Pyramid carries both, so the call names the
// level instead. `out` points at psz * psz floats, row-major (what the reference's Eigen::Map refers to).
inline void util_getPatch(const Pyramid &pyr, int level, const float *mid, float *out, const optparam *op) {
  check(ictr_get_patch(pyr.handle(), level, mid, 1, op->psz, op->dopatchnorm ? 1 : 0, out), "util_getPatch");
}
inline void util_getPatch_grad(const Pyramid &pyr, int level, const float *mid, float *out, float *out_dx, float *out_dy,
                               const optparam *op) {
  check(ictr_get_patch_grad(pyr.handle(), level, mid, 1, op->psz, op->dopatchnorm ? 1 : 0, out, out_dx, out_dy),
        "util_getPatch_grad");
}
// run_track_nposes.cpp:271-355 for all points of a pose sample at once (fetch, zero-mean, unit norm, the two dot
// products, the weighting and the validity tests on the device): mids = x_back[K] y_back[K] x_ref[K] y_ref[K] x_fwd[K]
// y_fwd[K] at `level`; out_corr[K]. A caller may also restate those lines literally on util_getPatch (tests/cxx/
// nposes_driver.cpp does both and compares).
inline void util_patchNCC(const Pyramid &back, const Pyramid &ref, const Pyramid &fwd, int level, const float *mids,
                          int npoints, const optparam *op, float w_back, float w_fwd, float *out_corr) {
  check(ictr_ncc_score(back.handle(), ref.handle(), fwd.handle(), level, mids, npoints, op->psz, w_back, w_fwd, out_corr),
        "util_patchNCC");
}
template <typename T> inline void util_SE3_coeff_to_group(T *G, const T *p);
template <> inline void util_SE3_coeff_to_group<float>(float *G, const float *p) { ictr_se3_coeff_to_group_f(G, p); }
template <> inline void util_SE3_coeff_to_group<double>(double *G, const double *p) { ictr_se3_coeff_to_group_d(G, p); }
template <typename T> inline void util_SE3_group_to_coeff(T *p, const T *G);
template <> inline void util_SE3_group_to_coeff<float>(float *p, const float *G) { ictr_se3_group_to_coeff_f(p, G); }
template <> inline void util_SE3_group_to_coeff<double>(double *p, const double *G) { ictr_se3_group_to_coeff_d(p, G); }

class CamClass {
 public:
  CamClass(const int noscales_in, const float *fc_in, const float *cc_in, const int *wh_in, const int padding_in)
      : h_(nullptr) {
    check(ictr_cam_create(&h_, noscales_in, fc_in, cc_in, wh_in, padding_in), "CamClass");
  }
  ~CamClass() { ictr_cam_destroy(h_); }
  CamClass(const CamClass &) = delete;
  CamClass &operator=(const CamClass &) = delete;
  float getfx(int sc) const { return ictr_cam_getfx(h_, sc); }
  float getfy(int sc) const { return ictr_cam_getfy(h_, sc); }
  float getcx(int sc) const { return ictr_cam_getcx(h_, sc); }
  float getcy(int sc) const { return ictr_cam_getcy(h_, sc); }
  float getswo(int sc) const { return ictr_cam_getswo(h_, sc); }
  float getsho(int sc) const { return ictr_cam_getsho(h_, sc); }
  float getsw(int sc) const { return ictr_cam_getsw(h_, sc); }
  float getsh(int sc) const { return ictr_cam_getsh(h_, sc); }
  const ictr_cam *handle() const { return h_; }

 private:
  ictr_cam *h_;
};

class PoseClass {
 public:
  PoseClass(const CamClass *camobj_in, const optparam *op_in) : camobj(camobj_in), h_(nullptr) {
    check(ictr_pose_create(&h_, camobj_in->handle(), op_in), "PoseClass");
  }
  ~PoseClass() { ictr_pose_destroy(h_); }
  PoseClass(const PoseClass &) = delete;
  PoseClass &operator=(const PoseClass &) = delete;
  // the reference passes an Eigen::Vector3d by value; any 3 contiguous doubles do here
  void setpose_se3(const double *p_in, const double *meanshift_in, const double varval_in) {
    check(ictr_pose_setpose_se3(h_, p_in, meanshift_in, varval_in), "setpose_se3");
  }
  void addpose_se3(const float *p_in) { check(ictr_pose_addpose_se3(h_, p_in), "addpose_se3"); }
  void subpose_se3(const float *p_in) { check(ictr_pose_subpose_se3(h_, p_in), "subpose_se3"); }
  void getPose_se3(double *p_out) const { check(ictr_pose_getpose_se3(h_, p_out), "getPose_se3"); }
  void project_pt(const float *pt3d, float *pt2d, int nopoints, int sc) const {
    check(ictr_pose_project_pt(h_, pt3d, pt2d, nopoints, sc), "project_pt");
  }
  void project_pt_save_rotated(const float *pt3d, float *pt3d_rot, float *pt2d, int nopoints, int sc) const {
    check(ictr_pose_project_pt_save_rotated(h_, pt3d, pt3d_rot, pt2d, nopoints, sc), "project_pt_save_rotated");
  }
  const CamClass *camobj;  // public member in the reference too (pose.h:40)
  ictr_pose *handle() const { return h_; }

 private:
  ictr_pose *h_;
};

class OdometerClass {
 public:
  OdometerClass(PoseClass *pose_in, const optparam *op_in) : h_(nullptr) {
    check(ictr_odometer_create(&h_, pose_in->handle(), op_in), "OdometerClass");
  }
  ~OdometerClass() { ictr_odometer_destroy(h_); }
  OdometerClass(const OdometerClass &) = delete;
  OdometerClass &operator=(const OdometerClass &) = delete;
  void Set3Dpoints(double *pt_in, const int nopoints_in) {
    check(ictr_odometer_set3dpoints(h_, pt_in, nopoints_in), "Set3Dpoints");
  }
  void SetPose(const double *p_in, const Pyramid &img_ref, const Pyramid &img_new) {
    check(ictr_odometer_setpose(h_, p_in, img_ref.handle(), img_new.handle()), "SetPose");
  }
  void SetPose(const double *p_in, const float **img_ref_in, const float **img_ref_dx_in, const float **img_ref_dy_in,
               const float **img_new_in) {
    check(ictr_odometer_setpose_host(h_, p_in, img_ref_in, img_ref_dx_in, img_ref_dy_in, img_new_in), "SetPose");
  }
  void TrackPose(double *p_out) { check(ictr_odometer_trackpose(h_, p_out), "TrackPose"); }
  const float *Get2DPoints() const { return ictr_odometer_get2dpoints(h_); }

 private:
  ictr_odometer *h_;
};

// Frame-to-frame sequence (run_odometer_test.m:172-250, ictr_sequence_* in include/ictr.h): every pair of a video tracked
// from the pose just found for the earlier frame, the step between pairs on the device; one read-back at the end.
class SequenceClass {
 public:
  SequenceClass(const CamClass *camobj_in, const optparam *op_in, int64_t nworld, int stride) : h_(nullptr) {
    check(ictr_sequence_create(&h_, camobj_in->handle(), op_in, nworld, stride), "SequenceClass");
  }
  ~SequenceClass() { ictr_sequence_destroy(h_); }
  SequenceClass(const SequenceClass &) = delete;
  SequenceClass &operator=(const SequenceClass &) = delete;
  void SetPoints(const double *pt3d /* SoA X..Y..Z.., nworld */) { check(ictr_sequence_set_points(h_, pt3d), "SetPoints"); }
  void SetFrames(const float *frames /* [N][h][w] */, int64_t nframes, int w, int h, bool on_device = false) {
    check(ictr_sequence_set_frames(h_, frames, nframes, w, h, on_device ? 1 : 0), "SetFrames");
  }
  void SetStream(void *hip_stream) { check(ictr_sequence_set_stream(h_, hip_stream), "SetStream"); }
  void TrackAsync(const double *p0) { check(ictr_sequence_track_async(h_, p0), "TrackAsync"); }
  void Wait(double *poses, int32_t *npts = nullptr, int32_t *iters = nullptr) {
    check(ictr_sequence_wait(h_, poses, npts, iters), "Wait");
  }
  int LastTeam() const { return ictr_sequence_last_team(h_); }

 private:
  ictr_sequence *h_;
};

// RANSAC pose sampling from 2-D/3-D matches (func_ransac_fitcameras_odom.m:17-87, ictr_ransac_* in include/ictr.h): the
// hypothesis stage on the device, one read-back at the end.
class RansacClass {
 public:
  RansacClass(int64_t n, int64_t max_samples) : h_(nullptr), n_(n), smax_(max_samples) {
    check(ictr_ransac_create(&h_, n, max_samples), "RansacClass");
  }
  ~RansacClass() { ictr_ransac_destroy(h_); }
  RansacClass(const RansacClass &) = delete;
  RansacClass &operator=(const RansacClass &) = delete;
  void SetPoints(const double *pt2d /* SoA x.. y.. */, const double *pt3d /* SoA X.. Y.. Z.. */) {
    check(ictr_ransac_set_points(h_, pt2d, pt3d), "SetPoints");
  }
  void Run(const double *fc, const double *cc, double kc, int64_t nsamples, int64_t maxtrials, double inlthresh,
           uint64_t seed = 0, void *hip_stream = nullptr) {
    check(ictr_ransac_run(h_, fc, cc, kc, nsamples, maxtrials, inlthresh, seed, hip_stream), "Run");
  }
  // counts[4] as ictr_ransac_wait; buffers sized for max_samples (inl_words: max_samples * WordsPerSample()) and N
  void Wait(int64_t *counts, double *R, double *t, double *p, uint64_t *inl_words, int32_t *inl_cnt) {
    check(ictr_ransac_wait(h_, counts, R, t, p, inl_words, inl_cnt), "Wait");
  }
  int64_t WordsPerSample() const { return (n_ + 63) / 64; }

 private:
  ictr_ransac *h_;
  int64_t n_, smax_;
};

class StereoTrackClass;
class CamRansacClass;

// Static / moving split of a track window (misc_src/run_test_OF_track.py:309-343, ictr_fsplit_* in include/ictr.h): RANSAC
// over 8-point fundamental matrices of several view pairs of the same points, one read-back at the end.
class StaticSplitClass {
 public:
  StaticSplitClass(int64_t n, int64_t npairs) : h_(nullptr), n_(n), npairs_(npairs) {
    check(ictr_fsplit_create(&h_, n, npairs), "StaticSplitClass");
  }
  ~StaticSplitClass() { ictr_fsplit_destroy(h_); }
  StaticSplitClass(const StaticSplitClass &) = delete;
  StaticSplitClass &operator=(const StaticSplitClass &) = delete;
  void SetPairs(const double *xy /* [npairs][4][n]: xa, ya, xb, yb */) { check(ictr_fsplit_set_pairs(h_, xy), "SetPairs"); }
  // the view pairs of a counted window, written on the device (needs n = Count(), npairs = 2 (Frames() / 2))
  inline void SetPairsFromWindow(const StereoTrackClass &win);
  ictr_fsplit *Handle() const { return h_; }
  void Run(int64_t ntrials, double thresh, uint64_t seed = 0, void *hip_stream = nullptr) {
    check(ictr_fsplit_run(h_, ntrials, thresh, seed, hip_stream), "Run");
  }
  // draws [8], F [npairs][9], inl_words [Words()], dd [n]; any may be NULL
  void Wait(int64_t *best_trial, int64_t *best_count, int32_t *draws, double *F, uint64_t *inl_words, double *dd) {
    check(ictr_fsplit_wait(h_, best_trial, best_count, draws, F, inl_words, dd), "Wait");
  }
  int64_t Words() const { return (n_ + 63) / 64; }
  int64_t Points() const { return n_; }
  int64_t Pairs() const { return npairs_; }

 private:
  ictr_fsplit *h_;
  int64_t n_, npairs_;
};

// One camera per frame of a track window (misc_src/run_test_OF_track.py:374-411, ictr_camfit_* in include/ictr.h):
// Levenberg-Marquardt on the reprojection error of the same points in every frame, one read-back at the end.
class CamFitClass {
 public:
  CamFitClass(int64_t n, int64_t nframes) : h_(nullptr), n_(n), nframes_(nframes) {
    check(ictr_camfit_create(&h_, n, nframes), "CamFitClass");
  }
  ~CamFitClass() { ictr_camfit_destroy(h_); }
  CamFitClass(const CamFitClass &) = delete;
  CamFitClass &operator=(const CamFitClass &) = delete;
  void SetPoints(const double *X /* [3][n] */) { check(ictr_camfit_set_points(h_, X), "SetPoints"); }
  void SetObservations(const double *xy /* [nframes][2][n] */) {
    check(ictr_camfit_set_observations(h_, xy), "SetObservations");
  }
  void SetMask(const uint64_t *words /* [Words()] or NULL: every point */) { check(ictr_camfit_set_mask(h_, words), "SetMask"); }
  void SetCamera(const double *fc, const double *cc) { check(ictr_camfit_set_camera(h_, fc, cc), "SetCamera"); }
  // points (after SetCamera; baseline: P1[0, 3] of the script) and one side's observations of a counted window, written
  // on the device (needs n = Count(), nframes = Frames()); the inlier words of a split's last run, waited for or in flight
  inline void SetPointsFromWindow(const StereoTrackClass &win, double baseline);
  inline void SetObservationsFromWindow(const StereoTrackClass &win, bool right = false);
  void SetMaskFromSplit(const StaticSplitClass &split, void *hip_stream = nullptr) {
    check(ictr_camfit_set_mask_from_fsplit(h_, split.Handle(), hip_stream), "SetMaskFromSplit");
  }
  // the winner's inlier words of a window camera RANSAC's last run, waited for or in flight
  inline void SetMaskFromRansac(const CamRansacClass &ransac, void *hip_stream = nullptr);
  // the schedule of triang.c:327
  void Run(const double *G0 /* [nframes][12] */, int32_t noiter = 20, double damp_init = 2.0, double damp_fct = 10.0,
           double minres = 1e-5, double maxdamp = 1e10, void *hip_stream = nullptr) {
    check(ictr_camfit_run(h_, G0, noiter, damp_init, damp_fct, minres, maxdamp, hip_stream), "Run");
  }
  // per frame: G [12], cost, damp, iters, status (ICTR_CAMFIT_*), n; any may be NULL
  void Wait(double *G, double *cost, double *damp, int32_t *iters, int32_t *status, int64_t *n) {
    check(ictr_camfit_wait(h_, G, cost, damp, iters, status, n), "Wait");
  }
  // per frame the mean reprojection distance at the poses G with dt [3] (NULL: zero) added to every translation
  void Reproject(const double *G, const double *dt, double *mean_err, int64_t *n = nullptr) {
    check(ictr_camfit_reproj(h_, G, dt, mean_err, n), "Reproject");
  }
  int64_t Words() const { return (n_ + 63) / 64; }
  int64_t Points() const { return n_; }
  int64_t Frames() const { return nframes_; }

 private:
  ictr_camfit *h_;
  int64_t n_, nframes_;
};

// Window bundle adjustment (item 3 of the list that ends misc_src/run_test_OF_track.py, ictr_ba_* in include/ictr.h): the
// poses of frames 1 .. nframes - 1 and the adjusted points moved together, one read-back at the end.
class BundleClass {
 public:
  BundleClass(int64_t n, int64_t nframes, int64_t nsides) : h_(nullptr), n_(n), nframes_(nframes), nsides_(nsides) {
    check(ictr_ba_create(&h_, n, nframes, nsides), "BundleClass");
  }
  ~BundleClass() { ictr_ba_destroy(h_); }
  BundleClass(const BundleClass &) = delete;
  BundleClass &operator=(const BundleClass &) = delete;
  void SetPoints(const double *X /* [3][n] */) { check(ictr_ba_set_points(h_, X), "SetPoints"); }
  void SetObservations(const double *xy /* [nsides][nframes][2][n] */) {
    check(ictr_ba_set_observations(h_, xy), "SetObservations");
  }
  void SetMask(const uint64_t *words /* [Words()] or NULL: every point */) { check(ictr_ba_set_mask(h_, words), "SetMask"); }
  void SetCamera(const double *fc, const double *cc) { check(ictr_ba_set_camera(h_, fc, cc), "SetCamera"); }
  void SetOffset(const double *offset /* [3]: P1[:, 3] of the script */) { check(ictr_ba_set_offset(h_, offset), "SetOffset"); }
  // points (after SetCamera), every side's observations of a counted window and a split's inlier words, on the device
  inline void SetPointsFromWindow(const StereoTrackClass &win, double baseline);
  inline void SetObservationsFromWindow(const StereoTrackClass &win);
  void SetMaskFromSplit(const StaticSplitClass &split, void *hip_stream = nullptr) {
    check(ictr_ba_set_mask_from_fsplit(h_, split.Handle(), hip_stream), "SetMaskFromSplit");
  }
  inline void SetMaskFromRansac(const CamRansacClass &ransac, void *hip_stream = nullptr);
  void Run(const double *G0 /* [nframes][12] */, int32_t noiter = 20, double damp_init = 2.0, double damp_fct = 10.0,
           double minres = 1e-5, double maxdamp = 1e10, void *hip_stream = nullptr) {
    check(ictr_ba_run(h_, G0, noiter, damp_init, damp_fct, minres, maxdamp, hip_stream), "Run");
  }
  // G [nframes][12], X [3][n], cost, damp, iters, status (ICTR_CAMFIT_*), n; any may be NULL
  void Wait(double *G, double *X, double *cost, double *damp, int32_t *iters, int32_t *status, int64_t *n) {
    check(ictr_ba_wait(h_, G, X, cost, damp, iters, status, n), "Wait");
  }
  int64_t Words() const { return (n_ + 63) / 64; }
  int64_t Points() const { return n_; }
  int64_t Frames() const { return nframes_; }
  int64_t Sides() const { return nsides_; }

 private:
  ictr_ba *h_;
  int64_t n_, nframes_, nsides_;
};

// Window camera RANSAC (item 1 of the list that ends misc_src/run_test_OF_track.py, ictr_camransac_* in include/ictr.h):
// one P3P draw per trial over all frames of a track window, scored in both cameras, one read-back at the end.
class CamRansacClass {
 public:
  CamRansacClass(int64_t n, int64_t nframes, int64_t nsides) : h_(nullptr), n_(n), nframes_(nframes), nsides_(nsides) {
    check(ictr_camransac_create(&h_, n, nframes, nsides), "CamRansacClass");
  }
  ~CamRansacClass() { ictr_camransac_destroy(h_); }
  CamRansacClass(const CamRansacClass &) = delete;
  CamRansacClass &operator=(const CamRansacClass &) = delete;
  void SetPoints(const double *X /* [3][n] */) { check(ictr_camransac_set_points(h_, X), "SetPoints"); }
  void SetObservations(const double *xy /* [nsides][nframes][2][n] */) {
    check(ictr_camransac_set_observations(h_, xy), "SetObservations");
  }
  void SetMask(const uint64_t *words /* [Words()] or NULL: every point */) { check(ictr_camransac_set_mask(h_, words), "SetMask"); }
  void SetCamera(const double *fc, const double *cc) { check(ictr_camransac_set_camera(h_, fc, cc), "SetCamera"); }
  void SetOffset(const double *offset /* [3]: P1[:, 3] of the script */) {
    check(ictr_camransac_set_offset(h_, offset), "SetOffset");
  }
  // points (after SetCamera) and every side's observations of a counted window, on the device
  inline void SetPointsFromWindow(const StereoTrackClass &win, double baseline);
  inline void SetObservationsFromWindow(const StereoTrackClass &win);
  const ictr_camransac *Handle() const { return h_; }
  void Run(int64_t ntrials, double thresh, uint64_t seed = 0, void *hip_stream = nullptr) {
    check(ictr_camransac_run(h_, ntrials, thresh, seed, hip_stream), "Run");
  }
  // draws [4], G [nframes][12], p [nframes][6], inl_words [Words()], dd [n]; any may be NULL. best_trial -1: no trial
  // succeeded
  void Wait(int64_t *best_trial, int64_t *best_count, int32_t *draws, double *G, double *p, uint64_t *inl_words,
            double *dd) {
    check(ictr_camransac_wait(h_, best_trial, best_count, draws, G, p, inl_words, dd), "Wait");
  }
  int64_t Words() const { return (n_ + 63) / 64; }
  int64_t Points() const { return n_; }
  int64_t Frames() const { return nframes_; }
  int64_t Sides() const { return nsides_; }

 private:
  ictr_camransac *h_;
  int64_t n_, nframes_, nsides_;
};

inline void CamFitClass::SetMaskFromRansac(const CamRansacClass &ransac, void *hip_stream) {
  check(ictr_camfit_set_mask_from_camransac(h_, ransac.Handle(), hip_stream), "SetMaskFromRansac");
}
inline void BundleClass::SetMaskFromRansac(const CamRansacClass &ransac, void *hip_stream) {
  check(ictr_ba_set_mask_from_camransac(h_, ransac.Handle(), hip_stream), "SetMaskFromRansac");
}

// The checked stereo track window (misc_src/run_test_OF_track.py:170-223, ictr_stereotrack_* in include/ictr.h): Open with
// the stereo fields of frame 0, Advance once per later frame, Count, Read. A field is an ictr_field; the helpers below
// fill one.
class StereoTrackClass {
 public:
  StereoTrackClass(int w, int h, int bsize, double th_ratio = 0.2, double th_abs = 1.0) : h_(nullptr), bsize_(bsize) {
    check(ictr_stereotrack_create(&h_, w, h, bsize, th_ratio, th_abs), "StereoTrackClass");
  }
  ~StereoTrackClass() { ictr_stereotrack_destroy(h_); }
  StereoTrackClass(const StereoTrackClass &) = delete;
  StereoTrackClass &operator=(const StereoTrackClass &) = delete;
  // a float32 plane [h][w] (moves x only) or interleaved flow [h][w][2], in host or device memory; sign +1 or -1
  static ictr_field Plane(const float *p, int sign = 1, bool on_device = false) {
    ictr_field f = {ICTR_FIELD_PLANE, sign, on_device ? 1 : 0, 1, p};
    return f;
  }
  static ictr_field Flow(const float *p, int sign = 1, bool on_device = false, bool x_only = false) {
    ictr_field f = {ICTR_FIELD_FLOW, sign, on_device ? 1 : 0, x_only ? 1 : 0, p};
    return f;
  }
  // a flow grid that holds a field; x_only for the stereo pair
  static ictr_field Grid(const ictr_flowgrid *g, bool x_only = false, int sign = 1) {
    ictr_field f = {ICTR_FIELD_GRID, sign, 1, x_only ? 1 : 0, g};
    return f;
  }
  // xy0 [n][2] or NULL: every pixel (n = 0). lr: the field that moves a left point to the right frame (the script's
  // -imgs_d[fr][0] is Plane(p, -1)), rl: the way back
  void Open(const double *xy0, int64_t n, const ictr_field &lr, const ictr_field &rl) {
    check(ictr_stereotrack_open(h_, xy0, n, &lr, &rl), "Open");
  }
  void Advance(const ictr_field &l_fwd, const ictr_field &l_bwd, const ictr_field &r_fwd, const ictr_field &r_bwd,
               const ictr_field &lr_next, const ictr_field &rl_next) {
    check(ictr_stereotrack_advance(h_, &l_fwd, &l_bwd, &r_fwd, &r_bwd, &lr_next, &rl_next), "Advance");
  }
  int64_t Count() {
    int64_t m = 0;
    check(ictr_stereotrack_count(h_, &m), "Count");
    return m;
  }
  // xy_t [Count()][4][bsize], rows [Count()]; either may be NULL
  void Read(double *xy_t, int64_t *rows) { check(ictr_stereotrack_read(h_, xy_t, rows), "Read"); }
  int Frames() const { return bsize_; }
  const ictr_stereotrack *Handle() const { return h_; }

 private:
  ictr_stereotrack *h_;
  int bsize_;
};

inline void StaticSplitClass::SetPairsFromWindow(const StereoTrackClass &win) {
  check(ictr_fsplit_set_pairs_from_window(h_, win.Handle()), "SetPairsFromWindow");
}
inline void CamFitClass::SetPointsFromWindow(const StereoTrackClass &win, double baseline) {
  check(ictr_camfit_set_points_from_window(h_, win.Handle(), baseline), "SetPointsFromWindow");
}
inline void CamFitClass::SetObservationsFromWindow(const StereoTrackClass &win, bool right) {
  check(ictr_camfit_set_observations_from_window(h_, win.Handle(), right ? 1 : 0), "SetObservationsFromWindow");
}
inline void BundleClass::SetPointsFromWindow(const StereoTrackClass &win, double baseline) {
  check(ictr_ba_set_points_from_window(h_, win.Handle(), baseline), "SetPointsFromWindow");
}
inline void BundleClass::SetObservationsFromWindow(const StereoTrackClass &win) {
  check(ictr_ba_set_observations_from_window(h_, win.Handle()), "SetObservationsFromWindow");
}
inline void CamRansacClass::SetPointsFromWindow(const StereoTrackClass &win, double baseline) {
  check(ictr_camransac_set_points_from_window(h_, win.Handle(), baseline), "SetPointsFromWindow");
}
inline void CamRansacClass::SetObservationsFromWindow(const StereoTrackClass &win) {
  check(ictr_camransac_set_observations_from_window(h_, win.Handle()), "SetObservationsFromWindow");
}

// Multi-view point triangulation (misc_src/triang.c, ictr_triang_* in include/ictr.h): a whole track set per launch, one
// read-back at the end. Mode: ICTR_TRIANG_DLT / _GN / _LM / _DEPTH.
class TriangClass {
 public:
  TriangClass(int64_t max_points, int64_t max_obs, int64_t max_frames) : h_(nullptr) {
    check(ictr_triang_create(&h_, max_points, max_obs, max_frames), "TriangClass");
  }
  ~TriangClass() { ictr_triang_destroy(h_); }
  TriangClass(const TriangClass &) = delete;
  TriangClass &operator=(const TriangClass &) = delete;
  void SetCameras(const float *P /* [F][12] */, int64_t nframes) {
    check(ictr_triang_set_cameras(h_, P, nframes), "SetCameras");
  }
  void SetTracks(int64_t n, const int64_t *offsets /* [n + 1] */, const int32_t *view, const float *x, const float *y) {
    check(ictr_triang_set_tracks(h_, n, offsets, view, x, y), "SetTracks");
  }
  void Run(int mode, const ictr_triang_params *params = nullptr, const float *init_pts = nullptr,
           const float *campos = nullptr, const float *ptdir = nullptr, void *hip_stream = nullptr) {
    check(ictr_triang_run(h_, mode, params, init_pts, campos, ptdir, hip_stream), "Run");
  }
  // buffers sized for the tracks set: pts [n][3], cov [n][9], iters [n], status [n]; any may be NULL
  void Wait(float *pts, float *cov, int32_t *iters = nullptr, int32_t *status = nullptr) {
    check(ictr_triang_wait(h_, pts, cov, iters, status), "Wait");
  }

 private:
  ictr_triang *h_;
};

// The point-track front end (ictr_pointtrack_* in include/ictr.h): the loop of misc_src/run_OF_point_track.py.ipynb on the
// device. Push the frames in order; block b (opened by the pair b, b + 1) is read back when it is wanted.
class PointTrackClass {
 public:
  PointTrackClass(int w, int h, int bsize, int maxcorners, int lv_f, int psz, int step, int maxiter = 10, float eps = 0.01f,
                  double quality = 0.001, int mindist = 5, int win = 3, double th_ratio = 0.2, double th_abs = 1.0)
      : h_(nullptr), bsize_(bsize), maxcorners_(maxcorners) {
    check(ictr_pointtrack_create(&h_, w, h, bsize, maxcorners, lv_f, psz, step, maxiter, eps, quality, mindist, win, th_ratio,
                                 th_abs),
          "PointTrackClass");
  }
  ~PointTrackClass() { ictr_pointtrack_destroy(h_); }
  PointTrackClass(const PointTrackClass &) = delete;
  PointTrackClass &operator=(const PointTrackClass &) = delete;
  void PushFrame(const float *img /* [h][w] */) { check(ictr_pointtrack_push_frame(h_, img), "PushFrame"); }
  int64_t FrameCounter() const {
    int64_t n = 0;
    check(ictr_pointtrack_frcounter(h_, &n), "FrameCounter");
    return n;
  }
  // buffers sized for maxcorners rows: tracks [.][2][bsize], valid [.], absmovement [.]; any may be NULL. Returns the rows.
  int ReadBlock(int64_t block, float *tracks, uint8_t *valid, double *absmovement) {
    int n = 0;
    check(ictr_pointtrack_read_block(h_, block, tracks, valid, absmovement, &n), "ReadBlock");
    return n;
  }
  int BlockSize() const { return bsize_; }
  int MaxCorners() const { return maxcorners_; }

 private:
  ictr_pointtrack *h_;
  int bsize_, maxcorners_;
};

// Variational refinement of a dense flow field at level 0 (ictr_flowrefine_* in include/ictr.h). Run enqueues, Result
// waits. A field is an ictr_field (StereoTrackClass::Flow / Grid fill one); Field() is this object's refined field on the
// device, for the stereo track window.
class FlowRefineClass {
 public:
  FlowRefineClass(int w, int h) : h_(nullptr) { check(ictr_flowrefine_create(&h_, w, h), "FlowRefineClass"); }
  ~FlowRefineClass() { ictr_flowrefine_destroy(h_); }
  FlowRefineClass(const FlowRefineClass &) = delete;
  FlowRefineClass &operator=(const FlowRefineClass &) = delete;
  void SetParams(float alpha = 16.0f, float gamma = 13.0f, float delta = 4.5f, int n_outer = 8, int n_sor = 5,
                 float omega = 1.6f) {
    check(ictr_flowrefine_set_params(h_, alpha, gamma, delta, n_outer, n_sor, omega), "SetParams");
  }
  void Run(const Pyramid &a, const Pyramid &b, const ictr_field &src, bool x_only = false, void *hip_stream = nullptr) {
    check(ictr_flowrefine_run(h_, a.handle(), b.handle(), &src, x_only ? 1 : 0, hip_stream), "Run");
  }
  // out [h][w][2], in host memory or (on_device) device memory
  void Result(float *out, bool on_device = false) { check(ictr_flowrefine_result(h_, out, on_device ? 1 : 0), "Result"); }
  ictr_field Field(bool x_only = false) const {
    ictr_field f = {ICTR_FIELD_FLOW, 1, 1, x_only ? 1 : 0, ictr_flowrefine_device_ptr(h_)};
    return f;
  }
  // which: 0 Bw, 1..5 a11 a12 a22 b1 b2, 6 7 the edge weights, 8 9 du dv, 10 11 u v of the last outer iteration; out [h][w]
  void ReadStage(int which, float *out) { check(ictr_flowrefine_read_stage(h_, which, out), "ReadStage"); }

 private:
  ictr_flowrefine *h_;
};

// Photometric densification of a flow grid at level 0 (ictr_flowdensify_* in include/ictr.h). Run enqueues, Result waits.
// Field() is this object's field on the device, for FlowRefineClass::Run and the stereo track window.
class FlowDensifyClass {
 public:
  FlowDensifyClass(int w, int h) : h_(nullptr) { check(ictr_flowdensify_create(&h_, w, h), "FlowDensifyClass"); }
  ~FlowDensifyClass() { ictr_flowdensify_destroy(h_); }
  FlowDensifyClass(const FlowDensifyClass &) = delete;
  FlowDensifyClass &operator=(const FlowDensifyClass &) = delete;
  void SetParams(float minerr = 2.0f, int power = 1) { check(ictr_flowdensify_set_params(h_, minerr, power), "SetParams"); }
  // grid: an ictr_flowgrid that holds a field, tracked a -> b with patches of psz
  void Run(const ictr_flowgrid *grid, const Pyramid &a, const Pyramid &b, int psz, void *hip_stream = nullptr) {
    check(ictr_flowdensify_run(h_, grid, a.handle(), b.handle(), psz, hip_stream), "Run");
  }
  // out [h][w][2], in host memory or (on_device) device memory
  void Result(float *out, bool on_device = false) { check(ictr_flowdensify_result(h_, out, on_device ? 1 : 0), "Result"); }
  ictr_field Field(bool x_only = false) const {
    ictr_field f = {ICTR_FIELD_FLOW, 1, 1, x_only ? 1 : 0, ictr_flowdensify_device_ptr(h_)};
    return f;
  }
  // which: 0 the votes a pixel took, 1 their summed weight; out [h][w]
  void ReadStage(int which, float *out) { check(ictr_flowdensify_read_stage(h_, which, out), "ReadStage"); }

 private:
  ictr_flowdensify *h_;
};

// Coarse-to-fine dense flow: search, densification and optional refinement per pyramid level (ictr_c2fflow_* in
// include/ictr.h). Run enqueues, Result and ReadLevel wait. Field() is level 0's field on the device, for
// FlowRefineClass::Run and the stereo track window.
class CoarseFlowClass {
 public:
  // lv_l: the finest level (ictr_c2fflow_create_lvl); above 0 the runs stop there and Result / Field are that level's field
  // up-sampled to w x h
  CoarseFlowClass(int w, int h, int lv_f, int step = 4, int psz = 8, int lv_l = 0) : h_(nullptr) {
    check(ictr_c2fflow_create_lvl(&h_, w, h, lv_f, lv_l, step, psz), "CoarseFlowClass");
  }
  int LvL() const {
    int lv_l = 0;
    check(ictr_c2fflow_get_lv_l(h_, &lv_l), "LvL");
    return lv_l;
  }
  ~CoarseFlowClass() { ictr_c2fflow_destroy(h_); }
  CoarseFlowClass(const CoarseFlowClass &) = delete;
  CoarseFlowClass &operator=(const CoarseFlowClass &) = delete;
  void SetParams(int maxiter = 10, float eps = 0.01f, float minerr = 2.0f, int power = 1) {
    check(ictr_c2fflow_set_params(h_, maxiter, eps, minerr, power), "SetParams");
  }
  void SetRefine(bool on, float alpha = 16.0f, float gamma = 13.0f, float delta = 4.5f, int n_outer = 8, int n_sor = 5,
                 float omega = 1.6f) {
    check(ictr_c2fflow_set_refine(h_, on ? 1 : 0, alpha, gamma, delta, n_outer, n_sor, omega), "SetRefine");
  }
  // patch-mean normalisation of the next runs (ictr_c2fflow_set_patnorm); default off
  void SetPatnorm(bool on) { check(ictr_c2fflow_set_patnorm(h_, on ? 1 : 0), "SetPatnorm"); }
  // the 1-D form of the next runs, for a rectified stereo pair (ictr_c2fflow_set_x_only): v is +0.0; default off
  void SetXOnly(bool on) { check(ictr_c2fflow_set_x_only(h_, on ? 1 : 0), "SetXOnly"); }
  bool XOnly() const {
    int on = 0;
    check(ictr_c2fflow_get_x_only(h_, &on), "XOnly");
    return on != 0;
  }
  // the patch cost of the next runs (ictr_c2fflow_set_cost): ICTR_C2F_COST_L2 (default) or ICTR_C2F_COST_HUBER, which clips
  // every residual of the search to [-huber_k, +huber_k] grey levels. Cost 1 (L1), unknown codes and a huber_k that is not
  // finite and > 0 throw, and the object stays as it was.
  void SetCost(int cost, float huber_k = 5.0f) { check(ictr_c2fflow_set_cost(h_, cost, huber_k), "SetCost"); }
  void GetCost(int *cost, float *huber_k) const { check(ictr_c2fflow_get_cost(h_, cost, huber_k), "GetCost"); }
  // a, b: pyramids of the object's size with levels 0 .. lv_f, padded by at least psz, a with gradient planes
  void Run(const Pyramid &a, const Pyramid &b, void *hip_stream = nullptr) {
    check(ictr_c2fflow_run(h_, a.handle(), b.handle(), hip_stream), "Run");
  }
  // out [h][w][2], in host memory or (on_device) device memory
  void Result(float *out, bool on_device = false) { check(ictr_c2fflow_result(h_, out, on_device ? 1 : 0), "Result"); }
  ictr_field Field(bool x_only = false) const {
    ictr_field f = {ICTR_FIELD_FLOW, 1, 1, x_only ? 1 : 0, ictr_c2fflow_device_ptr(h_)};
    return f;
  }
  void LevelDims(int level, int *w, int *h, int *nx, int *ny) const {
    check(ictr_c2fflow_level_dims(h_, level, w, h, nx, ny), "LevelDims");
  }
  // field [h_l][w_l][2], d [ny][nx][2] after the fill, status [ny][nx]; any pointer may be NULL
  void ReadLevel(int level, float *field, float *d, unsigned char *status) {
    check(ictr_c2fflow_read_level(h_, level, field, d, status), "ReadLevel");
  }
  // bias [ny][nx]: the node bias of a run with patch-mean normalisation
  void ReadLevelBias(int level, float *bias) { check(ictr_c2fflow_read_level_bias(h_, level, bias), "ReadLevelBias"); }
  // Colour frames (ictr.h, "colour (three-channel) frames"): n = 1 or 3, before the first run. With 3 a frame is three pyramids, one per
  // channel and equal in geometry, the run is RunRGB and the node bias has three values per node.
  void SetChannels(int n) { check(ictr_c2fflow_set_channels(h_, n), "SetChannels"); }
  int Channels() const {
    int n = 0;
    check(ictr_c2fflow_get_channels(h_, &n), "Channels");
    return n;
  }
  void RunRGB(const Pyramid *const a[3], const Pyramid *const b[3], void *hip_stream = nullptr) {
    const ictr_pyramid *pa[3] = {a[0]->handle(), a[1]->handle(), a[2]->handle()};
    const ictr_pyramid *pb[3] = {b[0]->handle(), b[1]->handle(), b[2]->handle()};
    check(ictr_c2fflow_run_rgb(h_, pa, pb, hip_stream), "RunRGB");
  }
  // bias [ny][nx][3]
  void ReadLevelBiasRGB(int level, float *bias) {
    check(ictr_c2fflow_read_level_bias_rgb(h_, level, bias), "ReadLevelBiasRGB");
  }
  ictr_c2fflow *handle() const { return h_; }  // for CoarseFlowSet

 private:
  ictr_c2fflow *h_;
};

// 1 .. ICTR_C2FSET_MAX CoarseFlowClass objects of equal shape and parameters run in lockstep, one launch per level and
// stage for all of them (ictr_c2fset_* in include/ictr_c2f_set.h): Run leaves every member as its own Run on its pair would
// have, bit for bit. The members are the caller's and outlive the set; a refused call throws with the library's message,
// which names the member and the field.
class CoarseFlowSet {
 public:
  CoarseFlowSet(CoarseFlowClass *const *members, int n) : h_(nullptr), n_(n) {
    ictr_c2fflow *m[ICTR_C2FSET_MAX] = {};
    for (int i = 0; i < n && i < ICTR_C2FSET_MAX; ++i) m[i] = members[i] ? members[i]->handle() : nullptr;
    check(ictr_c2fset_create(&h_, m, n), "CoarseFlowSet");
  }
  ~CoarseFlowSet() { ictr_c2fset_destroy(h_); }
  CoarseFlowSet(const CoarseFlowSet &) = delete;
  CoarseFlowSet &operator=(const CoarseFlowSet &) = delete;
  int Size() const {
    int n = 0;
    check(ictr_c2fset_size(h_, &n), "Size");
    return n;
  }
  // a[m], b[m]: member m's frames (grey members)
  void Run(const Pyramid *const *a, const Pyramid *const *b, void *hip_stream = nullptr) {
    const ictr_pyramid *pa[ICTR_C2FSET_MAX], *pb[ICTR_C2FSET_MAX];
    for (int i = 0; i < n_; ++i) pa[i] = a[i]->handle(), pb[i] = b[i]->handle();
    check(ictr_c2fset_run(h_, pa, pb, hip_stream), "CoarseFlowSet::Run");
  }
  // a[3 * m + ch], b[3 * m + ch]: channel ch of member m's frames (3-channel members)
  void RunRGB(const Pyramid *const *a, const Pyramid *const *b, void *hip_stream = nullptr) {
    const ictr_pyramid *pa[3 * ICTR_C2FSET_MAX], *pb[3 * ICTR_C2FSET_MAX];
    for (int i = 0; i < 3 * n_; ++i) pa[i] = a[i]->handle(), pb[i] = b[i]->handle();
    check(ictr_c2fset_run_rgb(h_, pa, pb, hip_stream), "CoarseFlowSet::RunRGB");
  }
  // kernel launches plus memsets of the last run: the same for any number of members
  int Operations() const {
    int ops = 0;
    check(ictr_c2fset_last_operations(h_, &ops), "Operations");
    return ops;
  }
  void SetTiming(bool on) { check(ictr_c2fset_set_timing(h_, on ? 1 : 0), "SetTiming"); }
  // ms [lv_f + 1][3], upsample_ms (may be NULL): ictr_c2fset_get_kernel_ms
  void KernelMs(float *ms, float *upsample_ms = nullptr) { check(ictr_c2fset_get_kernel_ms(h_, ms, upsample_ms), "KernelMs"); }

 private:
  ictr_c2fset *h_;
  int n_;
};

// A field of level lv of a w x h pyramid at the frame's size (ictr_flow_upsample): src [h_l][w_l][2], out [h][w][2], both
// in host memory (the call waits) or, on_device, both in device memory (enqueued on hip_stream).
inline void UpsampleFlow(const float *src, int w_l, int h_l, int lv, float *out, int w, int h, bool x_only = false,
                         bool on_device = false, void *hip_stream = nullptr) {
  check(ictr_flow_upsample(src, w_l, h_l, lv, out, w, h, x_only ? 1 : 0, on_device ? 1 : 0, hip_stream), "UpsampleFlow");
}

}  // namespace CTR
