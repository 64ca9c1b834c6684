// ictr_wininputs.h -- the inputs every window stage takes (camera fit, bundle adjuster, window camera RANSAC), stated
// once: points X [3][n], observations xy [nsides][nframes][2][n], a word mask [ceil(n / 64)], one camera and the second
// side's offset, each with the flag that says it has been set. The object embeds one block; its public setters hand over
// their own name (`what`), the object's name for the in-flight message and its Readback, whose run fixes the inputs. The
// least n, the frame limits and whether there are sides are the object's own (its *_create). Host only; included by the
// three objects' files and by ictr_handover.hip, which reaches a block through the WinDest of ictr_launch.h.
#pragma once

#include <stdint.h>
#include <string.h>

#include "ictr_camfit_hd.h"
#include "ictr_own.h"

namespace ictr {

inline int null_object(const char *what) { return fail(ICTR_ERR_INVALID, "%s: NULL argument", what); }

struct WinInputs {
  int n = 0, nwords = 0, nframes = 0, nsides = 0;
  DevBuf<double> X, xy;
  DevBuf<unsigned long long> words;
  CfCam cam = {0, 0, 0, 0};
  double off[3] = {0, 0, 0};
  bool points_set = false, obs_set = false, cam_set = false, off_set = false, use_mask = false;

  size_t obs_count() const { return 2 * (size_t)nsides * (size_t)nframes * (size_t)n; }

  int alloc(int n_, int nframes_, int nsides_) {
    n = n_;
    nwords = (n_ + 63) / 64;
    nframes = nframes_;
    nsides = nsides_;
    if (int rc = X.alloc(sizeof(double) * 3 * (size_t)n, true)) return rc;
    if (int rc = xy.alloc(sizeof(double) * obs_count(), true)) return rc;
    return words.alloc(sizeof(unsigned long long) * (size_t)nwords, true);
  }

  int set_points(const char *what, const char *object, const Readback &out, const double *X_) {
    if (!X_) return null_object(what);
    if (int rc = out.refuse(what, object)) return rc;
    HIPCHK(hipMemcpy(X.get(), X_, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice));
    points_set = true;
    return ICTR_OK;
  }

  int set_observations(const char *what, const char *object, const Readback &out, const double *xy_) {
    if (!xy_) return null_object(what);
    if (int rc = out.refuse(what, object)) return rc;
    HIPCHK(hipMemcpy(xy.get(), xy_, sizeof(double) * obs_count(), hipMemcpyHostToDevice));
    obs_set = true;
    return ICTR_OK;
  }

  // NULL: every point
  int set_mask(const char *what, const char *object, const Readback &out, const uint64_t *w) {
    if (int rc = out.refuse(what, object)) return rc;
    if (w) HIPCHK(hipMemcpy(words.get(), w, sizeof(uint64_t) * (size_t)nwords, hipMemcpyHostToDevice));
    use_mask = w != nullptr;
    return ICTR_OK;
  }

  int set_camera(const char *what, const char *object, const Readback &out, const double *fc, const double *cc) {
    if (!fc || !cc) return null_object(what);
    if (int rc = out.refuse(what, object)) return rc;
    for (int q = 0; q < 2; ++q)
      if (!cf_finite(fc[q]) || !cf_finite(cc[q]) || fc[q] == 0.0)
        return fail(ICTR_ERR_INVALID, "%s: fc must be finite and not 0, cc finite", what);
    cam = {fc[0], fc[1], cc[0], cc[1]};
    cam_set = true;
    return ICTR_OK;
  }

  int set_offset(const char *what, const char *object, const Readback &out, const double *offset) {
    if (!offset) return null_object(what);
    if (int rc = out.refuse(what, object)) return rc;
    for (int q = 0; q < 3; ++q)
      if (!cf_finite(offset[q])) return fail(ICTR_ERR_INVALID, "%s: the offset is not finite", what);
    memcpy(off, offset, sizeof(off));
    off_set = true;
    return ICTR_OK;
  }

  // what every entry that launches needs first
  int ready(const char *what, const Readback &out, const char *object) const {
    if (int rc = out.refuse(what, object)) return rc;
    if (!points_set || !obs_set || !cam_set)
      return fail(ICTR_ERR_STATE, "%s: set_points, set_observations and set_camera come first", what);
    if (nsides == 2 && !off_set) return fail(ICTR_ERR_STATE, "%s: two sides need ictr_%s_set_offset", what, object);
    return ICTR_OK;
  }

  // the inputs a hand-over has filled on the device count as set (mask: the words are to be used)
  void filled(bool points, bool obs, bool mask) {
    points_set = points_set || points;
    obs_set = obs_set || obs;
    use_mask = use_mask || mask;
  }

  const unsigned long long *mask_or_null() const { return use_mask ? words.get() : nullptr; }
};

}  // namespace ictr
