// ictr_pose_hd.h -- the pose (de)normalisation of PoseClass::setpose_se3 / getPose_se3 (pose.cpp:25-113) on a handful of
// scalars, compiled from the same text for the host (SetPose / get_poses of the batched engine) and for the device
// (the between-pairs step of a sequence, ictr_sequence.hip), so that both sides round alike.
#pragma once

#include <string.h>

#include "se3_math.h"

namespace ictr {

// pose.cpp:25-76
ICTR_HD void host_setpose(bool donorm, const double *p_in, const double *ms, double varval, float *p_f, float *G_f) {
  double pn[6];
  memcpy(pn, p_in, sizeof(pn));
  if (donorm) {
    double G[12];
    se3_exp<double>(G, pn);
    double t[3];
    t[0] = -G[0] * G[3] - G[4] * G[7] - G[8] * G[11];
    t[1] = -G[1] * G[3] - G[5] * G[7] - G[9] * G[11];
    t[2] = -G[2] * G[3] - G[6] * G[7] - G[10] * G[11];
    t[0] = (t[0] - ms[0]) / varval;
    t[1] = (t[1] - ms[1]) / varval;
    t[2] = (t[2] - ms[2]) / varval;
    G[3] = -G[0] * t[0] - G[1] * t[1] - G[2] * t[2];
    G[7] = -G[4] * t[0] - G[5] * t[1] - G[6] * t[2];
    G[11] = -G[8] * t[0] - G[9] * t[1] - G[10] * t[2];
    se3_log<double>(pn, G);
  }
  for (int i = 0; i < 6; ++i) p_f[i] = (float)pn[i];
  se3_exp<float>(G_f, p_f);
}
// pose.cpp:79-113 (f32 G, f64 camera centre, f32 log: the reference's mixed precision is kept)
ICTR_HD void host_getpose(bool donorm, const float *p_f, const float *G_f, const double *ms, double varval,
                         double *p_out) {
  float pu[6];
  memcpy(pu, p_f, sizeof(pu));
  if (donorm) {
    float G[12];
    memcpy(G, G_f, sizeof(G));
    double t[3];
    t[0] = (double)(-G[0] * G[3] - G[4] * G[7] - G[8] * G[11]);
    t[1] = (double)(-G[1] * G[3] - G[5] * G[7] - G[9] * G[11]);
    t[2] = (double)(-G[2] * G[3] - G[6] * G[7] - G[10] * G[11]);
    t[0] = t[0] * varval + ms[0];
    t[1] = t[1] * varval + ms[1];
    t[2] = t[2] * varval + ms[2];
    G[3] = (float)(-G[0] * t[0] - G[1] * t[1] - G[2] * t[2]);
    G[7] = (float)(-G[4] * t[0] - G[5] * t[1] - G[6] * t[2]);
    G[11] = (float)(-G[8] * t[0] - G[9] * t[1] - G[10] * t[2]);
    se3_log<float>(pu, G);
  }
  for (int i = 0; i < 6; ++i) p_out[i] = (double)pu[i];
}

}  // namespace ictr
