#pragma once
#include "cc_common.hpp"

// cc_rigk_start.hpp / cc_rigk_start.hip -- EXTENSION: the rig start (cc_rig_start.hpp) for a cc_rigk_* handle, whose observations
// are PIXELS (cc_rigk_estimate_start). One kernel in front of the start's own:
//   k_rigk_start_unproject   one wave per view: every pixel of the view through the inverse of the handle's pixel model at the
//                            handle's START intrinsics (what cc_rigk_set_intrinsics / _set_camera_intrinsics last wrote), into a
//                            float2 normalised point; a pixel without a root gives NaN, NaN (the start then counts its view invalid)
// RigStartDev::uv is pointed at the kernel's output and the start's kernels, tree and host code run on it as they are.
// The pixel start's kernels are a translation unit of their own (cc_rigk_start_dev.hpp has their text); cc_rig.hip launches them
// through the functions declared here.

namespace cc {

struct RigkStartDev {
  int64_t NG;
  int32_t model;            // CC_MODEL_RADTAN / CC_MODEL_FISHEYE
  const float* uv;          // [N] float2 pixel observations, (frame, camera)-sorted
  const int64_t* goff;      // [NG+1] observation range of each view
  const int32_t* gcam;      // [NG] camera of each view
  const int32_t* kset;      // [C] intrinsics set of a camera (0 when shared)
  const double* intr;       // [sets][16] start intrinsics
  float* out;               // [N] float2 normalised points, same order
};

void rigk_start_enqueue_unproject(const RigkStartDev& P, hipStream_t s);

//   k_rigk_start_unproject_cam   the same with the model of each view's camera (CC_MODEL_MIXED)
struct RigkStartCamDev {
  int64_t NG;
  const int32_t* cmodel;    // [C] CC_MODEL_RADTAN / CC_MODEL_FISHEYE of every camera
  const float* uv;          // [N] float2 pixel observations, (frame, camera)-sorted
  const int64_t* goff;      // [NG+1]
  const int32_t* gcam;      // [NG]
  const int32_t* kset;      // [C]
  const double* intr;       // [sets][16] start intrinsics
  float* out;               // [N] float2 normalised points, same order
};
void rigk_start_enqueue_unproject_cam(const RigkStartCamDev& P, hipStream_t s);

// EXTENSION: the bearing form of the pixel start (cc_rigk_estimate_start_bearing), for points at and beyond 90 degrees off the
// axis, where x / z does not exist:
//   k_rigk_start_bearing        one wave per view, laid out like k_rigk_start_unproject: every pixel into a float3 UNIT bearing.
//                               radial-tangential: the same root (x, y), b = (x, y, 1) / |.|; fisheye: theta in [0, pi) by the
//                               same rule with the bracket's far end at the double below pi, b = (sin theta (xd, yd) / theta_d,
//                               cos theta), the axis exactly (0, 0, 1); no root: NaN x 3
//   k_rigk_start_bearing_cam    the same with the model of the view's camera (CC_MODEL_MIXED)
// k_rig_start_view_bearing (cc_rig_start.hpp) reads the bearings; the start's other kernels see per-view poses only.
struct RigkBearingDev {
  int64_t NG;
  int32_t model;            // CC_MODEL_RADTAN / CC_MODEL_FISHEYE; not read when cmodel is set
  const int32_t* cmodel;    // [C] model of every camera, or nullptr: one model
  const float* uv;          // [N] float2 pixel observations, (frame, camera)-sorted
  const int64_t* goff;      // [NG+1]
  const int32_t* gcam;      // [NG]
  const int32_t* kset;      // [C]
  const double* intr;       // [sets][16] start intrinsics
  float* out;               // [3N] unit bearings, same order
};

void rigk_start_enqueue_bearing(const RigkBearingDev& P, hipStream_t s);

}  // namespace cc
