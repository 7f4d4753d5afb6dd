#pragma once
#include "cc_common.hpp"

// cc_rigk_start.hpp / cc_rigk_start.hip -- EXTENSION: the rig start (cc_rig_start.hpp) for a cc_rigk_* handle, whose observations
// are PIXELS (cc_rigk_estimate_start). One kernel in front of the start's own:
//   k_rigk_start_unproject   one wave per view: every pixel of the view through the inverse of the handle's pixel model at the
//                            handle's START intrinsics (what cc_rigk_set_intrinsics / _set_camera_intrinsics last wrote), into a
//                            float2 normalised point; a pixel without a root gives NaN, NaN (the start then counts its view invalid)
// RigStartDev::uv is pointed at the kernel's output and the start's kernels, tree and host code run on it as they are.
// The kernel is a translation unit of its own (cc_rigk_start_dev.hpp has its text); cc_rig.hip launches it through the function
// declared here.

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

}  // namespace cc
