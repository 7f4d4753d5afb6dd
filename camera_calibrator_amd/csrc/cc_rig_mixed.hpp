#pragma once
#include "cc_common.hpp"
#include "cc_rig_fisheye.hpp"

// cc_rig_mixed.hpp / cc_rig_mixed.hip -- EXTENSION: a pixel model PER CAMERA on one cc_rigk_* handle with a set of intrinsics per
// camera (cc_rigk_set_camera_model): a fisheye lens next to radial-tangential ones, refined jointly because they share the frame
// poses. A group is one (frame, camera) pair and a workgroup sweeps one group, so the model is uniform per workgroup; nothing
// behind the 16 x 16 group Gram knows it (cc_rig_fisheye.hpp). The unit holds
//   k_rig_sweep_adjk_sel<NW, MODEL>   k_rig_sweep_adjk_fisheye<NW> over a LIST of groups (g = glist[blockIdx.x]): the groups of
//                                     the cameras of one model. MODEL = CC_MODEL_RADTAN takes its rows from rigk_obs on the
//                                     normalised point, as k_rig_sweep_adjk forms them; everything else is the same text.
//                                     One launch per model that has a group, one after the other on the handle's stream
//   k_rig_obs_cost_mixed              k_rig_obs_cost_fisheye with a branch on the group's camera model
//   k_rigk_start_unproject_cam        k_rigk_start_unproject with the view's model from its camera
// The kernels of cc_rig.hip, cc_rig_fisheye.hip and cc_rigk_start.hip keep their text: a handle all of whose cameras have one
// model launches those, never these. There is no compact-record form: a mixed handle always sweeps into tiles.

namespace cc {

struct RigMixedDev {
  RigFishDev base;          // the handle's buffers (cc_rig.hip: rig_fish_dev)
  const int32_t* cmodel;    // [C] CC_MODEL_RADTAN / CC_MODEL_FISHEYE of every camera
  const int32_t* glist[2];  // the groups of the cameras of model m, ascending
  int32_t nlist[2];         // how many (0: no launch for that model)
};

// the sweep of the groups of the cameras of `model` (waves: 1 or 4 per workgroup); no launch when there is none. A sweep of all
// groups is one call per model, one after the other on the handle's stream
void rig_mixed_enqueue_sweep(const RigMixedDev& P, hipStream_t s, int waves, int model);
// per-observation robustified cost at buffer `cur`, sorted order
void rig_mixed_enqueue_obs_cost(const RigMixedDev& P, hipStream_t s, int cur, double* out);

// the pixel start's first kernel (cc_rigk_start.hpp) with the model of each view's camera
struct RigkStartCamDev {
  int64_t NG;
  const int32_t* cmodel;    // [C]
  const float* uv;          // [N] float2 pixel observations, (frame, camera)-sorted
  const int64_t* goff;      // [NG+1]
  const int32_t* gcam;      // [NG]
  const int32_t* kset;      // [C]
  const double* intr;       // [sets][16] start intrinsics
  float* out;               // [N] float2 normalised points, same order
};
void rigk_start_enqueue_unproject_cam(const RigkStartCamDev& P, hipStream_t s);

}  // namespace cc
