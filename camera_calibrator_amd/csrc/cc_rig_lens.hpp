#pragma once
#include "cc_common.hpp"

// cc_rig_lens.hpp / cc_rig_lens.hip -- EXTENSION: the pixel models of the rig solve with intrinsics (cc_rigk_*) beyond the
// radial-tangential default: the Kannala-Brandt / OpenCV `fisheye` model (cc_intrinsics_fisheye.hpp has the model and its slots:
// fx fy px py k1 k2 k3 k4 -) for every camera of a handle (cc_rigk_set_model), or a model PER CAMERA on a handle with a set of
// intrinsics per camera (cc_rigk_set_camera_model): a fisheye lens next to radial-tangential ones, refined jointly because they
// share the frame poses. The kernels are a translation unit of their own; cc_rig.hip launches them through the functions
// declared here. The models' arithmetic is cc_rig_lens_dev.hpp.
//
// The rig path meets the pixel model in one place: per observation the sweep needs the residual, B = d r / d x_cam (2 x 3) and
// J_k (2 x 9). Everything behind the 16 x 16 Gram of X = [J_cam(6) r J_k(9)] -- the three tiles AA / AB / BB, the elimination,
// the reduced system, the update, the LM state machine -- does not know the model. A group is one (frame, camera) pair and a
// workgroup sweeps one group, so the model is uniform per workgroup. The unit holds
//   k_rig_sweep_lens<NW, MODEL, LIST>   k_rig_sweep_adjk<NW> (cc_rig_sweeps.hpp) with the rows of MODEL: same pose chain, same
//                                       order of the sums, same tiles and 320-double compact record. The fisheye rows come from
//                                       the camera-frame point itself (no division by the depth: the model lives beyond 90 degrees
//                                       off the axis), the radial-tangential ones from the normalised point as k_rig_sweep_adjk
//                                       forms them. LIST = false: workgroup b sweeps group b (a handle whose cameras are all
//                                       fisheye); LIST = true: group glist[b], the groups of the cameras of one model -- one
//                                       launch per model that has a group, one after the other on the handle's stream
//   k_rig_obs_cost_fisheye              k_rig_obs_cost for the fisheye residual (cc_rig_get_state's per-observation costs)
//   k_rig_obs_cost_mixed                the same with a branch on the model of the group's camera
// and nothing else. There is no compact-record form (k_rig_sweep_k2): these handles always sweep into tiles. A handle all of
// whose cameras are radial-tangential launches the kernels of cc_rig.hip, never these.

namespace cc {

// what the kernels read of a rig handle (cc_rig.hip: RigDev, the same buffers)
struct RigLensDev {
  int64_t F, NG;
  int32_t C, CK;
  const float* uv;          // [N] float2, (frame, camera)-sorted
  const float* oxyz;        // [3N] world point of every observation
  const int32_t* widx;      // [N] world point index
  const float* wxyz;        // [3P]
  const int64_t* goff;      // [NG+1]
  const int32_t* gframe;    // [NG]
  const int32_t* gcam;      // [NG]
  const uint8_t* cam_fixed; // [C]
  const int32_t* kset;      // [C] intrinsics set of the camera
  const uint32_t* kmask;    // [max(CK,1)] bit i: intrinsic i of the set is held constant
  const double* cam;        // [2][C][8]
  const double* pose;       // [2][F][8]
  const double* intr;       // [2][max(CK,1)][16]
  const double* camrec;     // [C][32] R(9) t(3) unscaled step(6)
  const double* frec;       // [F][32]
  const double* krec;       // [max(CK,1)][32] candidate intrinsics [0..8], unscaled step [16..24]
  double* gblocks;          // [2][NG][gstride] AA | AB | BB tiles
  double* gstats;           // [NG][2] cost, model term
  double* ghd0;             // [NG][8] diag of H_cc at the initial point
  double* ghdk;             // [NG][16] diag of H_kk at the initial point
  double* gcomp;            // [2][NG][320] 16-column Gram (256), M (36)
  const LmCtl* ctl;
  int32_t gstride;
  double huber_a;
  double huber_b, huber_2a;   // a^2, 2 a as KERNEL ARGUMENTS: scalar registers from the start (computed in the kernel they are vector
                              // results that the compiler keeps -- and spills -- across the passes; cf. RigDev)
};

// One launch of the sweep with the rows of `model` (waves: 1 or 4 per workgroup, the handle's choice as for k_rig_sweep_adjk).
// glist == nullptr: all P.NG groups (model must be CC_MODEL_FISHEYE); otherwise the n groups glist[0..n), ascending -- a sweep of
// all groups is then one call per model. n <= 0 launches nothing: a grid of zero workgroups is a launch error.
void rig_lens_enqueue_sweep(const RigLensDev& P, hipStream_t s, int waves, int model, const int32_t* glist, int n);
// per-observation robustified cost at buffer `cur`, sorted order. cmodel == nullptr: every camera is fisheye; otherwise [C]
// CC_MODEL_RADTAN / CC_MODEL_FISHEYE of every camera
void rig_lens_enqueue_obs_cost(const RigLensDev& P, hipStream_t s, const int32_t* cmodel, int cur, double* out);

}  // namespace cc
