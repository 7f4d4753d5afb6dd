#pragma once
#include "cc_common.hpp"

// cc_rig_fisheye.hpp / cc_rig_fisheye.hip -- EXTENSION: the Kannala-Brandt / OpenCV `fisheye` camera model (cc_intrinsics_fisheye.hpp
// has the model and its slots: fx fy px py k1 k2 k3 k4 -) for the rig solve with intrinsics (cc_rigk_*, cc_rigk_set_model).
// The kernels are a translation unit of their own; cc_rig.hip launches them through the functions declared here.
//
// The rig path meets the pixel model in one place: per observation the sweep needs the residual, B = d r / d x_cam (2 x 3) and
// J_k (2 x 9). Everything behind the 16 x 16 Gram of X = [J_cam(6) r J_k(9)] -- the three tiles AA / AB / BB, the elimination,
// the reduced system, the update, the LM state machine -- does not know the model. So the unit holds
//   k_rig_sweep_adjk_fisheye<NW>   k_rig_sweep_adjk<NW> (cc_rig_sweeps.hpp) with the fisheye rows: same pose chain, same order of
//                                  the sums, same tiles and 320-double compact record; rows from the camera-frame point itself
//                                  (no division by the depth: the model lives beyond 90 degrees off the axis)
//   k_rig_obs_cost_fisheye         k_rig_obs_cost for the fisheye residual (cc_rig_get_state's per-observation costs)
// and nothing else. There is no compact-record form (k_rig_sweep_k2): a fisheye handle always sweeps into tiles.

namespace cc {

// what the kernels read of a rig handle (cc_rig.hip: RigDev, the same buffers)
struct RigFishDev {
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

// one sweep of all groups (waves: 1 or 4 per workgroup, the handle's choice as for k_rig_sweep_adjk)
void rig_fisheye_enqueue_sweep(const RigFishDev& P, hipStream_t s, int waves);
// per-observation robustified cost at buffer `cur`, sorted order
void rig_fisheye_enqueue_obs_cost(const RigFishDev& P, hipStream_t s, int cur, double* out);

}  // namespace cc
