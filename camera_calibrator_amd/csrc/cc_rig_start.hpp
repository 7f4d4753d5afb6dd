#pragma once
#include "cc_common.hpp"

// cc_rig_start.hpp / cc_rig_start.hip -- EXTENSION: start poses of a rig problem from its own observations
// (cc_rig_estimate_start): camera_T_rig of every camera and rig_T_world of every frame, closed form, on the device.
// The reference takes its start from OpenCV solvePnP in a helper package outside the library; a caller of cc_rig_* had to bring
// poses. A VIEW is one (frame, camera) group of the handle -- the index the sweeps already use.
//   k_rig_start_view     one wave per view: centroid, scale and scatter of the world points; planar views by a homography in the
//                        board's own basis, general views by a 3 x 4 DLT (Gram on the staged f64 matrix contraction, null vector
//                        by inverse iteration); then Levenberg-Marquardt on the view's six pose coordinates
//   (host)               spanning tree over the cameras' co-visible valid views (cc_rig_tree.hpp)
//   k_rig_start_edge     one wave per (child, parent) edge: inverse-variance weighted mean of the relative poses
//   k_rig_start_compose  one lane: camera poses composed along the tree, parents first
//   k_rig_start_frame    one wave per frame: weighted mean of the frame pose over its valid views of placed cameras
// The kernels are a translation unit of their own (cc_rig_start_dev.hpp has their text); cc_rig.hip launches them through the
// functions declared here.

namespace cc {

enum { RIG_VIEW_INVALID = 0, RIG_VIEW_PLANAR = 1, RIG_VIEW_GENERAL = 2 };
constexpr int kRigViewStride = 24;   // doubles per view: q(4) t(3) rms^2 R(9, row-major) -

struct RigStartDev {
  int64_t F, NG;
  int32_t C, CO;
  const float* uv;          // [N] float2 normalised image points, (frame, camera)-sorted
  const float* oxyz;        // [3N] world point of every observation
  const int64_t* goff;      // [NG+1] observation range of each view
  const int32_t* fslot;     // [F][CO] view of (frame, observed camera j), -1: none
  const int32_t* obs_cam;   // [CO] camera of observed camera j
  const int32_t* cobs;      // [C] observed index of a camera, -1: not observed
  double* view;             // [NG][kRigViewStride]
  int32_t* kind;            // [NG] RIG_VIEW_*
  const int32_t* edges;     // [C][2] child, parent, in the tree's order
  double* rel;              // [C][8] relative pose of each edge: q(4) t(3)
  const uint8_t* placed;    // [C]
  double* cam;              // [C][8] q(4) t(3): the caller's poses on entry, estimated cameras overwritten
  double* pose;             // [F][8] the same for the frames
  uint8_t* fplaced;         // [F] the frame had a valid view of a placed camera
};

void rig_start_enqueue_views(const RigStartDev& P, hipStream_t s, int refine_iterations);
// EXTENSION: stages V and R on float3 unit bearings [3N] in the order of the observations (cc_rigk_estimate_start_bearing;
// cc_rigk_start.hpp makes them). k_rig_start_view_bearing is k_rig_start_view restated: the closed form from b x (P y~) = 0, the
// refinement on the chord p / |p| - b, rms^2 = cost / (2 n); the record is the same, P.uv is not read. The bearings are an
// argument of their own: RigStartDev, and with it the other kernels' arguments, stays as it is. The kernel is a translation
// unit of its own (cc_rig_start_bearing.hip, text in cc_rig_start_bearing_dev.hpp).
void rig_start_enqueue_views_bearing(const RigStartDev& P, const float* bearing, hipStream_t s, int refine_iterations);
void rig_start_enqueue_poses(const RigStartDev& P, hipStream_t s, int n_edges);

}  // namespace cc
