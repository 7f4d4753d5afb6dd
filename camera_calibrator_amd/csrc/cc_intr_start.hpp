#pragma once
#include "cc_common.hpp"
#include "cc_rig_start.hpp"

// cc_intr_start.hpp / cc_intr_start.hip -- EXTENSION: a start of the single-camera FISHEYE solve from its own pixels
// (cc_intrinsics_estimate_start_fisheye): a search over the focal length of the equidistant lens r = f theta -- the fisheye
// model at k = 0, fx = fy = f -- on the bearing form of the rig start's stages V and R (cc_rig_start.hpp).
//   k_intr_start_extent  the bounding box of the finite pixels (the centre, unless the caller gives one) and r_max, their largest
//                        distance from the centre; then the candidates f_j = r_max / theta_j, theta_j evenly spaced
//   k_intr_start_view    grid (views, candidates), one wave each: the pixels of the view into fp64 bearings through candidate j,
//                        then the closed form from b x (P y~) = 0 and Levenberg-Marquardt on the chord p / |p| - b, the arithmetic
//                        of k_rig_start_view_bearing; the record of cc_rig_start.hpp with the chord cost in slot 17, the kind in slot 18
//   k_intr_start_pick    one wave: S_j = f_j^2 sum_v cost_{j,v} over the searched views in index order, the smallest wins
// and k_intr_start_view once more over all views at the picked candidate. The kernels are a translation unit of their own
// (cc_intr_start_dev.hpp has their text); cc_intrinsics.hip launches them through intr_start_enqueue.

namespace cc {

constexpr int kIntrStartMaxCandidates = 64;   // one lane of k_intr_start_pick each
constexpr int kIntrStartCostSlot = 17;        // of a view record: sum |p / |p| - b|^2 at the returned pose
constexpr int kIntrStartKindSlot = 18;        // ... and its RIG_VIEW_* as a double (an invalid view's record is all zeros)

struct IntrStartDev {
  int64_t F, N;
  int64_t S;                // searched views: view floor(k F / S), k = 0 .. S - 1 (1 <= S <= F)
  int32_t C;                // candidates, 1 .. kIntrStartMaxCandidates
  double centre[2];         // the caller's, or NaN: the midpoint of the bounding box
  double theta_lo, theta_hi;
  const int64_t* off;       // [F+1] observation range of each view
  const float* uv;          // [2N] pixels
  const float* xyz;         // [3N] board points
  unsigned long long* box;  // [8] order-preserving words under atomicMax: -min u, max u, -min v, max v, r_max; zeroed before the launch
  double* ext;              // [4] centre x, y, r_max, the picked f
  double* f;                // [kIntrStartMaxCandidates] candidates
  double* score;            // [kIntrStartMaxCandidates] S_j
  int32_t* qualified;       // [kIntrStartMaxCandidates]
  int32_t* best;            // [2] picked candidate (-1: none qualified), qualified candidates
  double* srec;             // [C][S][kRigViewStride] records of the search
  int32_t* skind;           // [C][S]
  double* view;             // [F][kRigViewStride] records at the picked candidate
  int32_t* kind;            // [F]
};

// Host checks both the single and the batched start make (cc_intr_start_host.hpp, cc_intr_start_batch_host.hpp), no device call.
inline int64_t intr_start_searched(const cc_intr_start_options& o, int64_t F) {
  return o.search_views <= 0 || o.search_views >= F ? F : (int64_t)o.search_views;
}

inline int intr_start_check(const cc_intr_start_options& o, const char* who) {
  if (o.candidates < 1 || o.candidates > kIntrStartMaxCandidates)
    return fail(CC_ERR_BAD_ARGUMENT, "%s: candidates must be in 1 .. %d", who, kIntrStartMaxCandidates);
  if (!(o.theta_lo > 0.0) || !(o.theta_hi < 3.14159265358979323846) || !(o.theta_hi >= o.theta_lo))
    return fail(CC_ERR_BAD_ARGUMENT, "%s: needs 0 < theta_lo <= theta_hi < pi", who);
  if (o.search_views < 0) return fail(CC_ERR_BAD_ARGUMENT, "%s: search_views must be >= 0 (0: every view)", who);
  if (o.refine_iterations < 0 || o.refine_iterations > 1000) return fail(CC_ERR_BAD_ARGUMENT, "%s: refine_iterations must be in 0 .. 1000", who);
  return CC_OK;
}

// Everything of one start on the stream, not waited for: extent, candidates, search, pick, pose pass. `marks` (may be NULL):
// four events recorded before the extent, after it, after the pick and after the pose pass.
void intr_start_enqueue(const IntrStartDev& P, hipStream_t s, int refine_iterations, hipEvent_t* marks);

}  // namespace cc
