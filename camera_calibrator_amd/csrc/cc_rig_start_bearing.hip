// cc_rig_start_bearing.hip -- stages V and R of the rig start on unit bearings (cc_rig_start.hpp) as a code object of their own,
// and their launch.
#include "cc_rig_start_bearing_dev.hpp"

namespace cc {

void rig_start_enqueue_views_bearing(const RigStartDev& P, const float* bearing, hipStream_t s, int refine_iterations) {
  if (P.NG > 0) hipLaunchKernelGGL(k_rig_start_view_bearing, dim3((unsigned)P.NG), dim3(64), 0, s, P, bearing, refine_iterations);
}

}  // namespace cc
