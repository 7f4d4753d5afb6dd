// cc_rig_start.hip -- the kernels of the rig start (cc_rig_start.hpp) as a code object of their own, and their launches.
#include "cc_rig_start_dev.hpp"

namespace cc {

void rig_start_enqueue_views(const RigStartDev& P, hipStream_t s, int refine_iterations) {
  if (P.NG > 0) hipLaunchKernelGGL(k_rig_start_view, dim3((unsigned)P.NG), dim3(64), 0, s, P, refine_iterations);
}

void rig_start_enqueue_poses(const RigStartDev& P, hipStream_t s, int n_edges) {
  if (n_edges > 0) {
    hipLaunchKernelGGL(k_rig_start_edge, dim3((unsigned)n_edges), dim3(64), 0, s, P, n_edges);
    hipLaunchKernelGGL(k_rig_start_compose, dim3(1), dim3(64), 0, s, P, n_edges);
  }
  if (P.F > 0) hipLaunchKernelGGL(k_rig_start_frame, dim3((unsigned)((P.F + 3) / 4)), dim3(256), 0, s, P);
}

}  // namespace cc
