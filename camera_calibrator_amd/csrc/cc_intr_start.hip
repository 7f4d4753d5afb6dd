// cc_intr_start.hip -- the kernels of the fisheye focal-length start (cc_intr_start.hpp) as a code object of their own, and
// their launch.
#include "cc_intr_start_dev.hpp"

namespace cc {

void intr_start_enqueue(const IntrStartDev& P, hipStream_t s, int refine_iterations, hipEvent_t* marks) {
  if (marks) (void)hipEventRecord(marks[0], s);
  (void)hipMemsetAsync(P.box, 0, 8 * sizeof(unsigned long long), s);
  // (one pixel a thread up to 256 workgroups, one a compute unit, a grid-stride loop beyond: every workgroup ends in atomics on the
  // same few words, and the result does not depend on the grid)
  const unsigned blocks = (unsigned)std::min<int64_t>(256, std::max<int64_t>(1, (P.N + 255) / 256));
  hipLaunchKernelGGL(k_intr_start_extent, dim3(blocks), dim3(256), 0, s, P, 0);
  hipLaunchKernelGGL(k_intr_start_extent, dim3(blocks), dim3(256), 0, s, P, 1);
  hipLaunchKernelGGL(k_intr_start_extent, dim3(1), dim3(64), 0, s, P, 2);
  if (marks) (void)hipEventRecord(marks[1], s);
  hipLaunchKernelGGL(k_intr_start_view, dim3((unsigned)P.S, (unsigned)P.C), dim3(64), 0, s, P, 0, refine_iterations);
  hipLaunchKernelGGL(k_intr_start_pick, dim3(1), dim3(64), 0, s, P);
  if (marks) (void)hipEventRecord(marks[2], s);
  hipLaunchKernelGGL(k_intr_start_view, dim3((unsigned)P.F, 1), dim3(64), 0, s, P, 1, refine_iterations);
  if (marks) (void)hipEventRecord(marks[3], s);
}

}  // namespace cc
