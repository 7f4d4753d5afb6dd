// cc_intr_start_batch.hip -- the kernels of the batched fisheye focal-length start (cc_intr_start_batch.hpp) as a code object of
// their own, and their launch.
#include "cc_intr_start_batch_dev.hpp"

namespace cc {

void intr_start_batch_enqueue(const IntrStartBatchDev& T, hipStream_t s, int refine_iterations) {
  (void)hipMemsetAsync(T.box, 0, (size_t)T.B * 8 * sizeof(unsigned long long), s);
  // (a batch without observations has no extent workgroup: the boxes stay zero, as a single problem's without pixels)
  if (T.E > 0) {
    hipLaunchKernelGGL(k_intrb_start_extent, dim3((unsigned)T.E), dim3(256), 0, s, T, 0);
    hipLaunchKernelGGL(k_intrb_start_extent, dim3((unsigned)T.E), dim3(256), 0, s, T, 1);
  }
  hipLaunchKernelGGL(k_intrb_start_extent, dim3((unsigned)T.B), dim3(64), 0, s, T, 2);
  hipLaunchKernelGGL(k_intrb_start_view, dim3((unsigned)T.Stot, (unsigned)T.C), dim3(64), 0, s, T, 0, refine_iterations);
  hipLaunchKernelGGL(k_intrb_start_pick, dim3((unsigned)T.B), dim3(64), 0, s, T);
  hipLaunchKernelGGL(k_intrb_start_view, dim3((unsigned)T.Ftot, 1), dim3(64), 0, s, T, 1, refine_iterations);
}

}  // namespace cc
