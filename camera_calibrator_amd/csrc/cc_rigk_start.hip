// cc_rigk_start.hip -- the kernels of the pixel start (cc_rigk_start.hpp) as a code object of their own, and their launches.
#include "cc_rigk_start_dev.hpp"

namespace cc {

void rigk_start_enqueue_unproject(const RigkStartDev& P, hipStream_t s) {
  if (P.NG > 0) hipLaunchKernelGGL(k_rigk_start_unproject, dim3((unsigned)P.NG), dim3(64), 0, s, P);
}

void rigk_start_enqueue_unproject_cam(const RigkStartCamDev& P, hipStream_t s) {
  if (P.NG > 0) hipLaunchKernelGGL(k_rigk_start_unproject_cam, dim3((unsigned)P.NG), dim3(64), 0, s, P);
}

void rigk_start_enqueue_bearing(const RigkBearingDev& P, hipStream_t s) {
  if (P.NG <= 0) return;
  if (P.cmodel) hipLaunchKernelGGL(k_rigk_start_bearing_cam, dim3((unsigned)P.NG), dim3(64), 0, s, P);
  else hipLaunchKernelGGL(k_rigk_start_bearing, dim3((unsigned)P.NG), dim3(64), 0, s, P);
}

}  // namespace cc
