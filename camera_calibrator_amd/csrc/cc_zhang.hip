// cc_zhang.hip -- Zhang's closed-form initialisation on the device: the step right before the LM
// hot path in Calibrator::Estimate (/root/reference/src/calibrator.cpp:47-66, geometry.cpp:70-203).
// The four kernels (k_zhang_gram, k_zhang_eig9, k_zhang_k, k_zhang_poses) and their device helpers are in
// cc_zhang_dev.hpp, which describes them; here: their launch sequence and the C entry point.
#include <vector>

#include "cc_common.hpp"
#include "cc_device.hpp"
#include "cc_zhang_dev.hpp"

namespace cc {
// The four kernels on arrays that are already on the device (cc_intrinsics_estimate: the handle's own copies), on
// `stream`. Scratch: gram double[F][256], H float[9F]; outputs K float[9], q float[4F], t float[3F] (device).
int zhang_on_device(hipStream_t stream, int64_t F, const int64_t* doff, const float* duv, const float* dxyz,
                    double* dgram, float* dH, float* dK, float* dq, float* dt) {
  hipLaunchKernelGGL(k_zhang_gram, dim3((unsigned)F), dim3(kZhangThreads), kZhangLdsBytes, stream, F, doff, duv, dxyz, dgram);
  hipLaunchKernelGGL(k_zhang_eig9, dim3((unsigned)((F + 63) / 64)), dim3(64), 0, stream, F, dgram, dH);
  hipLaunchKernelGGL(k_zhang_k, dim3(1), dim3(256), 0, stream, F, dH, dK);
  hipLaunchKernelGGL(k_zhang_poses, dim3((unsigned)((F + 63) / 64)), dim3(64), 0, stream, F, dH, dK, dq, dt);
  CC_HIP(hipGetLastError());
  return CC_OK;
}
}  // namespace cc

extern "C" int cc_zhang_init(int32_t device, int64_t F, const int64_t* off, const float* uv, const float* xyz,
                             float* K9, float* q_wxyz, float* t_xyz, float* homographies) {
  using namespace cc;
  if (F < 3 || !off || !K9) return fail(CC_ERR_BAD_ARGUMENT, "cc_zhang_init: needs >= 3 frames");
  if (off[0] != 0) return fail(CC_ERR_BAD_ARGUMENT, "frame_offsets[0] must be 0");
  for (int64_t f = 0; f < F; ++f)
    if (off[f + 1] - off[f] < 4) return fail(CC_ERR_BAD_ARGUMENT, "cc_zhang_init: frame %lld has fewer than 4 points", (long long)f);
  const int64_t N = off[F];
  if (F >= ((int64_t)1 << 28) || N >= ((int64_t)1 << 40))   // launch grids are 32-bit
    return fail(CC_ERR_BAD_ARGUMENT, "cc_zhang_init: problem too large (frames < 2^28, observations < 2^40)");
  if (!uv || !xyz) return fail(CC_ERR_BAD_ARGUMENT, "cc_zhang_init: NULL arrays");
  if (int rc = select_device(device)) return rc;
  // one scratch arena (one hipMalloc / hipFree per call), 256-byte aligned pieces
  ArenaCursor cur;
  const size_t o_uv = cur.take((size_t)N * 2 * sizeof(float)), o_xyz = cur.take((size_t)N * 3 * sizeof(float));
  const size_t o_off = cur.take((size_t)(F + 1) * sizeof(int64_t)), o_gram = cur.take((size_t)F * 256 * sizeof(double));
  const size_t o_H = cur.take((size_t)F * 9 * sizeof(float)), o_K = cur.take(9 * sizeof(float));
  const size_t o_q = cur.take((size_t)F * 4 * sizeof(float)), o_t = cur.take((size_t)F * 3 * sizeof(float));
  char* arena = nullptr;
  struct Release {  // frees the scratch arena on every exit path
    char** p;
    ~Release() { if (*p) hipFree(*p); }
  } release{&arena};
  CC_HIP(hipMalloc(&arena, cur.bytes));
  float* duv = reinterpret_cast<float*>(arena + o_uv);
  float* dxyz = reinterpret_cast<float*>(arena + o_xyz);
  int64_t* doff = reinterpret_cast<int64_t*>(arena + o_off);
  double* dgram = reinterpret_cast<double*>(arena + o_gram);
  float* dH = reinterpret_cast<float*>(arena + o_H);
  float* dK = reinterpret_cast<float*>(arena + o_K);
  float* dq = reinterpret_cast<float*>(arena + o_q);
  float* dt = reinterpret_cast<float*>(arena + o_t);
  CC_HIP(hipMemcpy(duv, uv, (size_t)N * 2 * sizeof(float), hipMemcpyHostToDevice));
  CC_HIP(hipMemcpy(dxyz, xyz, (size_t)N * 3 * sizeof(float), hipMemcpyHostToDevice));
  CC_HIP(hipMemcpy(doff, off, (size_t)(F + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  if (int rc = zhang_on_device(nullptr, F, doff, duv, dxyz, dgram, dH, dK, dq, dt)) return rc;
  CC_HIP(hipMemcpy(K9, dK, 9 * sizeof(float), hipMemcpyDeviceToHost));
  if (q_wxyz) CC_HIP(hipMemcpy(q_wxyz, dq, (size_t)F * 4 * sizeof(float), hipMemcpyDeviceToHost));
  if (t_xyz) CC_HIP(hipMemcpy(t_xyz, dt, (size_t)F * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (homographies) CC_HIP(hipMemcpy(homographies, dH, (size_t)F * 9 * sizeof(float), hipMemcpyDeviceToHost));
  return CC_OK;
}
