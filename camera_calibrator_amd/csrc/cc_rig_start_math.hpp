// cc_rig_start_math.hpp -- the device helpers of the rig start's view kernels (cc_rig_start_dev.hpp, cc_rig_start_bearing_dev.hpp):
// inline functions only, no kernel, so that more than one translation unit can include it.
#pragma once

#include "cc_rig_start.hpp"
#include "cc_device.hpp"
#include "cc_eigen_dev.hpp"

namespace cc {

constexpr double kPlanarTol = 1e-3;   // singular-value ratio at which OpenCV's iterative PnP takes its planar branch

// (lane 0's copy through the cross-lane network into a VECTOR register: v_readlane would put the LM sums -- 28 doubles, twice --
// into scalar registers, which the kernel does not have)
__device__ __forceinline__ double wsum0(double v) { return __shfl(wave_sum(v), 0, 64); }
__device__ __forceinline__ double wmin0(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return __shfl(v, 0, 64);
}

// R (R^T R)^-1/2, the rotation next to a near-rotation (FixRotationMatrix of the reference, as k_zhang_poses has it)
__device__ __forceinline__ void start_fix_rotation(double (&R)[3][3]) {
  double S[3][3], V[3][3], M[3][3], O[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) S[i][j] = R[0][i] * R[0][j] + R[1][i] * R[1][j] + R[2][i] * R[2][j];
  jacobi_eigen<3>(S, V, 10);
  const double i0 = 1.0 / sqrt(S[0][0]), i1 = 1.0 / sqrt(S[1][1]), i2 = 1.0 / sqrt(S[2][2]);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) M[i][j] = V[i][0] * V[j][0] * i0 + V[i][1] * V[j][1] * i1 + V[i][2] * V[j][2] * i2;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) O[i][j] = R[i][0] * M[0][j] + R[i][1] * M[1][j] + R[i][2] * M[2][j];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[i][j] = O[i][j];
}

// unit quaternion (w first) of a rotation matrix, row-major: Shepperd's method, the four cases written out
__device__ __forceinline__ void start_quat_of(const double* R, double* q) {
  const double tr = R[0] + R[4] + R[8];
  double w, x, y, z;   // (scalars, not q[] in four orders: the merged branches would index the array dynamically, through scratch)
  if (tr > 0.0) {
    const double s = sqrt(tr + 1.0), h = 0.5 / s;
    w = 0.5 * s; x = (R[7] - R[5]) * h; y = (R[2] - R[6]) * h; z = (R[3] - R[1]) * h;
  } else if (R[0] >= R[4] && R[0] >= R[8]) {
    const double s = sqrt(R[0] - R[4] - R[8] + 1.0), h = 0.5 / s;
    x = 0.5 * s; w = (R[7] - R[5]) * h; y = (R[3] + R[1]) * h; z = (R[6] + R[2]) * h;
  } else if (R[4] >= R[8]) {
    const double s = sqrt(R[4] - R[8] - R[0] + 1.0), h = 0.5 / s;
    y = 0.5 * s; w = (R[2] - R[6]) * h; z = (R[7] + R[5]) * h; x = (R[1] + R[3]) * h;
  } else {
    const double s = sqrt(R[8] - R[0] - R[4] + 1.0), h = 0.5 / s;
    z = 0.5 * s; w = (R[3] - R[1]) * h; x = (R[2] + R[6]) * h; y = (R[5] + R[7]) * h;
  }
  q[0] = w; q[1] = x; q[2] = y; q[3] = z;
}

// exp(w) R (Rodrigues), row-major
__device__ __forceinline__ void start_rotate(const double* w, const double* R, double* O) {
  const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double a, b;   // sin(th) / th, (1 - cos(th)) / th^2
  if (th2 < 1e-16) { a = 1.0; b = 0.5; }
  else { const double th = sqrt(th2); a = sin(th) / th; const double sh = sin(0.5 * th); b = 2.0 * sh * sh / th2; }
  double E[9];
  E[0] = 1.0 - b * (w[1] * w[1] + w[2] * w[2]); E[1] = -a * w[2] + b * w[0] * w[1]; E[2] = a * w[1] + b * w[0] * w[2];
  E[3] = a * w[2] + b * w[0] * w[1]; E[4] = 1.0 - b * (w[0] * w[0] + w[2] * w[2]); E[5] = -a * w[0] + b * w[1] * w[2];
  E[6] = -a * w[1] + b * w[0] * w[2]; E[7] = a * w[0] + b * w[1] * w[2]; E[8] = 1.0 - b * (w[0] * w[0] + w[1] * w[1]);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) O[i * 3 + j] = E[i * 3] * R[j] + E[i * 3 + 1] * R[3 + j] + E[i * 3 + 2] * R[6 + j];
}

// (H + lambda diag H) d = -g, H as packed upper triangle (row-major, 21): 6 x 6 Cholesky in registers
__device__ __forceinline__ bool start_solve6(const double (&H)[21], const double (&g)[6], double lambda, double (&d)[6]) {
  double A[6][6], L[6][6], y[6];
  {
    int e = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) { A[i][j] = H[e]; A[j][i] = H[e]; ++e; }
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double dj = A[j][j] + lambda * A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) dj -= L[j][k] * L[j][k];
    ok = ok && dj > 0.0 && isfinite(dj);
    const double r = 1.0 / sqrt(dj);
    L[j][j] = r;   // the reciprocal of the pivot
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double a = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) a -= L[i][k] * L[j][k];
      L[i][j] = a * r;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double a = -g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) a -= L[i][k] * y[k];
    y[i] = a * L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double a = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) a -= L[k][i] * d[k];
    d[i] = a * L[i][i];
  }
  return ok;
}

// Gauss-Newton sums of one view at the pose (R, t): residual x/z - u, y/z - v, update R <- exp(w) R, t <- t + d.
// H: packed upper triangle of J^T J, g = J^T r, cost = sum of squared residuals, minz = smallest depth. Wave-uniform on return.
__device__ __forceinline__ void start_view_sums(const float2* uv2, const float* xyz, int64_t s0, int64_t s1, int lane, const double* R,
                                                const double* t, double (&H)[21], double (&g)[6], double& cost, double& minz) {
#pragma unroll
  for (int e = 0; e < 21; ++e) H[e] = 0.0;
#pragma unroll
  for (int e = 0; e < 6; ++e) g[e] = 0.0;
  cost = 0.0;
  minz = 1e300;
  for (int64_t i = s0 + lane; i < s1; i += 64) {
    const double X0 = xyz[i * 3], X1 = xyz[i * 3 + 1], X2 = xyz[i * 3 + 2];
    const float2 m = uv2[i];
    const double px = R[0] * X0 + R[1] * X1 + R[2] * X2, py = R[3] * X0 + R[4] * X1 + R[5] * X2, pz = R[6] * X0 + R[7] * X1 + R[8] * X2;
    const double zc = pz + t[2], iz = 1.0 / zc;
    const double x = (px + t[0]) * iz, y = (py + t[1]) * iz;
    const double r0 = x - (double)m.x, r1 = y - (double)m.y;
    const double J0[6] = {-x * iz * py, iz * (pz + x * px), -iz * py, iz, 0.0, -x * iz};
    const double J1[6] = {-iz * (pz + y * py), y * iz * px, iz * px, 0.0, iz, -y * iz};
    int e = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int b = a; b < 6; ++b) { H[e] += J0[a] * J0[b] + J1[a] * J1[b]; ++e; }
      g[a] += J0[a] * r0 + J1[a] * r1;
    }
    cost += r0 * r0 + r1 * r1;
    minz = fmin(minz, zc);
  }
#pragma unroll
  for (int e = 0; e < 21; ++e) H[e] = wsum0(H[e]);
#pragma unroll
  for (int e = 0; e < 6; ++e) g[e] = wsum0(g[e]);
  cost = wsum0(cost);
  minz = wmin0(minz);
}

}  // namespace cc
