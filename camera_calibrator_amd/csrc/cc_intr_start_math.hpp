// cc_intr_start_math.hpp -- the device helpers of the fisheye focal-length start (cc_intr_start.hpp) that its kernels
// (cc_intr_start_dev.hpp) and the batch's (cc_intr_start_batch_dev.hpp) share: the order-preserving words of the extent, the
// bearing of a pixel through the equidistant lens, the settled inverse iteration and the chord's Gauss-Newton sums. No kernel
// here: a kernel's text lives in the one unit that launches it.
#pragma once

#include "cc_intr_start.hpp"
#include "cc_rig_start_math.hpp"

namespace cc {

// ---- extent ---------------------------------------------------------------------------------------------------------------------
// A float as a word whose unsigned order is the float's order (finite values; -0 < +0), and back.
__device__ __forceinline__ unsigned long long start_order_word(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? (uint32_t)~u : (u | 0x80000000u);
}
__device__ __forceinline__ float start_order_float(unsigned long long w) {
  const uint32_t u = (uint32_t)w;
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// The centre: the caller's when both coordinates are finite, else the midpoint of the bounding box in P.box (NaN when no pixel
// is finite). Exact: a sum of two floats and a halving in fp64.
__device__ __forceinline__ void intr_start_centre(const IntrStartDev& P, double& cx, double& cy) {
  cx = P.centre[0]; cy = P.centre[1];
  if (isfinite(cx) && isfinite(cy)) return;
  const unsigned long long a = P.box[0], b = P.box[1], c = P.box[2], d = P.box[3];
  const double nan_ = __builtin_nan("");
  cx = b ? 0.5 * ((double)start_order_float(~a & 0xffffffffull) + (double)start_order_float(b)) : nan_;
  cy = d ? 0.5 * ((double)start_order_float(~c & 0xffffffffull) + (double)start_order_float(d)) : nan_;
}

// ---- one (view, candidate) pair -------------------------------------------------------------------------------------------------
// The equidistant lens r = f theta about (cx, cy): where the bearing of observation i comes from.
struct IntrStartLens {
  const float* uv;
  double cx, cy, f;
};
// d = uv - c, theta = |d| / f, b = (sin theta d / |d|, cos theta), in fp64 from the float32 pixel; the centre pixel is (0, 0, 1)
// exactly. |b| = 1 to rounding: I - b b^T is a projector as it is after start_bearing_of.
__device__ __forceinline__ void intr_start_bearing_of(const IntrStartLens& lens, int64_t i, double (&b)[3]) {
  const double d0 = (double)lens.uv[i * 2] - lens.cx, d1 = (double)lens.uv[i * 2 + 1] - lens.cy;
  const double r = sqrt(d0 * d0 + d1 * d1);
  const double th = r / lens.f;
  const double s = r > 0.0 ? sin(th) / r : 0.0;
  b[0] = s * d0; b[1] = s * d1; b[2] = r > 0.0 ? cos(th) : 1.0;
}

// smallest_eigvec (cc_eigen_dev.hpp) with shift 0, carried on until the vector stops moving: the same equilibrated Cholesky and
// the same twelve steps, then further ones while a step still moves the unit vector by more than 1e-14 (100 steps at most).
// Twelve steps rest on the smallest eigenvalue being noise-sized next to the second one. That holds with the lens's own
// intrinsics (the rig start), not with a candidate focal length that is far off: at theta_hi = 3.0 the ratio reaches 0.18 on
// the test's boards and twelve steps leave 0.18^12 = 1e-9 of the second eigenvector in the result (4e-10 rad in the pose, where
// the closed form's bound is 3e-12). A step gains the ratio, so the steps needed are 37 / -log10(ratio): 22 there, 100 cover 0.43
// to full precision; a candidate beyond that keeps what the steps gave it -- it is nowhere near winning the pick. Every lane
// holds the same numbers: the exit is wave-uniform.
template <int N>
__device__ __forceinline__ void smallest_eigvec_settled(const double (&A)[N][N], double (&x)[N]) {
  double sc[N];
#pragma unroll
  for (int i = 0; i < N; ++i) sc[i] = A[i][i] > 0.0 ? rsqrt(A[i][i]) : 1.0;
  double L[N][N], inv[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double d = sc[j] * A[j][j] * sc[j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    d = fmax(d, 1e-30);
    const double r = rsqrt(d);
    inv[j] = r;
    L[j][j] = d * r;
#pragma unroll
    for (int i = j + 1; i < N; ++i) {
      double a = sc[i] * A[i][j] * sc[j];
#pragma unroll
      for (int k = 0; k < j; ++k) a -= L[i][k] * L[j][k];
      L[i][j] = a * r;
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) x[i] = (i & 1) ? 0.7 : 1.0;   // not orthogonal to anything in particular
  for (int it = 0; it < 100; ++it) {
    double was[N];
#pragma unroll
    for (int i = 0; i < N; ++i) was[i] = x[i];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      double a = x[i] * sc[i];
#pragma unroll
      for (int k = 0; k < i; ++k) a -= L[i][k] * x[k];
      x[i] = a * inv[i];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
      double a = x[i];
#pragma unroll
      for (int k = i + 1; k < N; ++k) a -= L[k][i] * x[k];
      x[i] = a * inv[i];
    }
    double n2 = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) { x[i] *= sc[i]; n2 += x[i] * x[i]; }
    const double rn = rsqrt(n2);
    double moved = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) { x[i] *= rn; moved += (x[i] - was[i]) * (x[i] - was[i]); }
    if (it >= 11 && !(moved > 1e-28)) break;   // (A^-1 is positive definite: the iterates keep their sign; NaN ends it too)
  }
}

// start_view_sums_bearing (cc_rig_start_bearing_dev.hpp) overloaded on where the bearing comes from: the Gauss-Newton sums of one
// view at the pose (R, t) on the chord, residual p / |p| - b (three components), p = R X + t, the updates of start_view_sums.
// J = (I - ph ph^T) / |p| [ -[R X]x | I ]. Nothing is singular short of p = 0. Wave-uniform on return.
__device__ __forceinline__ void start_view_sums_bearing(const IntrStartLens& lens, const float* xyz, int64_t s0, int64_t s1, int lane,
                                                        const double* R, const double* t, double (&H)[21], double (&g)[6], double& cost) {
#pragma unroll
  for (int e = 0; e < 21; ++e) H[e] = 0.0;
#pragma unroll
  for (int e = 0; e < 6; ++e) g[e] = 0.0;
  cost = 0.0;
  for (int64_t i = s0 + lane; i < s1; i += 64) {
    const double X0 = xyz[i * 3], X1 = xyz[i * 3 + 1], X2 = xyz[i * 3 + 2];
    double b[3];
    intr_start_bearing_of(lens, i, b);
    const double q0 = R[0] * X0 + R[1] * X1 + R[2] * X2, q1 = R[3] * X0 + R[4] * X1 + R[5] * X2, q2 = R[6] * X0 + R[7] * X1 + R[8] * X2;
    const double p0 = q0 + t[0], p1 = q1 + t[1], p2 = q2 + t[2];
    const double il = 1.0 / sqrt(p0 * p0 + p1 * p1 + p2 * p2);
    const double h0 = p0 * il, h1 = p1 * il, h2 = p2 * il;
    const double r[3] = {h0 - b[0], h1 - b[1], h2 - b[2]};
    // M = (I - ph ph^T) / |p|, symmetric
    const double m00 = (1.0 - h0 * h0) * il, m01 = -h0 * h1 * il, m02 = -h0 * h2 * il, m11 = (1.0 - h1 * h1) * il, m12 = -h1 * h2 * il,
                 m22 = (1.0 - h2 * h2) * il;
    // column a of -[q]x is e_a x q: (0, -q2, q1), (q2, 0, -q0), (-q1, q0, 0)
    const double J[3][6] = {{-m01 * q2 + m02 * q1, m00 * q2 - m02 * q0, -m00 * q1 + m01 * q0, m00, m01, m02},
                            {-m11 * q2 + m12 * q1, m01 * q2 - m12 * q0, -m01 * q1 + m11 * q0, m01, m11, m12},
                            {-m12 * q2 + m22 * q1, m02 * q2 - m22 * q0, -m02 * q1 + m12 * q0, m02, m12, m22}};
    int e = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int c = a; c < 6; ++c) { H[e] += J[0][a] * J[0][c] + J[1][a] * J[1][c] + J[2][a] * J[2][c]; ++e; }
      g[a] += J[0][a] * r[0] + J[1][a] * r[1] + J[2][a] * r[2];
    }
    cost += r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
  }
#pragma unroll
  for (int e = 0; e < 21; ++e) H[e] = wsum0(H[e]);
#pragma unroll
  for (int e = 0; e < 6; ++e) g[e] = wsum0(g[e]);
  cost = wsum0(cost);
}

}  // namespace cc
