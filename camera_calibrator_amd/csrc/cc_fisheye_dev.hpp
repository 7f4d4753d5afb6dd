// cc_fisheye_dev.hpp -- EXTENSION: the rows of the Kannala-Brandt / OpenCV `fisheye` model (cc_intrinsics_fisheye.hpp has the
// model and its slots), device helpers only, so that more than one translation unit can include them: the single-camera sweep
// (cc_intrinsics_fisheye.hpp, inside cc_intrinsics.hip) and the batch sweep (cc_intrinsics_batch_fisheye.hip).
#pragma once
#include "cc_common.hpp"
#include "cc_device.hpp"
#include "cc_intrinsics_dev.hpp"

namespace cc {

// ---------------------------------------------------------------------------------------------
// Per-observation quantities shared by the u-row and the v-row. With w = theta^2, P(w) = 1 + k1 w + .. + k4 w^4,
// Q = d theta_d / d theta = P + 2 w P'(w), g = theta_d / rho = (theta / rho) P, n^2 = rho^2 + zc^2 and the direction
// (cx, cy) = (xc, yc) / rho of the point around the axis:
//   xd = theta_d cx,                    d xd / d k_j = theta cx w^j,
//   d xd / d xc = g + D cx^2,  d xd / d yc = D cx cy,  d xd / d zc = -Q xc / n^2,   D = Q zc / n^2 - g
// (yd alike). Near the axis the two terms of D agree to rho^2 / zc^2, and the textbook form D / rho^2 times xc^2 divides the
// rounding of that difference by rho^2. Here D only ever meets cx^2, cx cy, cy^2 <= 1: its rounding, a few ulps of g, stays
// a few ulps of the g it is added to, for every rho > 0 -- no series and no threshold. theta / rho is a quotient of two
// accurately rounded numbers (atan2 has no cancellation). What is left is rho = 0 itself, 0 / 0 in cx, cy and theta / rho:
// there the direction is taken as 0 (D = 0 in the limit, any direction serves) and theta / rho as its limit 1 / zc.
// ---------------------------------------------------------------------------------------------
struct FishCommon {
  double a0, a1, a2, ex, ey, w, xd, yd, dxx, dxy, dyy, dxz, dyz;
};

__device__ __forceinline__ void fisheye_common(const double* k, const double* R, const double* t,
                                               double X0, double X1, double X2, FishCommon& c) {
  c.a0 = R[0] * X0 + R[1] * X1 + R[2] * X2;
  c.a1 = R[3] * X0 + R[4] * X1 + R[5] * X2;
  c.a2 = R[6] * X0 + R[7] * X1 + R[8] * X2;
  const double xc = c.a0 + t[0], yc = c.a1 + t[1], zc = c.a2 + t[2];
  const double rho2 = xc * xc + yc * yc;
  const double rho = sqrt(rho2);
  const double th = atan2(rho, zc);
  const bool off_axis = rho2 > 0.0;
  const double ir = off_axis ? 1.0 / rho : 0.0;
  const double cx = xc * ir, cy = yc * ir;
  const double e = off_axis ? th * ir : 1.0 / zc;
  c.w = th * th;
  const double k1 = k[4], k2 = k[5], k3 = k[6], k4 = k[7];
  const double P = 1.0 + c.w * (k1 + c.w * (k2 + c.w * (k3 + c.w * k4)));
  const double Q = 1.0 + c.w * (3.0 * k1 + c.w * (5.0 * k2 + c.w * (7.0 * k3 + c.w * (9.0 * k4))));
  const double g = e * P;
  const double qz = Q / (rho2 + zc * zc);
  const double D = qz * zc - g;
  c.ex = th * cx;
  c.ey = th * cy;
  c.xd = c.ex * P;
  c.yd = c.ey * P;
  const double Dx = D * cx;
  c.dxx = g + Dx * cx;
  c.dxy = Dx * cy;
  c.dyy = g + D * cy * cy;
  c.dxz = -qz * xc;
  c.dyz = -qz * yc;
}

// the pose columns and the residual behind a row's first nine entries: b = d r / d (xc, yc, zc)
__device__ __forceinline__ void fisheye_row_tail(const FishCommon& c, double b0, double b1, double b2, double rw, double* v) {
  v[9] = 2.0 * (b2 * c.a1 - b1 * c.a2); v[10] = 2.0 * (b0 * c.a2 - b2 * c.a0); v[11] = 2.0 * (b1 * c.a0 - b0 * c.a1);
  v[12] = b0; v[13] = b1; v[14] = b2; v[15] = rw;
}

// row of the u residual: d (fx xd + px - u) / d [fx fy px py k1 k2 k3 k4 - | rot(3) t(3)], then r; the weight wt (the Huber
// weight, or 0 on a lane beyond the frame's last observation) rides on the row's factors as in row_u
__device__ __forceinline__ void fisheye_row_u(const double* k, const FishCommon& c, double r, double* v, double wt) {
  const double fx = k[0] * wt;
  v[0] = c.xd * wt; v[1] = 0.0; v[2] = wt; v[3] = 0.0;
  const double f1 = fx * c.ex * c.w, f2 = f1 * c.w, f3 = f2 * c.w;
  v[4] = f1; v[5] = f2; v[6] = f3; v[7] = f3 * c.w; v[8] = 0.0;
  fisheye_row_tail(c, fx * c.dxx, fx * c.dxy, fx * c.dxz, r * wt, v);
}

__device__ __forceinline__ void fisheye_row_v(const double* k, const FishCommon& c, double r, double* v, double wt) {
  const double fy = k[1] * wt;
  v[0] = 0.0; v[1] = c.yd * wt; v[2] = 0.0; v[3] = wt;
  const double f1 = fy * c.ey * c.w, f2 = f1 * c.w, f3 = f2 * c.w;
  v[4] = f1; v[5] = f2; v[6] = f3; v[7] = f3 * c.w; v[8] = 0.0;
  fisheye_row_tail(c, fy * c.dxy, fy * c.dyy, fy * c.dyz, r * wt, v);
}

}  // namespace cc
