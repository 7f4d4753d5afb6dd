// cc_rig_lens_dev.hpp -- the pixel models of the rig solve with intrinsics (cc_rigk_*) as device functions, each defined ONCE:
// what a sweep or a per-observation cost needs of a lens behind the pose chain. Device functions only, no kernel: cc_rig.hip and
// cc_rig_lens.hip both include it, and every kernel that inlines these keeps its text.
#pragma once

#include "cc_common.hpp"

namespace cc {

// ceres::HuberLoss + Corrector: the arithmetic of huber_outlier / huber in cc_rig.hip, line for line, with b = a^2 and a2 = 2 a
// from the caller (kernel arguments: the same bits as the products formed there, in scalar registers from the start)
__device__ __forceinline__ void lens_huber(double a, double b, double a2, double s, double& rho, double& sr) {
  if (s > b) {
    const double y = rsqrt_pos(s);
    const double r = s * y;
    const double q = fmax(2.2250738585072014e-308, a * y);
    sr = q * rsqrt_pos(q);
    rho = a2 * r - b;
  } else {
    rho = s;
    sr = 1.0;
  }
}

// ---- radial-tangential rows on the normalised point (x, y, 1 / z), slots fx fy px py k1 k2 p1 p2 k3 ---------------------------
// The pixel residuals, B = d residual / d x_cam (what the rows chain through both poses) and the two rows of d residual / d k
// (DistortNormalized / DistortPixels, calibrator.cpp:70-95).
struct LensRadtanRows {
  double ru, rv, Bu0, Bu1, Bu2, Bv0, Bv1, Bv2;
  double ju[9], jv[9];
};
__device__ __forceinline__ void lens_radtan_rows(const double* k, double x, double y, double iz, double u, double v, LensRadtanRows& r) {
  const double fx = k[0], fy = k[1];
  const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
  const double m = 1.0 + k[4] * r2 + k[5] * r4 + k[8] * r6;
  const double xd = x * m + 2.0 * k[6] * x * y + k[7] * (r2 + 2.0 * x * x);
  const double yd = y * m + 2.0 * k[7] * x * y + k[6] * (r2 + 2.0 * y * y);
  r.ru = fx * xd + k[2] - u;
  r.rv = fy * yd + k[3] - v;
  r.ju[0] = xd; r.ju[1] = 0.0; r.ju[2] = 1.0; r.ju[3] = 0.0;
  r.ju[4] = fx * x * r2; r.ju[5] = fx * x * r4; r.ju[6] = fx * 2.0 * x * y; r.ju[7] = fx * (r2 + 2.0 * x * x); r.ju[8] = fx * x * r6;
  r.jv[0] = 0.0; r.jv[1] = yd; r.jv[2] = 0.0; r.jv[3] = 1.0;
  r.jv[4] = fy * y * r2; r.jv[5] = fy * y * r4; r.jv[6] = fy * (r2 + 2.0 * y * y); r.jv[7] = fy * 2.0 * x * y; r.jv[8] = fy * y * r6;
  const double mp = k[4] + 2.0 * k[5] * r2 + 3.0 * k[8] * r4;
  const double dxx = m + 2.0 * mp * x * x + 2.0 * k[6] * y + 6.0 * k[7] * x;
  const double dxy = 2.0 * mp * x * y + 2.0 * k[6] * x + 2.0 * k[7] * y;
  const double dyy = m + 2.0 * mp * y * y + 2.0 * k[7] * x + 6.0 * k[6] * y;
  r.Bu0 = fx * dxx * iz; r.Bu1 = fx * dxy * iz; r.Bu2 = -(fx * dxx * x + fx * dxy * y) * iz;
  r.Bv0 = fy * dxy * iz; r.Bv1 = fy * dyy * iz; r.Bv2 = -(fy * dxy * x + fy * dyy * y) * iz;
}

// ---- fisheye point on the camera-frame point itself, slots fx fy px py k1 k2 k3 k4 - ------------------------------------------
// fisheye_common (cc_fisheye_dev.hpp) from the camera-frame point on, restated so that the intrinsics kernels' translation
// units stay as they are. With w = theta^2, P = 1 + k1 w + .. + k4 w^4, Q = P + 2 w P', g = (theta / rho) P,
// n^2 = rho^2 + zc^2, (cx, cy) = (xc, yc) / rho and D = Q zc / n^2 - g:
//   xd = theta cx P,  d xd / d (xc, yc, zc) = (g + D cx^2, D cx cy, -Q xc / n^2),  d xd / d k_j = theta cx w^j   (yd alike).
// D only ever meets cx^2, cx cy, cy^2 <= 1, so its rounding stays a few ulps of g for every rho > 0. On the axis itself
// (rho = 0) the direction is taken as 0 and theta / rho as its limit 1 / zc.
struct LensFishPoint {
  double ex, ey, w, xd, yd, dxx, dxy, dyy, dxz, dyz;
};
__device__ __forceinline__ void lens_fish_point(const double* k, double xc, double yc, double zc, LensFishPoint& c) {
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

}  // namespace cc
