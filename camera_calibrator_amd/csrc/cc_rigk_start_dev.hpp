// cc_rigk_start_dev.hpp -- the kernels of the pixel start (cc_rigk_start.hpp says what they are for) and their device helpers, in
// a header so that cc_rigk_start.hip is the launches only. All arithmetic is fp64 on the float32 pixels.
//
// One wave per view: the view's camera and with it the intrinsics set are the same for every lane, so the set's 8 or 9
// coefficients are scalar loads and live in scalar registers; lanes stride over the view's observations. A lane's result depends
// on its own pixel and on the set's coefficients only -- no cross-lane operation, no dependence on the launch geometry.
// The methods are those of k_undistort / k_undistort_fisheye (cc_points.hip), restated here on double coefficients: those
// kernels keep their text.
#pragma once

#include "cc_rigk_start.hpp"

namespace cc {

// ---- radial-tangential model: slots fx fy px py k1 k2 p1 p2 k3 ---------------------------------------------------------------
// residual and Jacobian of the distortion map at (x, y); *scale: the sum of the magnitudes of the terms the residual is made
// of -- the map's rounding error is a few units in the last place of it
__device__ __forceinline__ void rigk_radtan_eval(double k1, double k2, double p1, double p2, double k3, double x, double y,
                                                 double xd, double yd, double (&r)[2], double (&J)[4], double* scale) {
  const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
  const double m = 1.0 + k1 * r2 + k2 * r4 + k3 * r6;
  const double tx = 2.0 * p1 * x * y, ux = p2 * (r2 + 2.0 * x * x);
  const double ty = 2.0 * p2 * x * y, uy = p1 * (r2 + 2.0 * y * y);
  r[0] = x * m + tx + ux - xd;
  r[1] = y * m + ty + uy - yd;
  const double mp = k1 + 2.0 * k2 * r2 + 3.0 * k3 * r4;
  J[0] = m + 2.0 * mp * x * x + 2.0 * p1 * y + 6.0 * p2 * x;
  J[1] = J[2] = 2.0 * mp * x * y + 2.0 * p1 * x + 2.0 * p2 * y;
  J[3] = m + 2.0 * mp * y * y + 2.0 * p2 * x + 6.0 * p1 * y;
  if (scale) {
    const double ma = 1.0 + fabs(k1) * r2 + fabs(k2) * r4 + fabs(k3) * r6;
    *scale = (fabs(x) + fabs(y)) * ma + fabs(tx) + fabs(ux) + fabs(ty) + fabs(uy) + fabs(xd) + fabs(yd);
  }
}

constexpr int kRigkRadtanSteps = 100;      // accepted and rejected steps together; a start inside the basin takes < 10
constexpr double kRigkRootLevel = 256.0;   // |residual| <= this many units of 2^-53 of the map's terms: a root

// Levenberg-Marquardt with the radius rules of k_undistort from the distorted point itself. A search that ends away from a root
// (a map that turns back before it reaches the pixel, a stationary point of the cost) gives false.
__device__ __forceinline__ bool rigk_radtan_root(const double* __restrict__ k, double xd, double yd, double* ox, double* oy) {
  const double k1 = k[4], k2 = k[5], p1 = k[6], p2 = k[7], k3 = k[8];
  double x = xd, y = yd, radius = 1e4, dec = 2.0;
  double r[2], J[4];
  rigk_radtan_eval(k1, k2, p1, p2, k3, x, y, xd, yd, r, J, nullptr);
  double cost = 0.5 * (r[0] * r[0] + r[1] * r[1]);
  for (int it = 0; it < kRigkRadtanSteps && cost > 0.0; ++it) {
    const double h00 = J[0] * J[0] + J[2] * J[2], h01 = J[0] * J[1] + J[2] * J[3];
    const double h11 = J[1] * J[1] + J[3] * J[3];
    const double g0 = J[0] * r[0] + J[2] * r[1], g1 = J[1] * r[0] + J[3] * r[1];
    const double a00 = h00 + fmax(h00, 1e-6) / radius, a11 = h11 + fmax(h11, 1e-6) / radius;
    const double det = a00 * a11 - h01 * h01;
    const double dx = -(a11 * g0 - h01 * g1) / det, dy = -(a00 * g1 - h01 * g0) / det;
    if (!(fabs(dx) + fabs(dy) > 1e-17 * (fabs(x) + fabs(y) + 1e-300))) break;
    double rn[2], Jn[4];
    rigk_radtan_eval(k1, k2, p1, p2, k3, x + dx, y + dy, xd, yd, rn, Jn, nullptr);
    const double cn = 0.5 * (rn[0] * rn[0] + rn[1] * rn[1]);
    if (cn < cost) {
      x += dx; y += dy; cost = cn;
      r[0] = rn[0]; r[1] = rn[1];
      J[0] = Jn[0]; J[1] = Jn[1]; J[2] = Jn[2]; J[3] = Jn[3];
      radius = fmin(1e16, radius * 3.0);
      dec = 2.0;
    } else {
      radius /= dec; dec *= 2.0;
      if (radius < 1e-32) break;
    }
  }
  double scale;
  rigk_radtan_eval(k1, k2, p1, p2, k3, x, y, xd, yd, r, J, &scale);
  *ox = x; *oy = y;
  return fmax(fabs(r[0]), fabs(r[1])) <= kRigkRootLevel * 1.1102230246251565e-16 * scale;   // (false for a NaN residual)
}

// ---- fisheye model: slots fx fy px py k1 k2 k3 k4 - ---------------------------------------------------------------------------
__device__ __forceinline__ double rigk_fisheye_theta_d(const double* __restrict__ k, double th) {
  const double w = th * th;
  return th * (1.0 + w * (k[4] + w * (k[5] + w * (k[6] + w * k[7]))));
}
__device__ __forceinline__ double rigk_fisheye_slope(const double* __restrict__ k, double th) {
  const double w = th * th;
  return 1.0 + w * (3.0 * k[4] + w * (5.0 * k[5] + w * (7.0 * k[6] + w * (9.0 * k[7]))));
}

// theta in [0, top) with theta_d(theta) = td > 0, by the rule of k_undistort_fisheye: a root bracketed by the interval's ends is
// found by Newton steps that fall back to bisection; otherwise plain Newton from theta = td climbs the first rising branch and
// either converges inside the interval or meets a slope <= 0 / leaves the interval / runs out of steps: no root.
// top is the double below pi/2 for the normalised point x / z = tan(theta) (xd, yd) / td, and with BEYOND_90 the double below pi
// for the bearing start: a point at 90 degrees off the axis and beyond it has a theta like any other; only tan(theta) had none.
template <bool BEYOND_90>
__device__ __forceinline__ bool rigk_fisheye_root(const double* __restrict__ k, double td, double* theta) {
  const double top = BEYOND_90 ? 3.141592653589793 : 1.5707963267948966;
  const bool bracketed = rigk_fisheye_theta_d(k, top) - td > 0.0;
  double lo = 0.0, hi = top;
  double th = td < top ? td : 0.5 * top;
  bool found = false;
  for (int it = 0; it < 200; ++it) {
    const double f = rigk_fisheye_theta_d(k, th) - td;
    const double fp = rigk_fisheye_slope(k, th);
    if (f == 0.0) { found = true; break; }
    double tn = th - f / fp;
    if (bracketed) {
      if (f > 0.0) hi = th; else lo = th;
      if (!(fp > 0.0) || !(tn > lo && tn < hi)) tn = 0.5 * (lo + hi);
    } else if (!(fp > 0.0) || !(tn >= 0.0 && tn <= top)) {
      break;
    }
    const bool small = fabs(tn - th) <= 4.5e-16 * th;
    th = tn;
    if (small) { found = true; break; }
  }
  *theta = th;
  return found || bracketed;
}

__global__ __launch_bounds__(64) void k_rigk_start_unproject(RigkStartDev P) {
  const int64_t g = blockIdx.x;
  if (g >= P.NG) return;
  const int64_t s0 = P.goff[g], s1 = P.goff[g + 1];
  const double* __restrict__ k = P.intr + (size_t)P.kset[P.gcam[g]] * 16;   // (the same for every lane: scalar loads)
  const double fx = k[0], fy = k[1], px = k[2], py = k[3];
  const bool focal_ok = isfinite(fx) && isfinite(fy) && fx != 0.0 && fy != 0.0;
  const float2* __restrict__ uv2 = reinterpret_cast<const float2*>(P.uv);
  float2* __restrict__ out2 = reinterpret_cast<float2*>(P.out);
  const float nanf_ = __builtin_nanf("");
  for (int64_t i = s0 + threadIdx.x; i < s1; i += 64) {
    const float2 p = uv2[i];
    float2 o = make_float2(nanf_, nanf_);
    if (focal_ok && isfinite(p.x) && isfinite(p.y)) {
      const double xd = ((double)p.x - px) / fx, yd = ((double)p.y - py) / fy;
      if (P.model == CC_MODEL_FISHEYE) {
        const double td = sqrt(xd * xd + yd * yd);
        double th;
        if (td == 0.0) o = make_float2((float)xd, (float)yd);   // the axis itself
        else if (td > 0.0 && rigk_fisheye_root<false>(k, td, &th)) {
          const double s = tan(th) / td;
          o = make_float2((float)(xd * s), (float)(yd * s));
        }
      } else {
        double x, y;
        if (rigk_radtan_root(k, xd, yd, &x, &y)) o = make_float2((float)x, (float)y);
      }
    }
    if (isnan(o.x) || isnan(o.y)) o = make_float2(nanf_, nanf_);   // (a non-finite coefficient: both coordinates or none)
    out2[i] = o;
  }
}

// ... with the model of the view's camera (CC_MODEL_MIXED): the model and the intrinsics set the same for every lane. The two
// bodies stand next to each other: a per-view function shared between them, as rigk_bearing_view is, moves both kernels'
// register allocation
__global__ __launch_bounds__(64) void k_rigk_start_unproject_cam(RigkStartCamDev P) {
  const int64_t g = blockIdx.x;
  if (g >= P.NG) return;
  const int64_t s0 = P.goff[g], s1 = P.goff[g + 1];
  const int cam = P.gcam[g];
  const bool fish = P.cmodel[cam] == CC_MODEL_FISHEYE;
  const double* __restrict__ k = P.intr + (size_t)P.kset[cam] * 16;   // (the same for every lane: scalar loads)
  const double fx = k[0], fy = k[1], px = k[2], py = k[3];
  const bool focal_ok = isfinite(fx) && isfinite(fy) && fx != 0.0 && fy != 0.0;
  const float2* __restrict__ uv2 = reinterpret_cast<const float2*>(P.uv);
  float2* __restrict__ out2 = reinterpret_cast<float2*>(P.out);
  const float nanf_ = __builtin_nanf("");
  for (int64_t i = s0 + threadIdx.x; i < s1; i += 64) {
    const float2 p = uv2[i];
    float2 o = make_float2(nanf_, nanf_);
    if (focal_ok && isfinite(p.x) && isfinite(p.y)) {
      const double xd = ((double)p.x - px) / fx, yd = ((double)p.y - py) / fy;
      if (fish) {
        const double td = sqrt(xd * xd + yd * yd);
        double th;
        if (td == 0.0) o = make_float2((float)xd, (float)yd);   // the axis itself
        else if (td > 0.0 && rigk_fisheye_root<false>(k, td, &th)) {
          const double s = tan(th) / td;
          o = make_float2((float)(xd * s), (float)(yd * s));
        }
      } else {
        double x, y;
        if (rigk_radtan_root(k, xd, yd, &x, &y)) o = make_float2((float)x, (float)y);
      }
    }
    if (isnan(o.x) || isnan(o.y)) o = make_float2(nanf_, nanf_);   // (a non-finite coefficient: both coordinates or none)
    out2[i] = o;
  }
}

// ---- the bearing start: unit directions instead of x / z ------------------------------------------------------------------------
// One view's pixels into float3 unit bearings (three floats per observation, packed); NaN x 3: no bearing.
__device__ __forceinline__ void rigk_bearing_view(const RigkBearingDev& P, int64_t g, bool fish, const double* __restrict__ k) {
  const int64_t s0 = P.goff[g], s1 = P.goff[g + 1];
  const double fx = k[0], fy = k[1], px = k[2], py = k[3];
  const bool focal_ok = isfinite(fx) && isfinite(fy) && fx != 0.0 && fy != 0.0;
  const float2* __restrict__ uv2 = reinterpret_cast<const float2*>(P.uv);
  float* __restrict__ out = P.out;
  const float nanf_ = __builtin_nanf("");
  for (int64_t i = s0 + threadIdx.x; i < s1; i += 64) {
    const float2 p = uv2[i];
    float o0 = nanf_, o1 = nanf_, o2 = nanf_;
    if (focal_ok && isfinite(p.x) && isfinite(p.y)) {
      const double xd = ((double)p.x - px) / fx, yd = ((double)p.y - py) / fy;
      if (fish) {
        const double td = sqrt(xd * xd + yd * yd);
        double th;
        if (td == 0.0) { o0 = 0.0f; o1 = 0.0f; o2 = 1.0f; }   // the axis itself
        else if (td > 0.0 && rigk_fisheye_root<true>(k, td, &th)) {
          const double s = sin(th) / td;
          o0 = (float)(xd * s); o1 = (float)(yd * s); o2 = (float)cos(th);
        }
      } else {
        double x, y;
        if (rigk_radtan_root(k, xd, yd, &x, &y)) {
          const double s = 1.0 / sqrt(x * x + y * y + 1.0);
          o0 = (float)(x * s); o1 = (float)(y * s); o2 = (float)s;
        }
      }
    }
    if (isnan(o0) || isnan(o1) || isnan(o2)) { o0 = nanf_; o1 = nanf_; o2 = nanf_; }   // (all three components or none)
    out[i * 3] = o0; out[i * 3 + 1] = o1; out[i * 3 + 2] = o2;
  }
}

// one wave per view, one model for the handle (P.cmodel is not read)
__global__ __launch_bounds__(64) void k_rigk_start_bearing(RigkBearingDev P) {
  const int64_t g = blockIdx.x;
  if (g >= P.NG) return;
  const double* __restrict__ k = P.intr + (size_t)P.kset[P.gcam[g]] * 16;   // (the same for every lane: scalar loads)
  rigk_bearing_view(P, g, P.model == CC_MODEL_FISHEYE, k);
}

// ... with the model of the view's camera (CC_MODEL_MIXED)
__global__ __launch_bounds__(64) void k_rigk_start_bearing_cam(RigkBearingDev P) {
  const int64_t g = blockIdx.x;
  if (g >= P.NG) return;
  const int cam = P.gcam[g];
  const double* __restrict__ k = P.intr + (size_t)P.kset[cam] * 16;
  rigk_bearing_view(P, g, P.cmodel[cam] == CC_MODEL_FISHEYE, k);
}

}  // namespace cc
