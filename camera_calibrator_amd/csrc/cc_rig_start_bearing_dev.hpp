// cc_rig_start_bearing_dev.hpp -- stages V and R of the rig start on unit bearings (cc_rig_start.hpp: rig_start_enqueue_views_bearing),
// in a header so that cc_rig_start_bearing.hip is the launch only. A translation unit of its own: a second kernel with a staging
// buffer in cc_rig_start.hip changes the text the compiler gives k_rig_start_view, and that kernel keeps its text.
#pragma once

#include "cc_rig_start_math.hpp"

namespace cc {

// ---- stages V and R on unit bearings (cc_rigk_estimate_start_bearing) -------------------------------------------------------------
// The float32 bearing of observation i, normalised again in fp64 (the rounding to float32 leaves |b| = 1 +- 6e-8): with an exact
// unit vector I - b b^T is a projector and the two tangent rows below give it without a weight of their own.
__device__ __forceinline__ void start_bearing_of(const float* bearing, int64_t i, double (&b)[3]) {
  const double b0 = bearing[i * 3], b1 = bearing[i * 3 + 1], b2 = bearing[i * 3 + 2];
  const double inv = 1.0 / sqrt(b0 * b0 + b1 * b1 + b2 * b2);
  b[0] = b0 * inv; b[1] = b1 * inv; b[2] = b2 * inv;
}

// Gauss-Newton sums of one view at the pose (R, t) on the chord: residual p / |p| - b (three components), p = R X + t, the
// updates of start_view_sums. J = (I - ph ph^T) / |p| [ -[R X]x | I ]. Nothing is singular short of p = 0. Wave-uniform on return.
__device__ __forceinline__ void start_view_sums_bearing(const float* bearing, const float* xyz, int64_t s0, int64_t s1, int lane,
                                                        const double* R, const double* t, double (&H)[21], double (&g)[6], double& cost) {
#pragma unroll
  for (int e = 0; e < 21; ++e) H[e] = 0.0;
#pragma unroll
  for (int e = 0; e < 6; ++e) g[e] = 0.0;
  cost = 0.0;
  for (int64_t i = s0 + lane; i < s1; i += 64) {
    const double X0 = xyz[i * 3], X1 = xyz[i * 3 + 1], X2 = xyz[i * 3 + 2];
    double b[3];
    start_bearing_of(bearing, i, b);
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

// k_rig_start_view restated for bearings: the same classification, centring / scaling, board basis, null vector, rotation fix and
// output record. The closed form comes from b x (P y~) = 0: its Gram is sum (I - b b^T) (x) y~ y~^T over the 9 (planar) or 12
// (general) unknowns of P, row-major, staged as the two rows e_k (x) y~ of an orthonormal tangent pair e_1, e_2 of b.
// P.uv is not read.
// (cc_intr_start_dev.hpp holds a second copy of this body and of start_view_sums_bearing, with the bearing formed from the pixel --
// k_intr_start_view; one shared definition changes this kernel's text, DESIGN 4.19. A fix here belongs there too.)
__global__ __launch_bounds__(64) void k_rig_start_view_bearing(RigStartDev P, const float* __restrict__ bearing, int refine_iterations) {
  __shared__ __attribute__((aligned(16))) double s_stage[kStageDoublesPerWave];
  const int lane = threadIdx.x;
  const int64_t g = blockIdx.x;
  if (g >= P.NG) return;
  const int64_t s0 = P.goff[g], s1 = P.goff[g + 1];
  const int64_t n = s1 - s0;
  const float* xyz = P.oxyz;
  double* out = P.view + g * kRigViewStride;
  int kind = RIG_VIEW_INVALID;

  // centroid; a non-finite coordinate anywhere makes every sum non-finite
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, bad = 0.0;
  for (int64_t i = s0 + lane; i < s1; i += 64) {
    a0 += xyz[i * 3]; a1 += xyz[i * 3 + 1]; a2 += xyz[i * 3 + 2];
    bad += (double)bearing[i * 3] * 0.0 + (double)bearing[i * 3 + 1] * 0.0 + (double)bearing[i * 3 + 2] * 0.0;
  }
  const double inv_n = 1.0 / (double)(n > 0 ? n : 1);
  const double c[3] = {wsum0(a0) * inv_n, wsum0(a1) * inv_n, wsum0(a2) * inv_n};
  bad = wsum0(bad) + (c[0] + c[1] + c[2]) * 0.0;
  // scatter about the centroid
  double sc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = s0 + lane; i < s1; i += 64) {
    const double d0 = xyz[i * 3] - c[0], d1 = xyz[i * 3 + 1] - c[1], d2 = xyz[i * 3 + 2] - c[2];
    sc[0] += d0 * d0; sc[1] += d0 * d1; sc[2] += d0 * d2; sc[3] += d1 * d1; sc[4] += d1 * d2; sc[5] += d2 * d2;
  }
#pragma unroll
  for (int e = 0; e < 6; ++e) sc[e] = wsum0(sc[e]);
  const double s2 = (sc[0] + sc[3] + sc[5]) * inv_n;   // mean squared radius
  const bool finite_in = bad == 0.0 && isfinite(s2) && s2 > 0.0 && n >= 4;
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
  if (finite_in) {
    const double s = sqrt(s2), is = 1.0 / s, w = inv_n / s2;
    double A[3][3] = {{sc[0] * w, sc[1] * w, sc[2] * w}, {sc[1] * w, sc[3] * w, sc[4] * w}, {sc[2] * w, sc[4] * w, sc[5] * w}}, V[3][3];
    jacobi_eigen<3>(A, V, 10);
    double l[3] = {A[0][0], A[1][1], A[2][2]}, e[3][3];   // e[k] = eigenvector k
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int r = 0; r < 3; ++r) e[k][r] = V[r][k];
    auto order = [&](int i, int j) {   // ascending, stable
      const bool sw = l[j] < l[i];
      const double li = sw ? l[j] : l[i], lj = sw ? l[i] : l[j];
      l[i] = li; l[j] = lj;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double ei = sw ? e[j][r] : e[i][r], ej = sw ? e[i][r] : e[j][r];
        e[i][r] = ei; e[j][r] = ej;
      }
    };
    order(0, 1); order(1, 2); order(0, 1);
    const double l0 = fmax(l[0], 0.0), l1 = fmax(l[1], 0.0), l2 = l[2];
    if (l2 > 0.0 && sqrt(l1 / l2) >= kPlanarTol) kind = sqrt(l0 / l1) < kPlanarTol ? RIG_VIEW_PLANAR : RIG_VIEW_GENERAL;
    if (kind == RIG_VIEW_GENERAL && n < 6) kind = RIG_VIEW_INVALID;

    if (kind != RIG_VIEW_INVALID) {
      // basis of the normalised points y = B^T (X - c) / s: the board's own axes (planar) or the world's (general)
      double B[3][3];   // columns
      if (kind == RIG_VIEW_PLANAR) {
        const double n0 = e[2][1] * e[1][2] - e[2][2] * e[1][1], n1 = e[2][2] * e[1][0] - e[2][0] * e[1][2], n2 = e[2][0] * e[1][1] - e[2][1] * e[1][0];
#pragma unroll
        for (int r = 0; r < 3; ++r) { B[r][0] = e[2][r]; B[r][1] = e[1][r]; }
        B[0][2] = n0; B[1][2] = n1; B[2][2] = n2;
      } else {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int k = 0; k < 3; ++k) B[r][k] = r == k ? 1.0 : 0.0;
      }
      // Gram of the tangent rows, 64 observations a pass on the staged matrix contraction
      d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
      const int npass = (int)((n + 63) / 64);
      for (int p = 0; p < npass; ++p) {
        const int64_t idx = s0 + (int64_t)p * 64 + lane;
        const bool valid = idx < s1;
        const int64_t ic = valid ? idx : s0;
        const double d0 = xyz[ic * 3] - c[0], d1 = xyz[ic * 3 + 1] - c[1], d2 = xyz[ic * 3 + 2] - c[2];
        const double y0 = (B[0][0] * d0 + B[1][0] * d1 + B[2][0] * d2) * is, y1 = (B[0][1] * d0 + B[1][1] * d1 + B[2][1] * d2) * is;
        const double y2 = (B[0][2] * d0 + B[1][2] * d1 + B[2][2] * d2) * is;
        double b[3];
        start_bearing_of(bearing, ic, b);
        // an orthonormal pair next to b without a branch on its direction (Duff et al. 2017): sg + b2 is never inside (-1, 1)
        const double sg = b[2] < 0.0 ? -1.0 : 1.0, ka = -1.0 / (sg + b[2]), kb = b[0] * b[1] * ka;
        const double e1[3] = {1.0 + sg * b[0] * b[0] * ka, sg * kb, -sg * b[0]}, e2[3] = {kb, sg + b[1] * b[1] * ka, -b[1]};
        double row[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) row[k] = 0.0;
        if (valid) {
          if (kind == RIG_VIEW_PLANAR) {
#pragma unroll
            for (int r = 0; r < 3; ++r) { row[r * 3] = e1[r] * y0; row[r * 3 + 1] = e1[r] * y1; row[r * 3 + 2] = e1[r]; }
          } else {
#pragma unroll
            for (int r = 0; r < 3; ++r) { row[r * 4] = e1[r] * y0; row[r * 4 + 1] = e1[r] * y1; row[r * 4 + 2] = e1[r] * y2; row[r * 4 + 3] = e1[r]; }
          }
        }
        stage_row(s_stage, lane, row);
        wave_lds_fence();
        gram_rows(s_stage, lane, acc0, acc1);
        wave_lds_fence();
#pragma unroll
        for (int k = 0; k < 16; ++k) row[k] = 0.0;
        if (valid) {
          if (kind == RIG_VIEW_PLANAR) {
#pragma unroll
            for (int r = 0; r < 3; ++r) { row[r * 3] = e2[r] * y0; row[r * 3 + 1] = e2[r] * y1; row[r * 3 + 2] = e2[r]; }
          } else {
#pragma unroll
            for (int r = 0; r < 3; ++r) { row[r * 4] = e2[r] * y0; row[r * 4 + 1] = e2[r] * y1; row[r * 4 + 2] = e2[r] * y2; row[r * 4 + 3] = e2[r]; }
          }
        }
        stage_row(s_stage, lane, row);
        wave_lds_fence();
        gram_rows(s_stage, lane, acc0, acc1);
        wave_lds_fence();
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) s_stage[((lane >> 4) + 4 * r) * 16 + (lane & 15)] = acc0[r] + acc1[r];
      wave_lds_fence();
      double Rp[3][3], tp[3];
      if (kind == RIG_VIEW_PLANAR) {
        double G[9][9], h[9];
#pragma unroll
        for (int i = 0; i < 9; ++i)
#pragma unroll
          for (int j = 0; j < 9; ++j) G[i][j] = s_stage[i * 16 + j];
        smallest_eigvec<9>(G, h, 0.0);
        // the sign that puts the points along their bearings: sum b . (H y~) > 0 (t_z > 0 is wrong for a board the camera's
        // plane cuts); r0, r1 and t are odd in h
        double along = 0.0;
        for (int64_t i = s0 + lane; i < s1; i += 64) {
          const double d0 = xyz[i * 3] - c[0], d1 = xyz[i * 3 + 1] - c[1], d2 = xyz[i * 3 + 2] - c[2];
          const double y0 = (B[0][0] * d0 + B[1][0] * d1 + B[2][0] * d2) * is, y1 = (B[0][1] * d0 + B[1][1] * d1 + B[2][1] * d2) * is;
          double b[3];
          start_bearing_of(bearing, i, b);
          along += b[0] * (h[0] * y0 + h[1] * y1 + h[2]) + b[1] * (h[3] * y0 + h[4] * y1 + h[5]) + b[2] * (h[6] * y0 + h[7] * y1 + h[8]);
        }
        along = wsum0(along);
        double lh = 1.0 / sqrt(h[0] * h[0] + h[3] * h[3] + h[6] * h[6]);
        if (along < 0.0) lh = -lh;
        const double r0[3] = {lh * h[0], lh * h[3], lh * h[6]}, r1[3] = {lh * h[1], lh * h[4], lh * h[7]};
        tp[0] = lh * h[2]; tp[1] = lh * h[5]; tp[2] = lh * h[8];
        const double r2[3] = {r0[1] * r1[2] - r0[2] * r1[1], r0[2] * r1[0] - r0[0] * r1[2], r0[0] * r1[1] - r0[1] * r1[0]};
#pragma unroll
        for (int r = 0; r < 3; ++r) { Rp[r][0] = r0[r]; Rp[r][1] = r1[r]; Rp[r][2] = r2[r]; }
      } else {
        double G[12][12], p[12];
#pragma unroll
        for (int i = 0; i < 12; ++i)
#pragma unroll
          for (int j = 0; j < 12; ++j) G[i][j] = s_stage[i * 16 + j];
        smallest_eigvec<12>(G, p, 0.0);
        // det P_3x3 > 0 after the division: the determinant fixes the sign, there is no mirror solution
        const double det = p[0] * (p[5] * p[10] - p[6] * p[9]) - p[1] * (p[4] * p[10] - p[6] * p[8]) + p[2] * (p[4] * p[9] - p[5] * p[8]);
        const double ia = 1.0 / cbrt(det);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int k = 0; k < 3; ++k) Rp[r][k] = p[r * 4 + k] * ia;
          tp[r] = p[r * 4 + 3] * ia;
        }
      }
      start_fix_rotation(Rp);
      // R = R_p B^T, t = s t_p - R c
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) R[r * 3 + k] = Rp[r][0] * B[k][0] + Rp[r][1] * B[k][1] + Rp[r][2] * B[k][2];
        t[r] = s * tp[r] - (R[r * 3] * c[0] + R[r * 3 + 1] * c[1] + R[r * 3 + 2] * c[2]);
      }
    }
  }

  double rms2 = 0.0;
  if (kind != RIG_VIEW_INVALID) {
    // stage R: Levenberg-Marquardt on the six pose coordinates; no depth test, the chord has no singularity short of p = 0
    double H[21], gr[6], cost;
    start_view_sums_bearing(bearing, xyz, s0, s1, lane, R, t, H, gr, cost);
    double lambda = 1e-4;
    for (int it = 0; it < refine_iterations; ++it) {
      double d[6], Rn[9], tn[3], Hn[21], gn[6], cn = 0.0;
      bool accept = start_solve6(H, gr, lambda, d);
      if (accept) {
        start_rotate(d, R, Rn);
        tn[0] = t[0] + d[3]; tn[1] = t[1] + d[4]; tn[2] = t[2] + d[5];
        start_view_sums_bearing(bearing, xyz, s0, s1, lane, Rn, tn, Hn, gn, cn);
        accept = cn < cost && isfinite(cn);
      }
      if (accept) {
#pragma unroll
        for (int e = 0; e < 21; ++e) H[e] = Hn[e];
#pragma unroll
        for (int e = 0; e < 6; ++e) gr[e] = gn[e];
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = Rn[e];
        t[0] = tn[0]; t[1] = tn[1]; t[2] = tn[2];
        cost = cn;
        lambda *= 0.1;
      } else {
        lambda *= 10.0;
      }
    }
    rms2 = cost / (2.0 * (double)n);   // a squared angle for small errors: the unit of the x / z form's rms^2 near the axis
    if (!isfinite(rms2) || !isfinite(t[0] + t[1] + t[2])) kind = RIG_VIEW_INVALID;
  }
  if (lane == 0) {
    P.kind[g] = kind;
    if (kind == RIG_VIEW_INVALID) {
#pragma unroll
      for (int i = 0; i < kRigViewStride; ++i) out[i] = 0.0;
    } else {
      double q[4];
      start_quat_of(R, q);
#pragma unroll
      for (int i = 0; i < 4; ++i) out[i] = q[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) out[4 + i] = t[i];
      out[7] = rms2;
#pragma unroll
      for (int i = 0; i < 9; ++i) out[8 + i] = R[i];
#pragma unroll
      for (int i = 17; i < kRigViewStride; ++i) out[i] = 0.0;
    }
  }
}

}  // namespace cc
