// cc_rig_start_dev.hpp -- the kernels of the rig start (cc_rig_start.hpp says what each one is for), in a header so that
// cc_rig_start.hip is launches only; their device helpers are in cc_rig_start_math.hpp. All arithmetic is fp64 on the float32 inputs.
//
// Every value a wave decides on (centroid, scale, classification, Gram, LM sums) is made wave-uniform by reading lane 0's copy
// of the cross-lane sum: the DPP sums of cc_device.hpp associate differently from lane to lane, and a wave whose lanes
// disagreed in the last bit about `cost_new < cost` would leave the loop in pieces. Each lane then runs the same small dense
// arithmetic on the same numbers (a wave per view: the 12 x 12 inverse iteration alone holds 78 doubles of L).
#pragma once

#include "cc_rig_start_math.hpp"

namespace cc {

// ---- stages V and R: one wave per view ---------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_rig_start_view(RigStartDev P, int refine_iterations) {
  __shared__ __attribute__((aligned(16))) double s_stage[kStageDoublesPerWave];
  const int lane = threadIdx.x;
  const int64_t g = blockIdx.x;
  if (g >= P.NG) return;
  const int64_t s0 = P.goff[g], s1 = P.goff[g + 1];
  const int64_t n = s1 - s0;
  const float2* uv2 = reinterpret_cast<const float2*>(P.uv);
  const float* xyz = P.oxyz;
  double* out = P.view + g * kRigViewStride;
  int kind = RIG_VIEW_INVALID;

  // centroid; a non-finite coordinate anywhere makes every sum non-finite
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, bad = 0.0;
  for (int64_t i = s0 + lane; i < s1; i += 64) {
    const float2 m = uv2[i];
    a0 += xyz[i * 3]; a1 += xyz[i * 3 + 1]; a2 += xyz[i * 3 + 2];
    bad += (double)m.x * 0.0 + (double)m.y * 0.0;
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
      // Gram of the DLT rows, 64 observations a pass on the staged matrix contraction
      d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
      const int npass = (int)((n + 63) / 64);
      for (int p = 0; p < npass; ++p) {
        const int64_t idx = s0 + (int64_t)p * 64 + lane;
        const bool valid = idx < s1;
        const int64_t ic = valid ? idx : s0;
        const double d0 = xyz[ic * 3] - c[0], d1 = xyz[ic * 3 + 1] - c[1], d2 = xyz[ic * 3 + 2] - c[2];
        const double y0 = (B[0][0] * d0 + B[1][0] * d1 + B[2][0] * d2) * is, y1 = (B[0][1] * d0 + B[1][1] * d1 + B[2][1] * d2) * is;
        const double y2 = (B[0][2] * d0 + B[1][2] * d1 + B[2][2] * d2) * is;
        const float2 m = uv2[ic];
        const double u = m.x, v = m.y;
        double row[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) row[k] = 0.0;
        if (valid) {
          if (kind == RIG_VIEW_PLANAR) { row[0] = y0; row[1] = y1; row[2] = 1.0; row[6] = -u * y0; row[7] = -u * y1; row[8] = -u; }
          else { row[0] = y0; row[1] = y1; row[2] = y2; row[3] = 1.0; row[8] = -u * y0; row[9] = -u * y1; row[10] = -u * y2; row[11] = -u; }
        }
        stage_row(s_stage, lane, row);
        wave_lds_fence();
        gram_rows(s_stage, lane, acc0, acc1);
        wave_lds_fence();
#pragma unroll
        for (int k = 0; k < 16; ++k) row[k] = 0.0;
        if (valid) {
          if (kind == RIG_VIEW_PLANAR) { row[3] = y0; row[4] = y1; row[5] = 1.0; row[6] = -v * y0; row[7] = -v * y1; row[8] = -v; }
          else { row[4] = y0; row[5] = y1; row[6] = y2; row[7] = 1.0; row[8] = -v * y0; row[9] = -v * y1; row[10] = -v * y2; row[11] = -v; }
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
        double lh = 1.0 / sqrt(h[0] * h[0] + h[3] * h[3] + h[6] * h[6]);
        if (h[8] < 0.0) lh = -lh;   // t_z > 0: r0, r1 and t are odd in h, so the other sign is their negation
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
    // stage R: Levenberg-Marquardt on the six pose coordinates
    double H[21], gr[6], cost, minz;
    start_view_sums(uv2, xyz, s0, s1, lane, R, t, H, gr, cost, minz);
    double lambda = 1e-4;
    for (int it = 0; it < refine_iterations; ++it) {
      double d[6], Rn[9], tn[3], Hn[21], gn[6], cn = 0.0, zn = 0.0;
      bool accept = start_solve6(H, gr, lambda, d);
      if (accept) {
        start_rotate(d, R, Rn);
        tn[0] = t[0] + d[3]; tn[1] = t[1] + d[4]; tn[2] = t[2] + d[5];
        start_view_sums(uv2, xyz, s0, s1, lane, Rn, tn, Hn, gn, cn, zn);
        accept = cn < cost && isfinite(cn) && zn > 0.0;
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
    rms2 = cost / (2.0 * (double)n);
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

// ---- weighted means of poses -------------------------------------------------------------------------------------------
// The mean rotation is the unit eigenvector of the largest eigenvalue of sum w q q^T (the same for q and -q); the mean
// translation the weighted mean. Each lane adds its items in index order, the lanes are added by the fixed cross-lane tree,
// lane 0's total is used: the result depends on the items only.
struct StartMean {
  double M[10], t[3], w;
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int e = 0; e < 10; ++e) M[e] = 0.0;
    t[0] = t[1] = t[2] = 0.0;
    w = 0.0;
  }
  __device__ __forceinline__ void add(double wi, const double* R, const double* ti) {
    double q[4];
    start_quat_of(R, q);
    int e = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = a; b < 4; ++b) { M[e] += wi * q[a] * q[b]; ++e; }
    t[0] += wi * ti[0]; t[1] += wi * ti[1]; t[2] += wi * ti[2];
    w += wi;
  }
  // wave total -> pose; false: nothing was added
  __device__ __forceinline__ bool finish(double* q, double* tm) {
#pragma unroll
    for (int e = 0; e < 10; ++e) M[e] = wsum0(M[e]);
#pragma unroll
    for (int e = 0; e < 3; ++e) t[e] = wsum0(t[e]);
    w = wsum0(w);
    if (!(w > 0.0) || !isfinite(w)) return false;
    double A[4][4], V[4][4];
    {
      const double iw = 1.0 / w;
      int e = 0;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = a; b < 4; ++b) { A[a][b] = M[e] * iw; A[b][a] = A[a][b]; ++e; }
      tm[0] = t[0] * iw; tm[1] = t[1] * iw; tm[2] = t[2] * iw;
    }
    jacobi_eigen<4>(A, V, 12);
    double best = A[0][0];
    q[0] = V[0][0]; q[1] = V[1][0]; q[2] = V[2][0]; q[3] = V[3][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      const bool b = A[k][k] > best;
      best = b ? A[k][k] : best;
#pragma unroll
      for (int r = 0; r < 4; ++r) q[r] = b ? V[r][k] : q[r];
    }
    const double nrm = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double sg = q[0] < 0.0 ? -nrm : nrm;
#pragma unroll
    for (int r = 0; r < 4; ++r) q[r] *= sg;
    return true;
  }
};

// ---- stage C: one wave per (child, parent) edge ----------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_rig_start_edge(RigStartDev P, int n_edges) {
  const int lane = threadIdx.x, k = blockIdx.x;
  if (k >= n_edges) return;
  const int jc = P.cobs[P.edges[k * 2]], jp = P.cobs[P.edges[k * 2 + 1]];
  StartMean m;
  m.clear();
  if (jc >= 0 && jp >= 0) {
    for (int64_t f = lane; f < P.F; f += 64) {
      const int gc = P.fslot[f * P.CO + jc], gp = P.fslot[f * P.CO + jp];
      if (gc < 0 || gp < 0 || P.kind[gc] == RIG_VIEW_INVALID || P.kind[gp] == RIG_VIEW_INVALID) continue;
      const double* vc = P.view + (int64_t)gc * kRigViewStride;
      const double* vp = P.view + (int64_t)gp * kRigViewStride;
      double R[9], t[3];   // R_rel = R_c R_p^T, t_rel = t_c - R_rel t_p
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i * 3 + j] = vc[8 + i * 3] * vp[8 + j * 3] + vc[8 + i * 3 + 1] * vp[8 + j * 3 + 1] + vc[8 + i * 3 + 2] * vp[8 + j * 3 + 2];
#pragma unroll
      for (int i = 0; i < 3; ++i) t[i] = vc[4 + i] - (R[i * 3] * vp[4] + R[i * 3 + 1] * vp[5] + R[i * 3 + 2] * vp[6]);
      m.add(1.0 / (vc[7] + vp[7] + 1e-30), R, t);
    }
  }
  double q[4] = {1.0, 0.0, 0.0, 0.0}, t[3] = {0.0, 0.0, 0.0};
  m.finish(q, t);   // (an edge of the tree has a co-visible frame; without one the relative pose stays the identity)
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) P.rel[k * 8 + i] = q[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) P.rel[k * 8 + 4 + i] = t[i];
  }
}

// ---- cam_T_rig[child] = rel o cam_T_rig[parent], parents first ---------------------------------------------------------------
__global__ __launch_bounds__(64) void k_rig_start_compose(RigStartDev P, int n_edges) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int k = 0; k < n_edges; ++k) {
    const int c = P.edges[k * 2], p = P.edges[k * 2 + 1];
    const double* a = P.rel + k * 8;
    const double* b = P.cam + (int64_t)p * 8;
    const double bn = 1.0 / sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + b[3] * b[3]);
    const double b0 = b[0] * bn, b1 = b[1] * bn, b2 = b[2] * bn, b3 = b[3] * bn;
    double Ra[9];
    quat_to_R(a, Ra);
    double* o = P.cam + (int64_t)c * 8;
    o[0] = a[0] * b0 - a[1] * b1 - a[2] * b2 - a[3] * b3;
    o[1] = a[0] * b1 + a[1] * b0 + a[2] * b3 - a[3] * b2;
    o[2] = a[0] * b2 - a[1] * b3 + a[2] * b0 + a[3] * b1;
    o[3] = a[0] * b3 + a[1] * b2 - a[2] * b1 + a[3] * b0;
    const double t0 = b[4], t1 = b[5], t2 = b[6];
    o[4] = Ra[0] * t0 + Ra[1] * t1 + Ra[2] * t2 + a[4];
    o[5] = Ra[3] * t0 + Ra[4] * t1 + Ra[5] * t2 + a[5];
    o[6] = Ra[6] * t0 + Ra[7] * t1 + Ra[8] * t2 + a[6];
    o[7] = 0.0;
  }
}

// ---- stage F: one wave per frame ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rig_start_frame(RigStartDev P) {
  const int lane = threadIdx.x & 63;
  const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= P.F) return;   // (whole waves: no barrier below)
  StartMean m;
  m.clear();
  for (int j = lane; j < P.CO; j += 64) {
    const int g = P.fslot[f * P.CO + j], cam = P.obs_cam[j];
    if (g < 0 || P.kind[g] == RIG_VIEW_INVALID || !P.placed[cam]) continue;
    const double* v = P.view + (int64_t)g * kRigViewStride;
    const double* cq = P.cam + (int64_t)cam * 8;
    double Rc[9], R[9], t[3];   // R = R_cr^T R_view, t = R_cr^T (t_view - t_cr)
    quat_to_R(cq, Rc);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) R[i * 3 + k] = Rc[i] * v[8 + k] + Rc[3 + i] * v[8 + 3 + k] + Rc[6 + i] * v[8 + 6 + k];
    const double d0 = v[4] - cq[4], d1 = v[5] - cq[5], d2 = v[6] - cq[6];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = Rc[i] * d0 + Rc[3 + i] * d1 + Rc[6 + i] * d2;
    m.add(1.0 / (v[7] + 1e-30), R, t);
  }
  double q[4], t[3];
  const bool ok = m.finish(q, t);
  if (lane != 0) return;
  P.fplaced[f] = ok ? 1 : 0;
  if (ok) {
#pragma unroll
    for (int i = 0; i < 4; ++i) P.pose[f * 8 + i] = q[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) P.pose[f * 8 + 4 + i] = t[i];
  }
}

}  // namespace cc
