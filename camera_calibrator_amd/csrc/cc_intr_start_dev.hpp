// cc_intr_start_dev.hpp -- the kernels of the fisheye focal-length start (cc_intr_start.hpp), in a header so that cc_intr_start.hip
// is the launch only. k_intr_start_view is k_rig_start_view_bearing (cc_rig_start_bearing_dev.hpp) with the bearing of
// observation i formed in fp64 from its pixel, the centre and the candidate focal length instead of read from a float3 buffer,
// written a second time on the helpers both share (cc_rig_start_math.hpp, cc_device.hpp, cc_eigen_dev.hpp): with the body as a
// function that both kernels instantiate, k_rig_start_view_bearing does not keep its text. One step differs: the
// null vector's inverse iteration goes on past its twelve steps until it has settled (smallest_eigvec_settled below says why).
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

// pass 0: the bounding box of the finite pixels; pass 1: r_max, their largest distance from the centre (any grid: max and min do
// not depend on the order); pass 2, one wave: the centre, r_max and the candidates f_j = r_max / theta_j as doubles.
// A pixel is finite when both its coordinates are. No product is fused into a sum here: the values are the ones IEEE arithmetic
// gives on any machine.
__global__ __launch_bounds__(256) void k_intr_start_extent(IntrStartDev P, int pass) {
#pragma clang fp contract(off)
  __shared__ unsigned long long s_max[4][4];   // the waves' maxima of a workgroup
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = (blockDim.x + 63) >> 6;
  if (pass == 2) {
    if (blockIdx.x || threadIdx.x >= 64) return;
    double cx, cy;
    intr_start_centre(P, cx, cy);
    const double r_max = __longlong_as_double((long long)P.box[4]);
    if (lane == 0) { P.ext[0] = cx; P.ext[1] = cy; P.ext[2] = r_max; P.ext[3] = 0.0; }
    if (lane < P.C) {
      const double th = P.C == 1 ? P.theta_lo : P.theta_lo + ((double)lane * (P.theta_hi - P.theta_lo)) / (double)(P.C - 1);
      P.f[lane] = r_max / th;
    }
    return;
  }
  const float2* __restrict__ uv2 = reinterpret_cast<const float2*>(P.uv);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (pass == 0) {
    unsigned long long lo_u = 0, hi_u = 0, lo_v = 0, hi_v = 0;   // (0: below the word of every finite float)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P.N; i += stride) {
      const float2 p = uv2[i];
      if (!(isfinite(p.x) && isfinite(p.y))) continue;
      const unsigned long long wu = start_order_word(p.x), wv = start_order_word(p.y);
      const unsigned long long nu = ~wu & 0xffffffffull, nv = ~wv & 0xffffffffull;
      lo_u = nu > lo_u ? nu : lo_u; hi_u = wu > hi_u ? wu : hi_u;
      lo_v = nv > lo_v ? nv : lo_v; hi_v = wv > hi_v ? wv : hi_v;
    }
    lo_u = wave_max_u64(lo_u); hi_u = wave_max_u64(hi_u); lo_v = wave_max_u64(lo_v); hi_v = wave_max_u64(hi_v);
    if (lane == 0) { s_max[wave][0] = lo_u; s_max[wave][1] = hi_u; s_max[wave][2] = lo_v; s_max[wave][3] = hi_v; }
    __syncthreads();
    if (threadIdx.x < 4) {   // one atomic per word and workgroup: they all land on the same four addresses
      unsigned long long m = s_max[0][threadIdx.x];
      for (int w = 1; w < nwaves; ++w) m = s_max[w][threadIdx.x] > m ? s_max[w][threadIdx.x] : m;
      if (m) atomicMax(P.box + threadIdx.x, m);
    }
    return;
  }
  double cx, cy;
  intr_start_centre(P, cx, cy);
  unsigned long long r = 0;   // (a non-negative double's bits order as the double does)
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P.N; i += stride) {
    const float2 p = uv2[i];
    if (!(isfinite(p.x) && isfinite(p.y))) continue;
    const double d0 = (double)p.x - cx, d1 = (double)p.y - cy;
    const double q0 = d0 * d0, q1 = d1 * d1;
    const double ri = sqrt(q0 + q1);
    const unsigned long long w = ri == ri ? (unsigned long long)__double_as_longlong(ri) : 0ull;
    r = w > r ? w : r;
  }
  r = wave_max_u64(r);
  if (lane == 0) s_max[wave][0] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < nwaves; ++w) r = s_max[w][0] > r ? s_max[w][0] : r;
    if (r) atomicMax(P.box + 4, r);
  }
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

// Grid (views, candidates), one wave each. pose_pass 0, the search: block (k, j) is searched view floor(k F / S) through candidate
// j, its record goes to P.srec / P.skind [j][k]. pose_pass 1: block (v, 0) is view v through the picked candidate, its record goes
// to P.view / P.kind [v]; nothing is written when no candidate qualified. A searched view comes out of the two passes with the
// same bits: the same instructions on the same inputs.
// Stages V and R of k_rig_start_view_bearing, unchanged in arithmetic: classification, centring / scaling, board basis, the Gram
// of the tangent rows on the staged matrix contraction, its null vector (iterated until it settles), the sign from sum b . (H y~), the rotation fix and
// Levenberg-Marquardt on the chord. The record is that kernel's, with the chord cost at the returned pose in slot 17 and the kind in slot 18.
__global__ __launch_bounds__(64) void k_intr_start_view(IntrStartDev P, int pose_pass, int refine_iterations) {
  __shared__ __attribute__((aligned(16))) double s_stage[kStageDoublesPerWave];
  const int lane = threadIdx.x;
  int64_t v = blockIdx.x;
  int j = blockIdx.y;
  double* out;
  int32_t* kind_out;
  if (pose_pass) {
    j = P.best[0];
    if (j < 0 || v >= P.F) return;
    out = P.view + v * kRigViewStride;
    kind_out = P.kind + v;
  } else {
    if (v >= P.S || j >= P.C) return;
    out = P.srec + ((int64_t)j * P.S + v) * kRigViewStride;
    kind_out = P.skind + (int64_t)j * P.S + v;
    v = (v * P.F) / P.S;
  }
  const IntrStartLens lens{P.uv, P.ext[0], P.ext[1], P.f[j]};
  const int64_t s0 = P.off[v], s1 = P.off[v + 1];
  const int64_t n = s1 - s0;
  const float* xyz = P.xyz;
  int kind = RIG_VIEW_INVALID;

  // centroid; a non-finite coordinate anywhere makes every sum non-finite
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, bad = 0.0;
  for (int64_t i = s0 + lane; i < s1; i += 64) {
    a0 += xyz[i * 3]; a1 += xyz[i * 3 + 1]; a2 += xyz[i * 3 + 2];
    bad += (double)lens.uv[i * 2] * 0.0 + (double)lens.uv[i * 2 + 1] * 0.0;
  }
  const double inv_n = 1.0 / (double)(n > 0 ? n : 1);
  const double c[3] = {wsum0(a0) * inv_n, wsum0(a1) * inv_n, wsum0(a2) * inv_n};
  bad = wsum0(bad) + (c[0] + c[1] + c[2]) * 0.0 + (lens.cx + lens.cy + lens.f) * 0.0;
  // scatter about the centroid
  double sc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = s0 + lane; i < s1; i += 64) {
    const double d0 = xyz[i * 3] - c[0], d1 = xyz[i * 3 + 1] - c[1], d2 = xyz[i * 3 + 2] - c[2];
    sc[0] += d0 * d0; sc[1] += d0 * d1; sc[2] += d0 * d2; sc[3] += d1 * d1; sc[4] += d1 * d2; sc[5] += d2 * d2;
  }
#pragma unroll
  for (int e = 0; e < 6; ++e) sc[e] = wsum0(sc[e]);
  const double s2 = (sc[0] + sc[3] + sc[5]) * inv_n;   // mean squared radius
  const bool finite_in = bad == 0.0 && isfinite(s2) && s2 > 0.0 && n >= 4 && lens.f > 0.0;
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
    auto order = [&](int i, int j2) {   // ascending, stable
      const bool sw = l[j2] < l[i];
      const double li = sw ? l[j2] : l[i], lj = sw ? l[i] : l[j2];
      l[i] = li; l[j2] = lj;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double ei = sw ? e[j2][r] : e[i][r], ej = sw ? e[i][r] : e[j2][r];
        e[i][r] = ei; e[j2][r] = ej;
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
        intr_start_bearing_of(lens, ic, b);
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
          for (int k = 0; k < 9; ++k) G[i][k] = s_stage[i * 16 + k];
        smallest_eigvec_settled<9>(G, h);
        // the sign that puts the points along their bearings: sum b . (H y~) > 0 (t_z > 0 is wrong for a board the camera's
        // plane cuts); r0, r1 and t are odd in h
        double along = 0.0;
        for (int64_t i = s0 + lane; i < s1; i += 64) {
          const double d0 = xyz[i * 3] - c[0], d1 = xyz[i * 3 + 1] - c[1], d2 = xyz[i * 3 + 2] - c[2];
          const double y0 = (B[0][0] * d0 + B[1][0] * d1 + B[2][0] * d2) * is, y1 = (B[0][1] * d0 + B[1][1] * d1 + B[2][1] * d2) * is;
          double b[3];
          intr_start_bearing_of(lens, i, b);
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
          for (int k = 0; k < 12; ++k) G[i][k] = s_stage[i * 16 + k];
        smallest_eigvec_settled<12>(G, p);
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

  double rms2 = 0.0, chord = 0.0;
  if (kind != RIG_VIEW_INVALID) {
    // stage R: Levenberg-Marquardt on the six pose coordinates; no depth test, the chord has no singularity short of p = 0
    double H[21], gr[6], cost;
    start_view_sums_bearing(lens, xyz, s0, s1, lane, R, t, H, gr, cost);
    double lambda = 1e-4;
    for (int it = 0; it < refine_iterations; ++it) {
      double d[6], Rn[9], tn[3], Hn[21], gn[6], cn = 0.0;
      bool accept = start_solve6(H, gr, lambda, d);
      if (accept) {
        start_rotate(d, R, Rn);
        tn[0] = t[0] + d[3]; tn[1] = t[1] + d[4]; tn[2] = t[2] + d[5];
        start_view_sums_bearing(lens, xyz, s0, s1, lane, Rn, tn, Hn, gn, cn);
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
    chord = cost;
    rms2 = cost / (2.0 * (double)n);   // a squared angle for small errors
    if (!isfinite(rms2) || !isfinite(t[0] + t[1] + t[2])) kind = RIG_VIEW_INVALID;
  }
  if (lane == 0) {
    *kind_out = kind;
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
      out[kIntrStartCostSlot] = chord;
      out[kIntrStartKindSlot] = (double)kind;
    }
  }
}

// ---- pick -----------------------------------------------------------------------------------------------------------------------
// One wave, lane j = candidate j: S_j = f_j^2 sum_k cost_{j,k} over the searched views k in index order (a serial sum per lane:
// the same bits on every call). A candidate with a searched view whose record is invalid is disqualified, unless that view is
// invalid for every candidate; the smallest S_j among the qualified wins, the lowest index on ties.
__global__ __launch_bounds__(64) void k_intr_start_pick(IntrStartDev P) {
  const int j = threadIdx.x;
  const bool live = j < P.C;
  double sum = 0.0;
  bool ok = live;
  for (int64_t k = 0; k < P.S; ++k) {
    bool inv = true;
    double cost = 0.0;
    if (live) {
      const int64_t at = (int64_t)j * P.S + k;
      cost = P.srec[at * kRigViewStride + kIntrStartCostSlot];
      inv = P.skind[at] == RIG_VIEW_INVALID || !isfinite(cost);
    }
    const bool all_inv = __ballot(!inv) == 0ull;
    if (inv) ok = ok && all_inv; else sum += cost;
  }
  const double f = live ? P.f[j] : 0.0;
  const double score = f * f * sum;
  ok = ok && isfinite(score);
  if (live) { P.score[j] = score; P.qualified[j] = ok ? 1 : 0; }
  const unsigned long long okm = __ballot(ok);
  int best = -1;
  double best_score = 0.0, best_f = 0.0;
  for (int c = 0; c < P.C; ++c) {   // (wave-uniform: every lane walks the candidates in index order)
    const double sc = __shfl(score, c, 64), fc = __shfl(f, c, 64);
    if (((okm >> c) & 1ull) && (best < 0 || sc < best_score)) { best = c; best_score = sc; best_f = fc; }
  }
  if (j == 0) { P.best[0] = best; P.best[1] = __popcll(okm); P.ext[3] = best_f; }
}

}  // namespace cc
