// cc_intr_start_batch_dev.hpp -- the kernels of the batched fisheye focal-length start (cc_intr_start_batch.hpp), in a header so
// that cc_intr_start_batch.hip is the launch only. Each is its single-problem kernel (cc_intr_start_dev.hpp) with the problem's
// IntrStartDev read from the device table instead of passed by value, on the same helpers (cc_intr_start_math.hpp); the view
// kernel's wave is compiled from the same lines (cc_intr_start_view_body.hpp).
#pragma once

#include "cc_intr_start_batch.hpp"
#include "cc_intr_start_math.hpp"

namespace cc {

// pass 0 / pass 1, grid T.E, 256 threads: workgroup w owns observations [begin, end) of one problem, a pixel a thread and pass of
// the loop; one atomic per word and workgroup on that problem's words. pass 2, grid T.B, one wave: problem blockIdx.x's centre,
// r_max and candidates. The expressions are k_intr_start_extent's, none fused: maxima and minima do not depend on the grid.
__global__ __launch_bounds__(256) void k_intrb_start_extent(IntrStartBatchDev T, int pass) {
#pragma clang fp contract(off)
  __shared__ unsigned long long s_max[4][4];   // the waves' maxima of a workgroup
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = (blockDim.x + 63) >> 6;
  if (pass == 2) {
    if ((int64_t)blockIdx.x >= T.B || threadIdx.x >= 64) return;
    const IntrStartDev P = T.prob[blockIdx.x];
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
  if ((int64_t)blockIdx.x >= T.E) return;
  const IntrStartExtentWg wg = T.extent[blockIdx.x];
  const IntrStartDev P = T.prob[wg.problem];
  const float2* __restrict__ uv2 = reinterpret_cast<const float2*>(P.uv);
  if (pass == 0) {
    unsigned long long lo_u = 0, hi_u = 0, lo_v = 0, hi_v = 0;   // (0: below the word of every finite float)
    for (int64_t i = wg.begin + threadIdx.x; i < wg.end; i += blockDim.x) {
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
    if (threadIdx.x < 4) {
      unsigned long long m = s_max[0][threadIdx.x];
      for (int w = 1; w < nwaves; ++w) m = s_max[w][threadIdx.x] > m ? s_max[w][threadIdx.x] : m;
      if (m) atomicMax(P.box + threadIdx.x, m);
    }
    return;
  }
  double cx, cy;
  intr_start_centre(P, cx, cy);
  unsigned long long r = 0;   // (a non-negative double's bits order as the double does)
  for (int64_t i = wg.begin + threadIdx.x; i < wg.end; i += blockDim.x) {
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

// Grid (workgroups, candidates), one wave each. pose_pass 0, the search: workgroup x is T.search_where[x] = {problem, k}, searched
// view floor(k F / S) of that problem through candidate blockIdx.y, its record goes to the problem's srec / skind [j][k].
// pose_pass 1: workgroup x is T.view_where[x] = {problem, view} through that problem's picked candidate, its record goes to the
// problem's view / kind; nothing is written for a problem without a qualified candidate. From there on the wave runs
// k_intr_start_view's lines on the problem's IntrStartDev.
__global__ __launch_bounds__(64) void k_intrb_start_view(IntrStartBatchDev T, int pose_pass, int refine_iterations) {
  __shared__ __attribute__((aligned(16))) double s_stage[kStageDoublesPerWave];
  const int lane = threadIdx.x;
  if ((int64_t)blockIdx.x >= (pose_pass ? T.Ftot : T.Stot)) return;
  const int2 wh = pose_pass ? T.view_where[blockIdx.x] : T.search_where[blockIdx.x];
  const IntrStartDev P = T.prob[wh.x];
  int64_t v = wh.y;
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
#include "cc_intr_start_view_body.hpp"
}

// Grid T.B, one wave per problem, lane j = candidate j: k_intr_start_pick on the problem's IntrStartDev -- S_j = f_j^2 sum_k
// cost_{j,k} over the problem's searched views k in index order, a serial sum per lane.
__global__ __launch_bounds__(64) void k_intrb_start_pick(IntrStartBatchDev T) {
  if ((int64_t)blockIdx.x >= T.B) return;
  const IntrStartDev P = T.prob[blockIdx.x];
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
