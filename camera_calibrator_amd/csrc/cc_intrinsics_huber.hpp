// cc_intrinsics_huber.hpp -- EXTENSION (the reference's Calibrator::Optimize sets no loss function, calibrator.cpp:236-324):
// ceres::HuberLoss(a) with its Corrector for the single-camera intrinsics solve, a in pixels (gfx950).
//
//   per observation  s = ru^2 + rv^2 (pixels^2),  rho(s) = s for s <= a^2, else 2 a sqrt(s) - a^2,  cost = 1/2 sum rho(s);
//   the observation's two rows of [J r] are multiplied by sqrt(rho'(s)): 1 up to a^2, sqrt(a / sqrt(s)) beyond
//   (rho'' <= 0: the Corrector has no second-order term).
//
// Gradient, Gauss-Newton block, Jacobi scale and model cost change all come from the scaled rows, so nothing behind the sweep
// changes -- except that the cost is no longer half of entry (15, 15) of the Gram block: the sweep adds 1/2 rho per lane and
// writes the sum to the statistics row's ST_COST, the one channel the step kernels and the host take the cost from.
//
// Included by cc_intrinsics.hip: k_intr_sweep_huber is k_intr_sweep (same prologue, tiles, staging, MFMA contraction and
// outputs) with the row weight and the cost above; k_intr_obs_cost writes the per-observation costs. The kernels are copies
// under names of their own so that k_intr_sweep keeps its code object (register table, bits); the batch form of the sweep is in
// cc_intrinsics_batch_huber.hip, the loss function itself (intr_huber) next to the rows it scales in cc_intrinsics_dev.hpp.
// Out of scope: the persistent per-solve kernel, every multi-GPU form (exchange, RCCL, optimize_multi), losses other than
// Huber, class-level access to the per-observation costs.
#pragma once
#include "cc_common.hpp"
#include "cc_device.hpp"
#include "cc_intrinsics_dev.hpp"

namespace cc {

// ---------------------------------------------------------------------------------------------
// The per-observation model of cc_intrinsics_dev.hpp (obs_common, row_u, row_v) with every fused multiply-add SPELLED OUT,
// the way k_intr_sweep's main loop is compiled: which of two products the compiler fuses into a sum is its own choice per
// kernel (in k_intr_sweep a0 fuses its second product and a1, a2 their first; row_u's b2 fuses b1 y and row_v's b0 x), and a
// copy of the loop under another name gets other choices and blocks that differ in the last bits. With the choices written
// down a weight of exactly 1 reproduces k_intr_sweep's rows bit for bit -- a threshold no observation exceeds leaves the
// blocks what they are with the loss off (tests/test_gpu_intr_huber.py holds the two kernels together). Nothing here is left
// to contract: every sum of a product is an fma. (The functions -- huber_obs_common, huber_row_u, huber_row_v, huber_residuals -- live in
// cc_intrinsics_dev.hpp: the persistent kernel's two sweeps, full and residual-only, are written with them too.)
// ---------------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------------
// robust sweep: k_intr_sweep with the Huber weight on the rows and 1/2 sum rho as the cost (huber_a > 0).
// sm layout and flags as in k_intr_sweep; sm[176..179] the waves' cost sums.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSweepThreads, 4) void k_intr_sweep_huber(IntrDev P, int flags, double huber_a) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* s_stage = reinterpret_cast<double*>(smem_raw);       // [4][1024]
  double* s_blk = s_stage;                                      // [1024] cross-wave reduce (after the loop)
  double* sm = s_stage + 4 * kStageDoublesPerWave;              // [256] prologue scratch
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = P.T;
  const int64_t f = (int64_t)blockIdx.x / T;
  const int tile = (int)(blockIdx.x - f * T);
  const bool in_solve = (flags & 1) != 0, restart = (flags & 2) != 0;
  const LmCtl* ctl = P.ctl;
  const int c_done = ctl->done, c_phase = ctl->phase, c_valid = ctl->step_valid, c_cur = ctl->cur;
  const int done = restart ? 0 : c_done, phase = restart ? 0 : c_phase, step_valid = restart ? 0 : c_valid,
            cur = restart ? 0 : c_cur;
  int64_t s0 = P.off[f], s1 = P.off[f + 1];
  if (T > 1) {   // this workgroup's tile of the frame
    const int64_t len = (s1 - s0 + T - 1) / T;
    s0 = s0 + tile * len < s1 ? s0 + tile * len : s1;
    s1 = s0 + len < s1 ? s0 + len : s1;
  }
  const float2* uv2 = reinterpret_cast<const float2*>(P.uv);
  const int64_t wrem = s1 - s0 - wave * 64;
  const int npass = wrem > 0 ? (int)((wrem + kSweepThreads - 1) / kSweepThreads) : 0;   // passes of THIS wave
  // unconditional loads from a clamped index (idle slots re-read a valid observation; the arena holds one slot even when N = 0)
  const int64_t safe0 = s0 < P.N ? s0 : 0;
  float2 nm;
  float nX0, nX1, nX2;
  {
    const int64_t idx = s0 + tid;
    const int64_t ic = idx < s1 ? idx : safe0;
    nm = uv2[ic];
    nX0 = P.xyz[ic * 3]; nX1 = P.xyz[ic * 3 + 1]; nX2 = P.xyz[ic * 3 + 2];
  }
  double gv;
  {
    const double* src;
    if (tid < 60) src = P.Y + f * kYStride + tid;
    else if (tid < 67) src = (restart ? P.init_pose : P.pose) + (size_t)f * 8 + (tid - 60);
    else if (tid < 74) src = P.pose + ((size_t)P.F + f) * 8 + (tid - 67);
    else if (tid < 83) src = (restart ? P.init_intr : P.intr) + (tid - 74);
    else if (tid < 92) src = P.intr + 16 + (tid - 83);
    else if (tid < 101) src = P.ds + (tid - 92);
    else if (tid < 110) src = P.ss + (tid - 101);
    else if (tid < 116) src = P.sp + f * 8 + (tid - 110);
    else src = P.ss;   // (threads without a slot: any readable word)
    gv = *src;
  }
  // previous Gram block of the frame (model-cost term): sum of its tiles, from the buffer of the accepted point
  double g_old = 0.0;
  if (tile == 0) {
    const size_t base = cur ? (size_t)P.F : 0;
    if (T == 1) g_old = P.blocks[(base + f) * 256 + tid];
    else for (int k = 0; k < T; ++k) g_old += P.blocks[((base + f) * T + k) * 256 + tid];
  }
  if (tid < 116) sm[tid] = gv;
  if (done) return;
  if (phase != 0 && !step_valid) return;
  if (P.x.on && in_solve && blockIdx.x == 0 && tid == 0) P.x.seq[1] += 1ull;   // (never with the loss on: kept so that the launch contract is k_intr_sweep's)
  if (restart) {   // restore buffer 0 and clear the arrival counter of the elimination
    if (tile == 0 && tid >= 60 && tid < 67) P.pose[(size_t)f * 8 + (tid - 60)] = sm[tid];
    if (blockIdx.x == 0 && tid >= 74 && tid < 83) P.intr[tid - 74] = sm[tid];
    if (blockIdx.x == 0 && tid == 0) *P.arrive = 0u;
  }
  const int dst = phase == 0 ? cur : (cur ^ 1);
  __syncthreads();
  const int pose_o = cur ? 67 : 60, intr_o = cur ? 83 : 74;
  if (tid < 6) {
    const double* Yr = sm + tid * 10;
    double a = Yr[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) a += Yr[j] * sm[92 + j];
    sm[129 + tid] = phase != 0 ? -a * sm[110 + tid] : 0.0;
  } else if (tid >= 8 && tid < 17) {
    const int j = tid - 8;
    const double d = (phase == 0 || (P.mask & (1u << j))) ? 0.0 : sm[92 + j] * sm[101 + j];
    sm[120 + j] = d;
    const double kc = sm[intr_o + j] + d;
    sm[148 + j] = kc;
    if (blockIdx.x == 0 && phase != 0) P.intr[dst * 16 + j] = kc;
  }
  __syncthreads();
  if (tid == 0) {
    double q[4], t[3], dp[6];
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = sm[pose_o + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = sm[pose_o + 4 + i];
#pragma unroll
    for (int i = 0; i < 6; ++i) dp[i] = sm[129 + i];
    double step2 = 0.0;
    if (phase != 0) {
      double qn[4];
      quat_plus(q, dp, qn);
#pragma unroll
      for (int i = 0; i < 4; ++i) { const double d = qn[i] - q[i]; step2 += d * d; q[i] = qn[i]; }
#pragma unroll
      for (int i = 0; i < 3; ++i) { const double tn = t[i] + dp[3 + i]; const double d = tn - t[i]; step2 += d * d; t[i] = tn; }
      if (tile == 0) {
        double* pose_dst = P.pose + ((size_t)dst * P.F + f) * 8;
#pragma unroll
        for (int i = 0; i < 4; ++i) pose_dst[i] = q[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) pose_dst[4 + i] = t[i];
      }
    }
    double R[9];
    quat_to_R(q, R);
#pragma unroll
    for (int i = 0; i < 9; ++i) sm[136 + i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) sm[145 + i] = t[i];
    sm[158] = step2;
    sm[159] = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] + t[0] * t[0] + t[1] * t[1] + t[2] * t[2];
  }
  __syncthreads();

  // model-cost term of this frame over the (scaled) block at the accepted point, reduced here and not behind the main loop
  double qterm = 0.0;
  if (phase != 0 && tile == 0) {
    const int a = tid >> 4, b = tid & 15;
    if (a < 15) qterm = b < 15 ? 0.5 * sm[120 + a] * g_old * sm[120 + b] : sm[120 + a] * g_old;
  }
  {
    const double qw = wave_sum(qterm);
    if (lane == 0) sm[170 + wave] = qw;
  }

  double R[9], tt[3], kk[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = rfl(sm[136 + i]);
#pragma unroll
  for (int i = 0; i < 3; ++i) tt[i] = rfl(sm[145 + i]);
#pragma unroll
  for (int i = 0; i < 9; ++i) kk[i] = rfl(sm[148 + i]);
  const uint32_t mask = P.mask;

  // ---- main loop: 64 observations per wave per pass, no workgroup barrier. obs_common gives both residual components before
  // the first row: the lane forms s, the weight of its two rows and its share of the cost
  double* stage = s_stage + wave * kStageDoublesPerWave;
  d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
  double hcost = 0.0;   // 1/2 sum rho over this lane's observations, in pass order
  for (int p = 0; p < npass; ++p) {
    const int64_t idx = s0 + (int64_t)p * kSweepThreads + tid;
    const bool valid = idx < s1;  // only the last pass of a frame has idle lanes
    const float2 m = nm;
    const float X0 = nX0, X1 = nX1, X2 = nX2;
    {   // next pass, unconditionally
      const int64_t nidx = idx + kSweepThreads;
      const int64_t ic = nidx < s1 ? nidx : safe0;
      nm = uv2[ic];
      nX0 = P.xyz[ic * 3]; nX1 = P.xyz[ic * 3 + 1]; nX2 = P.xyz[ic * 3 + 2];
    }
    ObsCommon oc;
    huber_obs_common(kk, R, tt, (double)X0, (double)X1, (double)X2, oc);
    double ru, rv;
    huber_residuals(kk, oc, (double)m.x, (double)m.y, ru, rv);
    double rho, sr;
    intr_huber(huber_a, ru * ru + rv * rv, rho, sr);
    const double wrow = valid ? sr : 0.0;   // (an idle lane's rows are zero and it adds nothing to the cost)
    hcost += valid ? 0.5 * rho : 0.0;
    double v[16];
    huber_row_u(kk, oc, ru, v, wrow);
    stage_row(stage, lane, v);
    wave_lds_fence();
    gram_rows(stage, lane, acc0, acc1);
    wave_lds_fence();
    huber_row_v(kk, oc, rv, v, wrow);
    stage_row(stage, lane, v);
    wave_lds_fence();
    gram_rows(stage, lane, acc0, acc1);
    wave_lds_fence();
  }
  {
    const double hw = wave_sum(hcost);
    if (lane == 0) sm[176 + wave] = hw;
  }

  // ---- cross-wave reduction of the 16x16 block (C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg)
  __syncthreads();  // s_blk aliases the staging buffers
#pragma unroll
  for (int r = 0; r < 4; ++r) s_blk[wave * 256 + ((lane >> 4) + 4 * r) * 16 + (lane & 15)] = acc0[r] + acc1[r];
  __syncthreads();
  const double g = gram_entry_held(mask, tid) ? 0.0 : (s_blk[tid] + s_blk[256 + tid]) + (s_blk[512 + tid] + s_blk[768 + tid]);
  P.blocks[(((size_t)dst * P.F + f) * T + tile) * 256 + tid] = g;
  if (tid == 255) {   // the thread that writes the row in k_intr_sweep; the cost is the waves' sum of 1/2 rho, not g / 2
    double* st = P.stats + (size_t)blockIdx.x * kStatsCols;
    st[ST_COST] = (sm[176] + sm[177]) + (sm[178] + sm[179]);
    st[ST_QMODEL] = (sm[170] + sm[171]) + (sm[172] + sm[173]);
    st[ST_STEP2] = tile == 0 ? sm[158] : 0.0;
    st[ST_XNORM2] = tile == 0 ? sm[159] : 0.0;
  }
  if (phase == 0 && tid < 9 * 17 && tid % 17 == 0) P.hd0[(size_t)blockIdx.x * 16 + tid / 17] = g;
}

// ---------------------------------------------------------------------------------------------
// per-observation cost at the point in buffer `cur`, in the caller's order: 1/2 rho(s), or 1/2 s with the loss off
// (huber_a <= 0). One lane per observation; the lane finds its frame in the offsets by bisection and rebuilds the frame's
// rotation itself (a read-back kernel, not part of an iteration). Exact square root: what the oracle computes.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_intr_obs_cost(IntrDev P, int cur, double huber_a, double* out /*[N]*/) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P.N) return;
  int64_t lo = 0, hi = P.F;   // the frame with off[lo] <= i < off[lo + 1] (empty frames share an offset: the last of them wins)
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (P.off[mid] <= i) lo = mid; else hi = mid;
  }
  const double* pose = P.pose + ((size_t)cur * P.F + lo) * 8;
  const double* k = P.intr + cur * 16;
  double kk[9], R[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) kk[j] = k[j];
  const double q[4] = {pose[0], pose[1], pose[2], pose[3]}, t[3] = {pose[4], pose[5], pose[6]};
  quat_to_R(q, R);
  ObsCommon oc;
  obs_common(kk, R, t, (double)P.xyz[i * 3], (double)P.xyz[i * 3 + 1], (double)P.xyz[i * 3 + 2], oc);
  const double ru = kk[0] * oc.xd + kk[2] - (double)P.uv[i * 2], rv = kk[1] * oc.yd + kk[3] - (double)P.uv[i * 2 + 1];
  const double s = ru * ru + rv * rv, b = huber_a * huber_a;
  out[i] = 0.5 * ((huber_a > 0.0 && s > b) ? 2.0 * huber_a * sqrt(s) - b : s);
}

}  // namespace cc
