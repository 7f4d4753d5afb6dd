// cc_intrinsics_batch.hip -- EXTENSION: many independent single-camera intrinsics problems solved together (gfx950).
//
// The reference calibrates a rig's cameras one after another (system_calibration.py keeps a list of CamCalibration objects,
// each running optimize_intrinsics: cam_calibration.py:290-314); a small problem leaves almost the whole chip idle. Here B
// problems share ONE pair of launches per LM iteration:
//
//   k_intrb_sweep : one workgroup (4 waves) per (problem, frame); the grid is the total number of frames and a device table
//            maps a workgroup to its problem and local frame. Same prologue, main loop and outputs as k_intr_sweep
//            (cc_intrinsics.hip) with one tile per frame: pose back-substitution + Plus, one observation per lane, rows
//            staged through LDS and contracted with v_mfma_f64_16x16x4_f64, the frame's 16 x 16 Gram block and statistics row.
//   k_intrb_step  : one workgroup per problem. Statistics summed in frame order, trust-region decision, every frame's damped
//            6 x 6 pose block eliminated (sixteen lanes per frame, register Cholesky), Schur sums added in a fixed order,
//            9 x 9 system solved by one wave (chol_solve_rows), gradient / radius tests, step, control block, log record.
//
// Stream order is the only synchronisation: no workgroup waits for another, no counters, no polling, no atomics. A problem
// whose control block says `done` is left alone while the rest iterate: its workgroups return behind their first loads. Every
// sum of a problem is taken over ITS frames in an order fixed by their local indices, so a problem's bits do not depend on
// the batch it sits in, nor on where.
#include "cc_common.hpp"
#include "cc_device.hpp"
#include "cc_intrinsics_dev.hpp"
#include "cc_intrinsics_batch_dev.hpp"
#include "cc_intr_start_batch.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

namespace cc {

constexpr int kBatchLogCap = 1024;   // log records per problem on the device (max_iterations is clamped to this - 1)
// (IntrBatchDev, the device view of a batch: cc_intrinsics_batch_dev.hpp)

// ---------------------------------------------------------------------------------------------
// batch sweep: k_intr_sweep for the frame of one problem of the batch (one tile per frame, current Gram buffer only)
// sm[0..59] Y, [60..66] pose buf 0, [67..73] pose buf 1, [74..82] intr buf 0, [83..91] intr buf 1,
// [92..100] ds (scaled), [101..109] ss, [110..115] sp
// sm[120..134] unscaled step (9 shared, 6 pose); sm[136..144] R; [145..147] t; [148..156] intr_cand
// sm[158] step^2 (pose part), sm[159] |x_cand|^2 (pose part); sm[170..173] model-cost term per wave
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSweepThreads, 4) void k_intrb_sweep(IntrBatchDev P) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* s_stage = reinterpret_cast<double*>(smem_raw);       // [4][1024]
  double* s_blk = s_stage;                                      // [1024] cross-wave reduce (after the loop)
  double* sm = s_stage + 4 * kStageDoublesPerWave;              // [256] prologue scratch
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t f = blockIdx.x;
  const int2 wh = P.where[f];
  const int64_t s0 = P.off[f], s1 = P.off[f + 1];
  const int p = wh.x;
  const bool first_frame = wh.y == 0;   // (the problem's candidate intrinsics are published by its first frame)
  // first pass of observations: needs only the frame's offsets, consumed after the prologue. UNCONDITIONAL loads from a
  // clamped index (idle slots re-read a valid observation; the arena holds one slot even when N = 0): inside an `if` the
  // loaded registers are merged with the defaults at the end of the region, and that merge waits for the load.
  const float2* uv2 = reinterpret_cast<const float2*>(P.uv);
  const int64_t wrem = s1 - s0 - wave * 64;
  const int npass = wrem > 0 ? (int)((wrem + kSweepThreads - 1) / kSweepThreads) : 0;   // passes of THIS wave
  const int64_t safe0 = s0 < P.N ? s0 : 0;
  float2 nm;
  float nX0, nX1, nX2;
  {
    const int64_t idx = s0 + tid;
    const int64_t ic = idx < s1 ? idx : safe0;
    nm = uv2[ic];
    nX0 = P.xyz[ic * 3]; nX1 = P.xyz[ic * 3 + 1]; nX2 = P.xyz[ic * 3 + 2];
  }
  const LmCtl* ctl = P.ctl + p;
  const int done = ctl->done, phase = ctl->phase, step_valid = ctl->step_valid, cur = ctl->cur;
  if (done) return;                              // a finished problem stays untouched while the others iterate
  if (phase != 0 && !step_valid) return;         // no candidate to evaluate: the step kernel shrinks the radius
  const uint32_t mask = P.mask[p];
  const int Ftot = P.Ftot;
  double gv;
  {
    const double* src;
    if (tid < 60) src = P.Y + f * kYStride + tid;
    else if (tid < 67) src = P.pose + (size_t)f * 8 + (tid - 60);
    else if (tid < 74) src = P.pose + ((size_t)Ftot + f) * 8 + (tid - 67);
    else if (tid < 83) src = P.intr + (size_t)p * 32 + (tid - 74);
    else if (tid < 92) src = P.intr + (size_t)p * 32 + 16 + (tid - 83);
    else if (tid < 101) src = P.ds + (size_t)p * 16 + (tid - 92);
    else if (tid < 110) src = P.ss + (size_t)p * 16 + (tid - 101);
    else if (tid < 116) src = P.sp + f * 8 + (tid - 110);
    else src = P.ss;   // (threads without a slot: any readable word)
    gv = *src;
  }
  // previous Gram block of the frame (model-cost term), from the buffer of the accepted point
  const double g_old = P.blocks[((cur ? (size_t)Ftot : 0) + f) * 256 + tid];
  if (tid < 116) sm[tid] = gv;
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
    const double d = (phase == 0 || (mask & (1u << j))) ? 0.0 : sm[92 + j] * sm[101 + j];
    sm[120 + j] = d;
    const double kc = sm[intr_o + j] + d;
    sm[148 + j] = kc;
    if (first_frame && phase != 0) P.intr[(size_t)p * 32 + dst * 16 + j] = kc;
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
      double* pose_dst = P.pose + ((size_t)dst * Ftot + f) * 8;
#pragma unroll
      for (int i = 0; i < 4; ++i) pose_dst[i] = q[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) pose_dst[4 + i] = t[i];
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

  // model-cost term of this frame: q_f = d^T g_f + 1/2 d^T H_f d over the frame's 15 x 15 block at the accepted point,
  // reduced here and not behind the main loop (kept alive across the loop it does not fit four waves per SIMD)
  double qterm = 0.0;
  if (phase != 0) {
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

  // ---- main loop: 64 observations per wave per pass, no workgroup barrier; a frame longer than one pass of the
  // workgroup (256 observations) loops, the next pass's observations are fetched while the current one is processed
  double* stage = s_stage + wave * kStageDoublesPerWave;
  d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
  for (int ps = 0; ps < npass; ++ps) {
    const int64_t idx = s0 + (int64_t)ps * kSweepThreads + tid;
    const bool valid = idx < s1;  // only the last pass of a frame has idle lanes
    const float2 m = nm;
    const float X0 = nX0, X1 = nX1, X2 = nX2;
    {   // next pass, unconditionally (the last pass fetches a slot nobody uses: cheaper than the wait a branch costs)
      const int64_t nidx = idx + kSweepThreads;
      const int64_t ic = nidx < s1 ? nidx : safe0;
      nm = uv2[ic];
      nX0 = P.xyz[ic * 3]; nX1 = P.xyz[ic * 3 + 1]; nX2 = P.xyz[ic * 3 + 2];
    }
    ObsCommon oc;
    obs_common(kk, R, tt, (double)X0, (double)X1, (double)X2, oc);
    double v[16];
    const double wrow = valid ? 1.0 : 0.0;   // (an idle lane's rows are zero: the weight rides on the rows' factors)
    row_u(kk, oc, (double)m.x, v, wrow);
    stage_row(stage, lane, v);
    wave_lds_fence();
    gram_rows_ahead(stage, lane, acc0, acc1);
    wave_lds_fence();
    row_v(kk, oc, (double)m.y, v, wrow);
    stage_row(stage, lane, v);
    wave_lds_fence();
    gram_rows_ahead(stage, lane, acc0, acc1);
    wave_lds_fence();
  }

  // ---- cross-wave reduction of the 16 x 16 block (C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg)
  __syncthreads();  // s_blk aliases the staging buffers
#pragma unroll
  for (int r = 0; r < 4; ++r) s_blk[wave * 256 + ((lane >> 4) + 4 * r) * 16 + (lane & 15)] = acc0[r] + acc1[r];
  __syncthreads();
  // coordinates held constant: their rows and columns are zeroed here, where the block is assembled
  const double g = gram_entry_held(mask, tid) ? 0.0 : (s_blk[tid] + s_blk[256 + tid]) + (s_blk[512 + tid] + s_blk[768 + tid]);
  P.blocks[((size_t)dst * Ftot + f) * 256 + tid] = g;
  if (tid == 255) {   // the thread that holds entry (15, 15) = sum r^2
    double* st = P.stats + (size_t)f * kStatsCols;
    st[ST_COST] = 0.5 * g;
    st[ST_QMODEL] = (sm[170] + sm[171]) + (sm[172] + sm[173]);
    st[ST_STEP2] = sm[158];
    st[ST_XNORM2] = sm[159];
  }
  if (phase == 0 && tid < 9 * 17 && tid % 17 == 0) P.hd0[(size_t)f * 16 + tid / 17] = g;
}

// ---------------------------------------------------------------------------------------------
// batch step: one workgroup per problem -- decision, elimination of every frame's pose block, reduced solve.
// Column layout of the Schur sums as in k_intr_decide_elim: [0..44] upper triangle of the reduced 9 x 9 system (row-major
// pairs j <= k), [45..53] reduced rhs, [54..62] diag of the scaled H_ss, [63] Cholesky failures, [64..72] unscaled shared
// gradient, [73] max over the frames of Ceres' gradient norm of the pose block.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int upper_index(int j, int k) { return j * 9 - (j * (j - 1)) / 2 + (k - j); }   // j <= k

__global__ __launch_bounds__(256) void k_intrb_step(IntrBatchDev P) {
  __shared__ double Zs[16][64];
  __shared__ double red[16][kPartialCols];
  __shared__ double s_part[64 * 4];     // statistics: one partial row per chunk of frames
  __shared__ double s_hpart[16 * 16];   // hd0 (initial round): one partial row per chunk of frames
  __shared__ double s_tot[16];
  __shared__ double s_ss[16];
  __shared__ double sv[kPartialCols];
  __shared__ LmCtl s_ctl;
  __shared__ cc_iteration s_log;
  __shared__ int s_logged;
  __shared__ unsigned char pj[48], pk[48];
  __shared__ unsigned long long s_in[64];
  const int tid = threadIdx.x, g = tid >> 4, l = tid & 15;
  const int p = blockIdx.x;
  const int f0 = P.first[p], F = P.first[p + 1] - f0;
  // one round trip: [control block (18) | options (12) | intrinsics, both buffers (9 + 9)] and the statistics rows
  unsigned long long word;
  {
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(P.ctl + p);
    if (tid < 18) src = reinterpret_cast<const unsigned long long*>(P.ctl + p) + tid;
    else if (tid < 30) src = reinterpret_cast<const unsigned long long*>(P.opts) + (tid - 18);
    else if (tid < 39) src = reinterpret_cast<const unsigned long long*>(P.intr + (size_t)p * 32) + (tid - 30);
    else if (tid < 48) src = reinterpret_cast<const unsigned long long*>(P.intr + (size_t)p * 32) + 16 + (tid - 39);
    word = *src;
  }
  static_assert(sizeof(LmCtl) == 18 * 8 && sizeof(LmOpts) == 12 * 8, "layout of the gathered decision inputs");
  // statistics in frame order: thread (chunk, column) adds the rows of its chunk of consecutive frames one after the other,
  // then one thread per column adds the 64 chunks in order -- fixed by F alone
  {
    const int col = tid & 3, chunk = tid >> 2;
    const int len = (F + 63) / 64;
    const int r0 = chunk * len, r1 = min(F, r0 + len);
    double a = 0.0;
    for (int r = r0; r < r1; ++r) a += P.stats[(size_t)(f0 + r) * kStatsCols + col];
    s_part[chunk * 4 + col] = a;
  }
  if (tid < 48) s_in[tid] = word;
  __syncthreads();
  const LmCtl& c_in = *reinterpret_cast<const LmCtl*>(s_in);
  const LmOpts& o_in = *reinterpret_cast<const LmOpts*>(s_in + 18);
  const double* k_in0 = reinterpret_cast<const double*>(s_in + 30);
  const double* k_in1 = reinterpret_cast<const double*>(s_in + 39);
  if (c_in.done) return;   // untouched
  const int phase = c_in.phase;
  const bool pending = c_in.cand_pending != 0;
  const bool need = phase == 0 || (pending && c_in.step_valid);
  const uint32_t mask = P.mask[p];
  if (phase == 0) {   // diagonal of H_ss summed over the frames, the same way (sixteen chunks)
    const int col = tid & 15, chunk = tid >> 4;
    const int len = (F + 15) / 16;
    const int r0 = chunk * len, r1 = min(F, r0 + len);
    double a = 0.0;
    for (int r = r0; r < r1; ++r) a += P.hd0[(size_t)(f0 + r) * 16 + col];
    s_hpart[chunk * 16 + col] = a;
    __syncthreads();
  }
  if (tid < 4) {
    double a = 0.0;
    for (int c = 0; c < 64; ++c) a += s_part[c * 4 + tid];
    s_tot[tid] = a;
  } else if (tid < 13) {
    double a = 0.0;
    if (phase == 0)
      for (int c = 0; c < 16; ++c) a += s_hpart[c * 16 + (tid - 4)];
    s_tot[tid] = a;
  }
  __syncthreads();
  if (tid == 0) {
    LmCtl c = c_in;
    const LmOpts o = o_in;
    const int len0 = c.log_len;
    double tot[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) tot[i] = need ? s_tot[i] : 0.0;
    const double* kc0 = c.cur ? k_in1 : k_in0;   // accepted intrinsics
    const double* kc1 = c.cur ? k_in0 : k_in1;   // candidate
    if (phase == 0) {
      double xn2 = tot[ST_XNORM2];
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        const double ki = kc0[i];
        xn2 += ki * ki;
        const double sc = o.jacobi_scaling ? 1.0 / (1.0 + sqrt(s_tot[4 + i])) : 1.0;
        s_ss[i] = sc;
        P.ss[(size_t)p * 16 + i] = sc;
      }
      lm_init(c, o, tot[ST_COST], sqrt(xn2));
    } else if (pending) {
      double step2 = tot[ST_STEP2], xn2 = tot[ST_XNORM2];
      if (c.step_valid) {
#pragma unroll
        for (int i = 0; i < 9; ++i) {
          const double kc = kc1[i], k0 = kc0[i];
          const double d = kc - k0;
          step2 += d * d;
          xn2 += kc * kc;
        }
      }
      lm_decide(c, o, &s_log, tot[ST_COST], tot[ST_QMODEL], step2, xn2);
    }
    s_ctl = c;
    s_logged = c.log_len != len0;
  }
  if (phase != 0 && tid < 9) s_ss[tid] = P.ss[(size_t)p * 16 + tid];
  if (tid == 32) {
    int o = 0;
    for (int j = 0; j < 9; ++j)
      for (int k = j; k < 9; ++k) { pj[o] = (unsigned char)j; pk[o] = (unsigned char)k; ++o; }
  }
  __syncthreads();
  const bool stop = s_ctl.done != 0;
  if (!stop) {
    const int cur = s_ctl.cur;
    const bool jac = o_in.jacobi_scaling != 0;
    const double inv_radius = 1.0 / s_ctl.radius;
    const double mn = o_in.min_lm_diagonal, mx = o_in.max_lm_diagonal;
    // Output slots l * 5 + r of this lane: what they read is the same for every frame
    int gi[5], zj[5], zk[5];
    double sa[5], sb[5];
    bool use_z[5];
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const int o = l * 5 + r;
      gi[r] = 0; zj[r] = 0; zk[r] = 0; sa[r] = 0.0; sb[r] = 0.0; use_z[r] = false;
      if (o < 45) {
        const int j = pj[o], k = pk[o];
        gi[r] = j * 16 + k; zj[r] = j; zk[r] = k; sa[r] = s_ss[j]; sb[r] = s_ss[k]; use_z[r] = true;
      } else if (o < 54) {
        const int j = o - 45;
        gi[r] = j * 16 + 15; zj[r] = j; zk[r] = 9; sa[r] = s_ss[j]; sb[r] = 1.0; use_z[r] = true;
      } else if (o < 63) {
        const int j = o - 54;
        gi[r] = j * 17; sa[r] = s_ss[j] * s_ss[j]; sb[r] = 1.0;
      } else if (o >= PC_GS && o < PC_GS + 9) {
        gi[r] = (o - PC_GS) * 16 + 15; sa[r] = 1.0; sb[r] = 1.0;
      }  // PC_FAIL, PC_GMAXP and the padding columns: 0 here, the two live ones are filled in below
    }
    const int l6 = l < 6 ? l : l - 6 < 6 ? l - 6 : l - 12;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    double gacc = 0.0, facc = 0.0;
    // sixteen frames per pass, sixteen lanes per frame; group g adds its frames g, g + 16, ... in that order
    for (int base = 0; base < F; base += 16) {
      const int fl = base + g;
      const bool valid = fl < F;
      const size_t f = (size_t)f0 + (valid ? fl : 0);
      const double* G = P.blocks + ((size_t)cur * P.Ftot + f) * 256;
      double fail = 0.0;
      double gv[5];
#pragma unroll
      for (int r = 0; r < 5; ++r) gv[r] = G[gi[r]];
      const double gpe = G[(9 + l6) * 16 + 15];   // entry l6 of the pose block's gradient
      const double* qf = P.pose + ((size_t)cur * P.Ftot + f) * 8;
      const double qw = qf[0], qx = qf[1], qy = qf[2], qz = qf[3];
      const int col = l < 9 ? l : 15;   // column l (< 10) of [H_ps | g_p]
      double w[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) w[i] = G[(9 + i) * 16 + col];
      if (valid) {
        double s[6], L[21];
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int j = 0; j <= i; ++j) L[tri(i, j)] = G[(9 + i) * 16 + 9 + j];
        if (phase == 0) {
          // first elimination: Jacobi scale of this frame's pose block (Ceres: 1 / (1 + sqrt(diag J^T J)), once)
#pragma unroll
          for (int i = 0; i < 6; ++i) s[i] = jac ? 1.0 / (1.0 + sqrt(L[tri(i, i)])) : 1.0;
          if (l < 6) P.sp[f * 8 + l] = jac ? 1.0 / (1.0 + sqrt(G[(9 + l) * 17])) : 1.0;
        } else {
#pragma unroll
          for (int i = 0; i < 6; ++i) s[i] = P.sp[f * 8 + i];
        }
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int j = 0; j <= i; ++j) L[tri(i, j)] = s[i] * L[tri(i, j)] * s[j];
#pragma unroll
        for (int i = 0; i < 6; ++i) L[tri(i, i)] += clampd(L[tri(i, i)], mn, mx) * inv_radius;
        // in-place Cholesky (lower) in registers, redundant per lane; L_jj = d * rsqrt(d), 1 / L_jj = rsqrt(d)
        bool ok = true;
        double Li[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          double d = L[tri(j, j)];
#pragma unroll
          for (int k = 0; k < j; ++k) d -= L[tri(j, k)] * L[tri(j, k)];
          ok = ok && (d > 0.0) && isfinite(d);
          const double inv = rsqrt_pos(d);
          L[tri(j, j)] = d * inv;
          Li[j] = inv;
#pragma unroll
          for (int i = j + 1; i < 6; ++i) {
            double a = L[tri(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) a -= L[tri(i, k)] * L[tri(j, k)];
            L[tri(i, j)] = a * inv;
          }
        }
        if (!ok) fail = 1.0;
        if (l < 10) {
          // z = L^-1 w (for the Schur sums), y = L^-T z (for the back-substitution)
          const double sc = l < 9 ? s_ss[l] : 1.0;
          double z[6], y[6];
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            double a = s[i] * w[i] * sc;
#pragma unroll
            for (int k = 0; k < i; ++k) a -= L[tri(i, k)] * z[k];
            z[i] = a * Li[i];
          }
#pragma unroll
          for (int i = 5; i >= 0; --i) {
            double a = z[i];
#pragma unroll
            for (int k = i + 1; k < 6; ++k) a -= L[tri(k, i)] * y[k];
            y[i] = a * Li[i];
          }
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            Zs[g][i * 10 + l] = z[i];
            P.Y[f * kYStride + i * 10 + l] = y[i];
          }
        }
      }
      __syncthreads();
      if (valid) {
#pragma unroll
        for (int r = 0; r < 5; ++r) {
          double zz = 0.0;
#pragma unroll
          for (int i = 0; i < 6; ++i) zz += Zs[g][i * 10 + zj[r]] * Zs[g][i * 10 + zk[r]];
          acc[r] += sa[r] * gv[r] * sb[r] - (use_z[r] ? zz : 0.0);
        }
        {   // the frame's share of Ceres' gradient_max_norm, ||x - Plus(x, -g)||_inf (pose_grad_proj_max, cc_common.hpp)
          const int base16 = (threadIdx.x & 63) & ~15;
          double g6[6];
#pragma unroll
          for (int i = 0; i < 6; ++i) g6[i] = __shfl(gpe, base16 + i, 64);
          const double q4[4] = {qw, qx, qy, qz};
          gacc = fmax(gacc, pose_grad_proj_max(q4, g6));
        }
        facc += fail;
      }
      __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 5; ++r)
      if (l * 5 + r != PC_FAIL && l * 5 + r != PC_GMAXP) red[g][l * 5 + r] = acc[r];
    gacc = row16_max(gacc);
    if (l == 0) { red[g][PC_FAIL] = facc; red[g][PC_GMAXP] = gacc; }
    __syncthreads();
    if (tid < kPartialCols) {   // the sixteen groups in order
      double a = 0.0;
      if (tid == PC_GMAXP) { for (int g2 = 0; g2 < 16; ++g2) a = fmax(a, red[g2][tid]); }
      else { for (int g2 = 0; g2 < 16; ++g2) a += red[g2][tid]; }
      sv[tid] = a;
    }
    __syncthreads();
  }
  if (tid >= 64) return;

  // ---- wave 0: gradient / radius tests of the accepted point, then the reduced 9 x 9 system with its rows spread over
  // the lanes (chol_solve_rows); every lane carries the same copy of the control block, lane 0 writes it back
  LmCtl c = s_ctl;
  const LmOpts o = o_in;
  cc_iteration* e = (tid == 0 && s_logged) ? &s_log : nullptr;
  bool go = false;
  if (!stop) {
    double gmax = sv[PC_GMAXP];
#pragma unroll
    for (int j = 0; j < 9; ++j)
      if (!(mask & (1u << j))) gmax = fmax(gmax, fabs(sv[PC_GS + j]));
    if (e && e->accepted) e->gradient_max_norm = gmax;
    go = lm_finalize(c, o, gmax);
  }
  if (go) {   // (the same answer in every lane)
    const int i = tid < 9 ? tid : 8;   // lanes beyond the ninth repeat row 8: finite, never read
    const bool held_i = ((mask >> i) & 1u) != 0;
    double a[9], x[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) a[j] = j <= i ? sv[upper_index(j, i)] : 0.0;
    const double dg = clampd(sv[PC_HDIAG + i], o.min_lm_diagonal, o.max_lm_diagonal) / c.radius;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      if (j == i) a[j] += dg;
      if (held_i || ((mask >> j) & 1u)) a[j] = j == i ? 1.0 : 0.0;   // a constant coordinate: identity row and column
    }
    const double b = held_i ? 0.0 : sv[PC_B + i];
    bool ok = chol_solve_rows<9>(a, b, x);
    ok = ok && !(sv[PC_FAIL] > 0.0);
#pragma unroll
    for (int j = 0; j < 9; ++j) ok = ok && isfinite(x[j]);
    if (tid == 0) {
#pragma unroll
      for (int j = 0; j < 9; ++j) P.ds[(size_t)p * 16 + j] = -x[j];
    }
    c.step_valid = ok ? 1 : 0;
    c.cand_pending = 1;
  }
  if (tid != 0) return;
  if (e && c.log_len <= P.log_cap) P.log[(size_t)(c.log_len - 1) * P.B + p] = *e;
  P.ctl[p] = c;
}

// Head of a solve: a problem whose accepted point sits in buffer 1 (the last solve ended there) gets it moved to buffer 0;
// the control blocks are cleared behind this kernel (stream order).
__global__ __launch_bounds__(256) void k_intrb_begin(IntrBatchDev P) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (int64_t)P.Ftot * 8) {
    const int p = P.where[i >> 3].x;
    if (P.ctl[p].cur & 1) P.pose[i] = P.pose[(size_t)P.Ftot * 8 + i];
  }
  if (i < (int64_t)P.B * 16) {
    const int p = (int)(i >> 4);
    if (P.ctl[p].cur & 1) P.intr[(size_t)p * 32 + (i & 15)] = P.intr[(size_t)p * 32 + 16 + (i & 15)];
  }
}

// ---------------------------------------------------------------------------------------------
// host code without a device call: argument checks, the offset tables, state packing
// ---------------------------------------------------------------------------------------------
// problem_offsets [B + 1] into frames, frame_offsets [Ftot + 1] into observations. Fills first [B + 1] and
// where [Ftot] = {problem, local frame} (int32 pairs). who: the entry point, for the message.
int batch_build_tables(const char* who, int64_t B, const int64_t* problem_offsets, const int64_t* frame_offsets,
                       std::vector<int32_t>* first, std::vector<int32_t>* where) {
  if (B <= 0) return fail(CC_ERR_BAD_ARGUMENT, "%s: n_problems must be positive", who);
  if (!problem_offsets || !frame_offsets) return fail(CC_ERR_BAD_ARGUMENT, "%s: problem_offsets / frame_offsets are NULL", who);
  if (B >= ((int64_t)1 << 24)) return fail(CC_ERR_BAD_ARGUMENT, "%s: too many problems (< 2^24)", who);
  if (problem_offsets[0] != 0) return fail(CC_ERR_BAD_ARGUMENT, "%s: problem_offsets[0] must be 0", who);
  for (int64_t p = 0; p < B; ++p) {
    if (problem_offsets[p + 1] < problem_offsets[p]) return fail(CC_ERR_BAD_ARGUMENT, "%s: problem_offsets must be non-decreasing", who);
    if (problem_offsets[p + 1] == problem_offsets[p]) return fail(CC_ERR_BAD_ARGUMENT, "%s: problem %lld has no frames", who, (long long)p);
  }
  const int64_t Ftot = problem_offsets[B];
  if (Ftot >= ((int64_t)1 << 28)) return fail(CC_ERR_BAD_ARGUMENT, "%s: too many frames (< 2^28 in all)", who);
  if (frame_offsets[0] != 0) return fail(CC_ERR_BAD_ARGUMENT, "%s: frame_offsets[0] must be 0", who);
  for (int64_t f = 0; f < Ftot; ++f)
    if (frame_offsets[f + 1] < frame_offsets[f]) return fail(CC_ERR_BAD_ARGUMENT, "%s: frame_offsets must be non-decreasing", who);
  if (frame_offsets[Ftot] >= ((int64_t)1 << 40)) return fail(CC_ERR_BAD_ARGUMENT, "%s: too many observations (< 2^40 in all)", who);
  first->resize((size_t)B + 1);
  where->resize((size_t)Ftot * 2);
  for (int64_t p = 0; p <= B; ++p) (*first)[(size_t)p] = (int32_t)problem_offsets[p];
  for (int64_t p = 0; p < B; ++p)
    for (int64_t f = problem_offsets[p]; f < problem_offsets[p + 1]; ++f) {
      (*where)[(size_t)f * 2] = (int32_t)p;
      (*where)[(size_t)f * 2 + 1] = (int32_t)(f - problem_offsets[p]);
    }
  return CC_OK;
}

// the caller's state as the device holds it: intr [B][2][16] (both buffers alike), pose [Ftot][8]
void batch_pack_state(int64_t B, int64_t Ftot, const double* intr9, const double* q, const double* t, double* intr_out, double* pose_out) {
  std::memset(intr_out, 0, (size_t)B * 32 * sizeof(double));
  std::memset(pose_out, 0, (size_t)Ftot * 8 * sizeof(double));
  for (int64_t p = 0; p < B; ++p)
    for (int i = 0; i < 9; ++i) intr_out[p * 32 + i] = intr_out[p * 32 + 16 + i] = intr9[p * 9 + i];
  for (int64_t f = 0; f < Ftot; ++f) {
    for (int i = 0; i < 4; ++i) pose_out[f * 8 + i] = q[f * 4 + i];
    for (int i = 0; i < 3; ++i) pose_out[f * 8 + 4 + i] = t[f * 3 + i];
  }
}

}  // namespace cc

// =============================================================================================
// handle
// =============================================================================================
struct cc_intrinsics_batch {
  int device = 0;
  hipStream_t stream = nullptr;
  cc::IntrBatchDev d{};
  int64_t B = 0, Ftot = 0, N = 0;
  std::vector<int32_t> first, where;
  void* arena = nullptr;
  bool arena_cached = false;
  char* extra = nullptr;           // scratch behind the handle's own buffers (cc_intrinsics_batch_estimate's initialisation)
  cc::LmCtl* h_ctl = nullptr;      // pinned, [B]
  uint32_t* d_mask = nullptr;
  cc::LmOpts h_opts{};             // source of the options' upload (alive until the solve's first wait)
  bool have_state = false;
  double* d_huber = nullptr;       // EXTENSION (cc_intrinsics_batch_set_huber): [B] HuberLoss(a) per problem, pixels; <= 0: off
  bool huber_on = false;           // ... on for at least one problem: the solve launches k_intrb_sweep_huber behind k_intrb_sweep
  bool huber_all = false;          // ... on for every problem: k_intrb_sweep has nothing to sweep and is left out
  int model = CC_MODEL_RADTAN;     // EXTENSION (cc_intrinsics_batch_set_model): CC_MODEL_FISHEYE -> k_intrb_sweep_fisheye sweeps every problem
  // EXTENSION (cc_intrinsics_batch_estimate_start_fisheye, cc_intr_start_batch_host.hpp): the start's device scratch, grown on demand,
  // and where the last search's tables lie in it ([B][kIntrStartMaxCandidates] each; start_candidates 0: no search yet)
  std::vector<int64_t> foff;       // [Ftot + 1] the frame offsets as uploaded (the start's workgroup tables are built from them)
  void* start_work = nullptr;
  size_t start_work_bytes = 0;
  int start_candidates = 0;
  const double *start_f = nullptr, *start_score = nullptr;
  const int32_t* start_qualified = nullptr;
};

namespace cc {

static void batch_destroy(cc_intrinsics_batch* h) {
  if (!h) return;
  hipSetDevice(h->device);
  bool stream_ok = true;
  if (h->stream) { stream_ok = hipStreamSynchronize(h->stream) == hipSuccess; (void)hipGetLastError(); }
  if (h->arena) arena_put(h->device, h->arena, h->arena_cached);
  if (h->h_ctl) hipHostFree(h->h_ctl);
  if (h->start_work) (void)hipFree(h->start_work);
  if (stream_ok) stream_put(h->device, h->stream);
  else if (h->stream) hipStreamDestroy(h->stream);
  delete h;
}

// allocation and upload behind the argument checks; `wait`: the caller's arrays may go away after the call
static int batch_create_impl(cc_intrinsics_batch* h, const int64_t* frame_offsets, const float* uv, const float* xyz, size_t extra_bytes, bool wait) {
  const size_t B = (size_t)h->B, F = (size_t)h->Ftot, n1 = (size_t)std::max<int64_t>(h->N, 1);
  if (int rc = stream_get(h->device, &h->stream)) return rc;
  ArenaCursor cur;
  const size_t o_intr = cur.take(B * 32 * sizeof(double));
  const size_t o_pose = cur.take(2 * F * 8 * sizeof(double));
  const size_t o_stats = cur.take(F * kStatsCols * sizeof(double));
  const size_t o_hd0 = cur.take(F * 16 * sizeof(double));
  const size_t o_sp = cur.take(F * 8 * sizeof(double));
  const size_t o_Y = cur.take(F * kYStride * sizeof(double));
  const size_t o_ds = cur.take(B * 16 * sizeof(double));
  const size_t o_ss = cur.take(B * 16 * sizeof(double));
  const size_t o_ctl = cur.take(B * sizeof(LmCtl));
  const size_t o_opts = cur.take(sizeof(LmOpts));
  const size_t o_mask = cur.take(B * sizeof(uint32_t));
  const size_t o_huber = cur.take(B * sizeof(double));
  const size_t zeroed = cur.bytes;   // everything above starts as zeros
  const size_t o_blocks = cur.take(2 * F * 256 * sizeof(double));
  const size_t o_log = cur.take((size_t)kBatchLogCap * B * sizeof(cc_iteration));
  const size_t o_uv = cur.take(n1 * 2 * sizeof(float));
  const size_t o_xyz = cur.take(n1 * 3 * sizeof(float));
  const size_t o_off = cur.take((F + 1) * sizeof(int64_t));
  const size_t o_where = cur.take(F * 2 * sizeof(int32_t));
  const size_t o_first = cur.take((B + 1) * sizeof(int32_t));
  const size_t o_extra = cur.take(extra_bytes);
  if (int rc = arena_get(h->device, cur.bytes, &h->arena, &h->arena_cached)) return rc;
  char* base = static_cast<char*>(h->arena);
  h->extra = extra_bytes ? base + o_extra : nullptr;
  CC_HIP(hipHostMalloc(reinterpret_cast<void**>(&h->h_ctl), B * sizeof(LmCtl), hipHostMallocDefault));
  CC_HIP(hipMemsetAsync(base, 0, zeroed, h->stream));
  if (h->N > 0) {
    CC_HIP(hipMemcpyAsync(base + o_uv, uv, (size_t)h->N * 2 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    CC_HIP(hipMemcpyAsync(base + o_xyz, xyz, (size_t)h->N * 3 * sizeof(float), hipMemcpyHostToDevice, h->stream));
  }
  CC_HIP(hipMemcpyAsync(base + o_off, frame_offsets, (F + 1) * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  CC_HIP(hipMemcpyAsync(base + o_where, h->where.data(), F * 2 * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  CC_HIP(hipMemcpyAsync(base + o_first, h->first.data(), (B + 1) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  if (wait) CC_HIP(hipStreamSynchronize(h->stream));
  IntrBatchDev& d = h->d;
  d.N = h->N; d.B = (int32_t)B; d.Ftot = (int32_t)F;
  d.uv = reinterpret_cast<const float*>(base + o_uv);
  d.xyz = reinterpret_cast<const float*>(base + o_xyz);
  d.off = reinterpret_cast<const int64_t*>(base + o_off);
  d.where = reinterpret_cast<const int2*>(base + o_where);
  d.first = reinterpret_cast<const int32_t*>(base + o_first);
  h->d_mask = reinterpret_cast<uint32_t*>(base + o_mask);
  d.mask = h->d_mask;
  h->d_huber = reinterpret_cast<double*>(base + o_huber);
  d.intr = reinterpret_cast<double*>(base + o_intr);
  d.pose = reinterpret_cast<double*>(base + o_pose);
  d.blocks = reinterpret_cast<double*>(base + o_blocks);
  d.stats = reinterpret_cast<double*>(base + o_stats);
  d.hd0 = reinterpret_cast<double*>(base + o_hd0);
  d.sp = reinterpret_cast<double*>(base + o_sp);
  d.Y = reinterpret_cast<double*>(base + o_Y);
  d.ds = reinterpret_cast<double*>(base + o_ds);
  d.ss = reinterpret_cast<double*>(base + o_ss);
  d.ctl = reinterpret_cast<LmCtl*>(base + o_ctl);
  d.opts = reinterpret_cast<const LmOpts*>(base + o_opts);
  d.log = reinterpret_cast<cc_iteration*>(base + o_log);
  d.log_cap = kBatchLogCap;
  d.pad_ = 0;
  CC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_intrb_sweep), hipFuncAttributeMaxDynamicSharedMemorySize, kSweepLdsBytes));
  if (int rc = batch_sweep_huber_prepare()) return rc;
  if (int rc = batch_sweep_fisheye_prepare()) return rc;
  return CC_OK;
}

static int batch_create(const char* who, int32_t device, int64_t B, const int64_t* problem_offsets, const int64_t* frame_offsets,
                        const float* uv, const float* xyz, size_t extra_per_frame, size_t extra_per_problem, bool wait, cc_intrinsics_batch** out) {
  if (!out) return fail(CC_ERR_BAD_ARGUMENT, "%s: the handle pointer is NULL", who);
  *out = nullptr;
  std::vector<int32_t> first, where;
  if (int rc = batch_build_tables(who, B, problem_offsets, frame_offsets, &first, &where)) return rc;
  const int64_t Ftot = problem_offsets[B], N = frame_offsets[Ftot];
  if (N > 0 && (!uv || !xyz)) return fail(CC_ERR_BAD_ARGUMENT, "%s: uv / xyz are NULL", who);
  if (int rc = select_device(device)) return rc;
  cc_intrinsics_batch* h = new cc_intrinsics_batch();
  h->device = device; h->B = B; h->Ftot = Ftot; h->N = N;
  h->first.swap(first);
  h->where.swap(where);
  h->foff.assign(frame_offsets, frame_offsets + Ftot + 1);
  const size_t extra = extra_per_frame * (size_t)Ftot + extra_per_problem * (size_t)B;
  if (int rc = batch_create_impl(h, frame_offsets, uv, xyz, extra, wait)) { batch_destroy(h); return rc; }
  *out = h;
  return CC_OK;
}

static int batch_read_ctl(cc_intrinsics_batch* h) {
  CC_HIP(hipMemcpyAsync(h->h_ctl, h->d.ctl, (size_t)h->B * sizeof(LmCtl), hipMemcpyDeviceToHost, h->stream));
  CC_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

}  // namespace cc

extern "C" {

int cc_intrinsics_batch_create(int32_t device, int64_t n_problems, const int64_t* problem_offsets, const int64_t* frame_offsets,
                               const float* uv, const float* xyz, cc_intrinsics_batch** out) {
  return cc::batch_create("cc_intrinsics_batch_create", device, n_problems, problem_offsets, frame_offsets, uv, xyz, 0, 0, true, out);
}

void cc_intrinsics_batch_destroy(cc_intrinsics_batch* h) { cc::batch_destroy(h); }

int cc_intrinsics_batch_set_state(cc_intrinsics_batch* h, const double* intr9, const uint32_t* const_mask, const double* q, const double* t) {
  using namespace cc;
  if (!h || !intr9 || !q || !t) return fail(CC_ERR_BAD_ARGUMENT, "cc_intrinsics_batch_set_state: NULL argument");
  CC_HIP(hipSetDevice(h->device));
  std::vector<double> intr((size_t)h->B * 32), pose((size_t)h->Ftot * 8);
  batch_pack_state(h->B, h->Ftot, intr9, q, t, intr.data(), pose.data());
  std::vector<uint32_t> mask((size_t)h->B, 0u);
  if (const_mask) for (int64_t p = 0; p < h->B; ++p) mask[(size_t)p] = const_mask[p] & 0x1ffu;
  if (h->model == CC_MODEL_FISHEYE)   // EXTENSION: slot 8 is unused by the fisheye model: held, and 0, for every problem
    for (int64_t p = 0; p < h->B; ++p) {
      intr[(size_t)p * 32 + 8] = intr[(size_t)p * 32 + 16 + 8] = 0.0;
      mask[(size_t)p] |= 1u << 8;
    }
  CC_HIP(hipStreamSynchronize(h->stream));
  CC_HIP(hipMemcpy(h->d.intr, intr.data(), intr.size() * sizeof(double), hipMemcpyHostToDevice));
  CC_HIP(hipMemcpy(h->d.pose, pose.data(), pose.size() * sizeof(double), hipMemcpyHostToDevice));   // buffer 0
  CC_HIP(hipMemcpy(h->d_mask, mask.data(), mask.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  CC_HIP(hipMemsetAsync(h->d.ctl, 0, (size_t)h->B * sizeof(LmCtl), h->stream));   // the point is in buffer 0
  CC_HIP(hipStreamSynchronize(h->stream));
  h->have_state = true;
  return CC_OK;
}

// EXTENSION: ceres::HuberLoss(a_pixels[p]) for problem p in later solves (cc_intrinsics_huber.hpp); <= 0: off, NULL: all off.
int cc_intrinsics_batch_set_huber(cc_intrinsics_batch* h, const double* a_pixels) {
  using namespace cc;
  if (!h) return fail(CC_ERR_BAD_ARGUMENT, "cc_intrinsics_batch_set_huber: NULL handle");
  std::vector<double> a((size_t)h->B, 0.0);
  bool on = false, all = a_pixels != nullptr;
  if (a_pixels)
    for (int64_t p = 0; p < h->B; ++p) {
      if (a_pixels[p] != a_pixels[p]) return fail(CC_ERR_BAD_ARGUMENT, "cc_intrinsics_batch_set_huber: a_pixels[%lld] is NaN", (long long)p);
      a[(size_t)p] = a_pixels[p] > 0.0 ? a_pixels[p] : 0.0;
      on = on || a_pixels[p] > 0.0;
      all = all && a_pixels[p] > 0.0;
    }
  CC_HIP(hipSetDevice(h->device));
  CC_HIP(hipStreamSynchronize(h->stream));
  CC_HIP(hipMemcpy(h->d_huber, a.data(), a.size() * sizeof(double), hipMemcpyHostToDevice));
  h->huber_on = on;
  h->huber_all = all;
  return CC_OK;
}

// EXTENSION: the camera model of later set_state / solve / get_state calls (cc_intrinsics_fisheye.hpp), ONE for the whole batch.
// The slots of the state mean something else under another model, so a change drops the state: cc_intrinsics_batch_set_state
// comes next. The Huber thresholds stay. No device call.
int cc_intrinsics_batch_set_model(cc_intrinsics_batch* h, int32_t model) {
  using namespace cc;
  if (!h) return fail(CC_ERR_BAD_ARGUMENT, "cc_intrinsics_batch_set_model: NULL handle");
  if (model != CC_MODEL_RADTAN && model != CC_MODEL_FISHEYE) return fail(CC_ERR_BAD_ARGUMENT, "cc_intrinsics_batch_set_model: unknown model %d", (int)model);
  if (model == h->model) return CC_OK;
  h->model = model;
  h->have_state = false;
  return CC_OK;
}

int cc_intrinsics_batch_get_model(const cc_intrinsics_batch* h, int32_t* model) {
  using namespace cc;
  if (!h || !model) return fail(CC_ERR_BAD_ARGUMENT, "cc_intrinsics_batch_get_model: NULL argument");
  *model = h->model;
  return CC_OK;
}

int cc_intrinsics_batch_get_state(cc_intrinsics_batch* h, double* intr9, double* q, double* t) {
  using namespace cc;
  if (!h) return fail(CC_ERR_BAD_ARGUMENT, "cc_intrinsics_batch_get_state: NULL handle");
  if (!h->have_state) return fail(CC_ERR_STATE, "cc_intrinsics_batch_get_state: no state set");
  CC_HIP(hipSetDevice(h->device));
  if (int rc = batch_read_ctl(h)) return rc;
  if (intr9) {
    std::vector<double> intr((size_t)h->B * 32);
    CC_HIP(hipMemcpy(intr.data(), h->d.intr, intr.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t p = 0; p < h->B; ++p)
      for (int i = 0; i < 9; ++i) intr9[p * 9 + i] = intr[(size_t)p * 32 + (h->h_ctl[p].cur & 1) * 16 + i];
  }
  if (q || t) {
    std::vector<double> pose((size_t)2 * h->Ftot * 8);
    CC_HIP(hipMemcpy(pose.data(), h->d.pose, pose.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t f = 0; f < h->Ftot; ++f) {
      const int cur = h->h_ctl[h->where[(size_t)f * 2]].cur & 1;
      const double* s = pose.data() + ((size_t)cur * h->Ftot + f) * 8;
      if (q) for (int i = 0; i < 4; ++i) q[f * 4 + i] = s[i];
      if (t) for (int i = 0; i < 3; ++i) t[f * 3 + i] = s[4 + i];
    }
  }
  return CC_OK;
}

int cc_intrinsics_batch_solve(cc_intrinsics_batch* h, const cc_options* opt, cc_summary* summaries) {
  using namespace cc;
  if (!h) return fail(CC_ERR_BAD_ARGUMENT, "cc_intrinsics_batch_solve: NULL handle");
  if (!h->have_state) return fail(CC_ERR_STATE, "cc_intrinsics_batch_solve: no state set");
  const auto t0 = std::chrono::steady_clock::now();
  cc_options o;
  if (opt) o = *opt; else cc_options_init(&o);
  if (o.profile_kernels) return fail(CC_ERR_BAD_ARGUMENT, "cc_intrinsics_batch_solve: profile_kernels is not supported by the batched solve");
  if (o.check_interval < 1) o.check_interval = 1;
  if (o.max_iterations > h->d.log_cap - 1) o.max_iterations = h->d.log_cap - 1;
  CC_HIP(hipSetDevice(h->device));
  opts_from_public(o, &h->h_opts);
  const int64_t B = h->B;
  // the accepted point of a previous solve moves to buffer 0, fresh control blocks, the options
  const unsigned begin_blocks = (unsigned)((std::max<int64_t>(h->Ftot * 8, B * 16) + 255) / 256);
  hipLaunchKernelGGL(k_intrb_begin, dim3(begin_blocks), dim3(256), 0, h->stream, h->d);
  CC_HIP(hipMemsetAsync(h->d.ctl, 0, (size_t)B * sizeof(LmCtl), h->stream));
  CC_HIP(hipMemcpyAsync(const_cast<LmOpts*>(h->d.opts), &h->h_opts, sizeof(LmOpts), hipMemcpyHostToDevice, h->stream));
  int launched = 0;
  for (int chunk = 0;; ++chunk) {
    // plain launches, stream order only; the first chunk holds the initial evaluation plus check_interval iterations
    const int n = o.check_interval + (chunk == 0 ? 1 : 0);
    for (int i = 0; i < n; ++i) {
      // (EXTENSION, cc_intrinsics_batch_huber.hip: the problems with a Huber loss are swept again by the robust kernel, which
      // overwrites their blocks and statistics; the plain ones keep k_intrb_sweep's bits)
      // (EXTENSION, cc_intrinsics_batch_fisheye.hip: a fisheye handle's one sweep serves every problem, loss on or off)
      if (h->model == CC_MODEL_FISHEYE) {
        batch_sweep_fisheye_launch(h->d, h->d_huber, h->stream);
      } else {
        if (!h->huber_all) hipLaunchKernelGGL(k_intrb_sweep, dim3((unsigned)h->Ftot), dim3(kSweepThreads), kSweepLdsBytes, h->stream, h->d);
        if (h->huber_on) batch_sweep_huber_launch(h->d, h->d_huber, h->stream);
      }
      hipLaunchKernelGGL(k_intrb_step, dim3((unsigned)B), dim3(256), 0, h->stream, h->d);
    }
    CC_HIP(hipGetLastError());
    launched += n;
    if (int rc = batch_read_ctl(h)) return rc;   // the B control blocks in one transfer
    bool all_done = true;
    for (int64_t p = 0; p < B; ++p) all_done = all_done && h->h_ctl[p].done != 0;
    if (all_done) break;
    if (launched > o.max_iterations + 2 * o.check_interval + 2) return fail(CC_ERR_STATE, "batched LM loop did not terminate");
  }
  if (summaries) {
    int rows = 0;   // log rows any caller's buffer can take
    for (int64_t p = 0; p < B; ++p) {
      const LmCtl& st = h->h_ctl[p];
      cc_summary& s = summaries[p];
      s.iterations = st.iter;
      s.successful_steps = st.n_success;
      s.termination = st.term;
      s.initial_cost = st.initial_cost;
      s.final_cost = st.x_cost;
      s.sweeps = st.sweeps;
      s.log_len = s.log ? std::min(std::min(st.log_len, s.log_capacity), h->d.log_cap) : 0;
      if (s.log_len < 0) s.log_len = 0;
      rows = std::max(rows, (int)s.log_len);
      for (int i = 0; i < CC_K_COUNT; ++i) { s.kernel_ms[i] = s.kernel_idle_ms[i] = 0.0; s.kernel_launches[i] = s.kernel_idle_launches[i] = 0; }
    }
    if (rows > 0) {
      std::vector<cc_iteration> log((size_t)rows * B);
      CC_HIP(hipMemcpy(log.data(), h->d.log, log.size() * sizeof(cc_iteration), hipMemcpyDeviceToHost));
      for (int64_t p = 0; p < B; ++p)
        for (int r = 0; r < summaries[p].log_len; ++r) summaries[p].log[r] = log[(size_t)r * B + p];
    }
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int64_t p = 0; p < B; ++p) summaries[p].seconds = seconds;
  }
  return CC_OK;
}

}  // extern "C"

// EXTENSION: the fisheye focal-length start for every problem of a batch, on a handle (cc_intrinsics_batch_estimate_start_fisheye,
// cc_intrinsics_batch_start_scores; the one-shot pipeline below runs it too)
#include "cc_intr_start_batch_host.hpp"

// The one-shot calls (cc_intrinsics_batch_optimize, cc_intrinsics_batch_estimate and its _huber / _model / _start forms): one body
// -- the checks, a handle, a start, set_state -> set_huber -> solve -> get_state -- and one filled-in BatchOneShot per entry point.
namespace cc {

struct BatchOneShot {
  const char* who;                // the call's name in every message
  const cc_options* opt;
  int32_t device;
  int64_t B;                      // n_problems
  const int64_t *problem_offsets, *frame_offsets;
  const float *uv, *xyz;
  const uint32_t* const_mask;
  double *intr9, *q, *t;          // CALLER: the start on entry; every start: the solution on return
  cc_summary* summaries;          // (the public calls' arguments, in their order)
  // The start: the caller's state; Zhang's closed form per problem on the handle's device arrays, K and poses rounded to float as
  // cc_intrinsics_estimate hands them over; or the batched fisheye focal search (`search`).
  enum Start { CALLER, ZHANG, FOCAL_SEARCH } start = CALLER;
  const cc_intr_start_options* search = nullptr;
  const double* distortion5 = nullptr;   // ZHANG / FOCAL_SEARCH: [B][5] where the distortion starts (NULL: zeros; fisheye: k1..k4, the fifth ignored)
  float* K_init9 = nullptr;              // ... and [B][9] where the start's K goes (may be NULL)
  const double* huber_a = nullptr;       // EXTENSION: [B] or NULL
  int32_t model = CC_MODEL_RADTAN;       // EXTENSION: the camera model of the whole batch
};

// scratch of Zhang's initialisation, per frame: gram double[256] | H float[9] (padded to 12) | q float[4] | t float[3] (padded to 4);
// per problem: K float[9] (padded to 64 bytes)
constexpr size_t kBatchZhangPerFrame = 256 * sizeof(double) + 12 * sizeof(float) + 4 * sizeof(float) + 4 * sizeof(float), kBatchZhangPerProblem = 64;

// Zhang per problem (zhang_on_device, the handle's stream): K_init9, intr9[p][0..3], q and t. Its wait covers the upload.
static int batch_start_zhang(cc_intrinsics_batch* h, const BatchOneShot& a) {
  const size_t B = (size_t)h->B, F = (size_t)h->Ftot;
  double* dgram = reinterpret_cast<double*>(h->extra);
  float* dH = reinterpret_cast<float*>(h->extra + F * 256 * sizeof(double));
  float* dq = dH + F * 12;
  float* dt = dq + F * 4;
  float* dK = dt + F * 4;   // [B][16]
  for (size_t p = 0; p < B; ++p) {
    const int64_t f0 = a.problem_offsets[p], Fp = a.problem_offsets[p + 1] - f0;
    if (int rc = zhang_on_device(h->stream, Fp, h->d.off + f0, h->d.uv, h->d.xyz, dgram + (size_t)f0 * 256, dH + (size_t)f0 * 9,
                                 dK + p * 16, dq + (size_t)f0 * 4, dt + (size_t)f0 * 3)) return rc;
  }
  std::vector<float> Kf(B * 16), qf(F * 4), tf(F * 3);
  CC_HIP(hipMemcpyAsync(Kf.data(), dK, Kf.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  CC_HIP(hipMemcpyAsync(qf.data(), dq, qf.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  CC_HIP(hipMemcpyAsync(tf.data(), dt, tf.size() * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  CC_HIP(hipStreamSynchronize(h->stream));   // (covers the upload: uv / xyz are the caller's)
  for (size_t p = 0; p < B; ++p) {
    const float* K9 = Kf.data() + p * 16;
    if (a.K_init9) std::memcpy(a.K_init9 + p * 9, K9, 9 * sizeof(float));
    double* k = a.intr9 + p * 9;
    k[0] = K9[0]; k[1] = K9[4]; k[2] = K9[2]; k[3] = K9[5];
  }
  for (size_t i = 0; i < qf.size(); ++i) a.q[i] = qf[i];
  for (size_t i = 0; i < tf.size(); ++i) a.t[i] = tf[i];
  return CC_OK;
}

// The batched focal search in the arena's scratch (L): intr9[p][0..3], q and t are its picks, K_init9 those Ks. One host wait,
// which covers the upload.
static int batch_start_search(cc_intrinsics_batch* h, const BatchOneShot& a, const IntrStartBatchTables& tables, const IntrStartBatchLayout& L) {
  IntrStartBatchOutcome outcome;
  int rc = intr_start_batch_run(h, h->extra, tables, L, *a.search, a.who, a.intr9, a.q, a.t, nullptr, &outcome);
  if (rc == CC_ERR_STATE) {   // (the data admit no start: the caller's arguments, not a state of a handle the caller has)
    const std::string why = last_error();
    rc = fail(CC_ERR_BAD_ARGUMENT, "%s", why.c_str());
  }
  if (rc) return rc;
  if (outcome.invalid_problem >= 0)
    return fail(CC_ERR_BAD_ARGUMENT, "%s: problem %lld: view %lld has no pose at any candidate focal length (fewer than 4 points, collinear points, or a non-finite pixel or point)",
                a.who, (long long)outcome.invalid_problem, (long long)outcome.invalid_view);
  if (a.K_init9)
    for (int64_t p = 0; p < a.B; ++p) {
      const double* k = a.intr9 + p * 9;
      const float K9[9] = {(float)k[0], 0.0f, (float)k[2], 0.0f, (float)k[1], (float)k[3], 0.0f, 0.0f, 1.0f};
      std::memcpy(a.K_init9 + p * 9, K9, sizeof(K9));
    }
  return CC_OK;
}

static int batch_one_shot(const BatchOneShot& a) {
  const char* who = a.who;
  const int64_t B = a.B;
  // Which refusal wins when several apply belongs to each symbol as it is: the Zhang call names an unknown model ahead of a NaN
  // threshold, the search call its model and its options behind one.
  if (!a.intr9 || !a.q || !a.t) return fail(CC_ERR_BAD_ARGUMENT, "%s: intr9 / q / t are NULL", who);
  if (a.start == BatchOneShot::ZHANG && a.model != CC_MODEL_RADTAN && a.model != CC_MODEL_FISHEYE)
    return fail(CC_ERR_BAD_ARGUMENT, "%s: unknown model %d", who, (int)a.model);
  if (a.huber_a)
    for (int64_t p = 0; p < B; ++p)
      if (a.huber_a[p] != a.huber_a[p]) return fail(CC_ERR_BAD_ARGUMENT, "%s: huber_a[%lld] is NaN", who, (long long)p);
  if (a.start == BatchOneShot::FOCAL_SEARCH) {
    if (a.model != CC_MODEL_FISHEYE) return fail(CC_ERR_BAD_ARGUMENT, "%s: the focal-length search is a start of the fisheye model (model %d)", who, (int)a.model);
    if (int rc = intr_start_check(*a.search, who)) return rc;
  }
  IntrStartBatchTables tables;
  IntrStartBatchLayout L(0, 0, 0, 0, 0);   // (the search's)
  size_t per_frame = 0, per_problem = 0;   // the start's scratch, a part of the one-shot arena (batch_create sizes it per frame and per problem)
  if (a.start != BatchOneShot::CALLER) {   // the start's preconditions, before any device call
    std::vector<int32_t> first, where;
    if (int rc = batch_build_tables(who, B, a.problem_offsets, a.frame_offsets, &first, &where)) return rc;
    for (int64_t p = 0; p < B; ++p) {
      if (a.problem_offsets[p + 1] - a.problem_offsets[p] < 3) return fail(CC_ERR_BAD_ARGUMENT, "%s: problem %lld has fewer than 3 frames", who, (long long)p);
      for (int64_t f = a.problem_offsets[p]; a.start == BatchOneShot::ZHANG && f < a.problem_offsets[p + 1]; ++f)
        if (a.frame_offsets[f + 1] - a.frame_offsets[f] < 4) return fail(CC_ERR_BAD_ARGUMENT, "%s: frame %lld has fewer than 4 points", who, (long long)f);
    }
    if (a.start == BatchOneShot::ZHANG) {
      per_frame = kBatchZhangPerFrame; per_problem = kBatchZhangPerProblem;
    } else {
      intr_start_batch_tables(B, a.problem_offsets, a.frame_offsets, a.search->search_views, &tables);
      L = IntrStartBatchLayout(B, a.problem_offsets[B], tables.searched[(size_t)B], (int64_t)tables.extent.size(), a.search->candidates);
      per_problem = (L.bytes + (size_t)B - 1) / (size_t)B;
    }
  }
  cc_intrinsics_batch* h = nullptr;
  // (the caller's state needs no start whose wait would cover the upload: the handle's creation waits for it, as it always has)
  if (int rc = batch_create(who, a.device, B, a.problem_offsets, a.frame_offsets, a.uv, a.xyz, per_frame, per_problem, a.start == BatchOneShot::CALLER, &h)) return rc;
  struct Guard { cc_intrinsics_batch* h; ~Guard() { batch_destroy(h); } } guard{h};
  h->model = a.model;   // (a fresh handle: no state yet)
  if (a.start != BatchOneShot::CALLER) {
    if (int rc = a.start == BatchOneShot::ZHANG ? batch_start_zhang(h, a) : batch_start_search(h, a, tables, L)) {
      (void)hipStreamSynchronize(h->stream);   // (uv / xyz are the caller's: nothing of them is in flight when the call returns)
      return rc;
    }
    for (int64_t p = 0; p < B; ++p) {   // the distortion starts from the caller's
      double* k = a.intr9 + p * 9;
      for (int i = 0; i < 5; ++i) k[4 + i] = a.distortion5 ? a.distortion5[p * 5 + i] : 0.0;
      if (a.model == CC_MODEL_FISHEYE) k[8] = 0.0;
    }
  }
  int rc = cc_intrinsics_batch_set_state(h, a.intr9, a.const_mask, a.q, a.t);
  if (!rc && a.huber_a) rc = cc_intrinsics_batch_set_huber(h, a.huber_a);
  if (!rc) rc = cc_intrinsics_batch_solve(h, a.opt, a.summaries);
  if (!rc) rc = cc_intrinsics_batch_get_state(h, a.intr9, a.q, a.t);
  return rc;
}

}  // namespace cc

extern "C" {

int cc_intrinsics_batch_optimize(const cc_options* opt, int32_t device, int64_t n_problems, const int64_t* problem_offsets,
                                 const int64_t* frame_offsets, const float* uv, const float* xyz, double* intr9,
                                 const uint32_t* const_mask, double* q, double* t, cc_summary* summaries) {
  const cc::BatchOneShot a{"cc_intrinsics_batch_optimize", opt, device, n_problems, problem_offsets, frame_offsets, uv, xyz, const_mask, intr9, q, t, summaries};
  return cc::batch_one_shot(a);
}

// Calibrator::Estimate for every problem of the batch: Zhang's closed-form initialisation per problem on the handle's
// device arrays (zhang_on_device, same stream), its K and poses rounded to float as cc_intrinsics_estimate hands them
// over, then the batched solve. distortion5 [B][5] (may be NULL: zeros), const_mask [B] (may be NULL), K_init9 [B][9] (may be NULL).
// (huber_a [B] or NULL: EXTENSION, a Huber loss per problem; cc_intrinsics_batch_estimate is this with NULL -- the same path, bit for bit)
// (model: EXTENSION, the camera model of the whole batch; cc_intrinsics_batch_estimate_huber is this with CC_MODEL_RADTAN -- the
// same path, bit for bit. With the fisheye model the start is still Zhang's pinhole K and poses, distortion5[p] holds k1..k4
// and its fifth entry is ignored.)
int cc_intrinsics_batch_estimate_model(const cc_options* opt, int32_t device, int64_t n_problems, const int64_t* problem_offsets,
                                       const int64_t* frame_offsets, const float* uv, const float* xyz, const double* distortion5,
                                       const uint32_t* const_mask, float* K_init9, double* intr9, double* q, double* t, cc_summary* summaries,
                                       const double* huber_a, int32_t model) {
  return cc_intrinsics_batch_estimate_start(opt, device, n_problems, problem_offsets, frame_offsets, uv, xyz, distortion5, const_mask,
                                            K_init9, intr9, q, t, summaries, huber_a, model, nullptr);
}

int cc_intrinsics_batch_estimate_huber(const cc_options* opt, int32_t device, int64_t n_problems, const int64_t* problem_offsets,
                                       const int64_t* frame_offsets, const float* uv, const float* xyz, const double* distortion5,
                                       const uint32_t* const_mask, float* K_init9, double* intr9, double* q, double* t, cc_summary* summaries,
                                       const double* huber_a) {
  return cc_intrinsics_batch_estimate_model(opt, device, n_problems, problem_offsets, frame_offsets, uv, xyz, distortion5, const_mask,
                                            K_init9, intr9, q, t, summaries, huber_a, CC_MODEL_RADTAN);
}

int cc_intrinsics_batch_estimate(const cc_options* opt, int32_t device, int64_t n_problems, const int64_t* problem_offsets,
                                 const int64_t* frame_offsets, const float* uv, const float* xyz, const double* distortion5,
                                 const uint32_t* const_mask, float* K_init9, double* intr9, double* q, double* t, cc_summary* summaries) {
  return cc_intrinsics_batch_estimate_huber(opt, device, n_problems, problem_offsets, frame_offsets, uv, xyz, distortion5, const_mask,
                                            K_init9, intr9, q, t, summaries, nullptr);
}

// EXTENSION: cc_intrinsics_batch_estimate_model with the start chosen: NULL -> that call (Zhang, under its name and its checks); else
// the focal search on the fisheye model
int cc_intrinsics_batch_estimate_start(const cc_options* opt, int32_t device, int64_t n_problems, const int64_t* problem_offsets,
                                       const int64_t* frame_offsets, const float* uv, const float* xyz, const double* distortion5,
                                       const uint32_t* const_mask, float* K_init9, double* intr9, double* q, double* t, cc_summary* summaries,
                                       const double* huber_a, int32_t model, const cc_intr_start_options* start) {
  cc::BatchOneShot a{start ? "cc_intrinsics_batch_estimate_start" : "cc_intrinsics_batch_estimate", opt, device, n_problems, problem_offsets, frame_offsets,
                     uv, xyz, const_mask, intr9, q, t, summaries};
  a.start = start ? cc::BatchOneShot::FOCAL_SEARCH : cc::BatchOneShot::ZHANG;
  a.search = start;
  a.distortion5 = distortion5; a.K_init9 = K_init9; a.huber_a = huber_a; a.model = model;
  return cc::batch_one_shot(a);
}

}  // extern "C"
