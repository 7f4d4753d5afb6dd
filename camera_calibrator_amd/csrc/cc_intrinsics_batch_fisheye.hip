// cc_intrinsics_batch_fisheye.hip -- EXTENSION: the batch sweep of the Kannala-Brandt / OpenCV `fisheye` camera model (gfx950;
// the model, its slots and its rows: cc_intrinsics_fisheye.hpp, cc_fisheye_dev.hpp). k_intrb_sweep_fisheye is
// k_intrb_sweep_huber (cc_intrinsics_batch_huber.hip) under a name and in a translation unit of its own -- the two
// radial-tangential sweeps keep their code objects -- with the fisheye rows: same grid (one workgroup of four waves per
// (problem, frame)), same prologue (table, control block, gather, back-substitution and Plus), same staging and MFMA
// contraction, same outputs (blocks, hd0, statistics row with ST_COST = the waves' sum of 1/2 rho).
// The model belongs to the batch (cc_intrinsics_batch_set_model), the loss to a problem: huber_a[p] <= 0 runs the loss with
// a = +inf, as k_intr_sweep_fisheye does -- nothing is in the tail, the weight is exactly 1 and rho = s. So this ONE kernel
// sweeps every problem of a fisheye batch, loss on or off, and a fisheye batch launches it alone each round: no double sweep
// in a mixed-loss batch, and a problem with the loss off gets, bit for bit, what it gets in a batch with no loss at all
// (the same instructions on the same numbers; a threshold of +inf is the same again).
#include "cc_common.hpp"
#include "cc_device.hpp"
#include "cc_intrinsics_dev.hpp"
#include "cc_fisheye_dev.hpp"
#include "cc_intrinsics_batch_dev.hpp"

namespace cc {

// sm layout as in k_intrb_sweep; sm[176..179] the waves' cost sums.
// THREE waves per SIMD, as k_intr_sweep_fisheye and for its reason: the library's atan2 in the loop wants about 150 vector
// registers, which four waves per SIMD (128) do not have (DESIGN.md 4.13 has the register line).
__global__ __launch_bounds__(kSweepThreads, 3) void k_intrb_sweep_fisheye(IntrBatchDev P, const double* huber_a /*[B]*/) {
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
  const double a_p = huber_a[p];
  if (done) return;                              // a finished problem stays untouched while the others iterate
  if (phase != 0 && !step_valid) return;         // no candidate to evaluate: the step kernel shrinks the radius
  const double a = a_p > 0.0 ? a_p : __builtin_huge_val();   // (loss off: the loss whose tail nothing reaches -- weight exactly 1, rho = s)
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
  const double g_old = P.blocks[((cur ? (size_t)Ftot : 0) + f) * 256 + tid];
  if (tid < 116) sm[tid] = gv;
  const int dst = phase == 0 ? cur : (cur ^ 1);
  __syncthreads();
  const int pose_o = cur ? 67 : 60, intr_o = cur ? 83 : 74;
  if (tid < 6) {
    const double* Yr = sm + tid * 10;
    double acc = Yr[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) acc += Yr[j] * sm[92 + j];
    sm[129 + tid] = phase != 0 ? -acc * sm[110 + tid] : 0.0;
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

  double qterm = 0.0;
  if (phase != 0) {
    const int ra = tid >> 4, rb = tid & 15;
    if (ra < 15) qterm = rb < 15 ? 0.5 * sm[120 + ra] * g_old * sm[120 + rb] : sm[120 + ra] * g_old;
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

  double* stage = s_stage + wave * kStageDoublesPerWave;
  d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
  double hcost = 0.0;   // 1/2 sum rho over this lane's observations, in pass order
  for (int ps = 0; ps < npass; ++ps) {
    const int64_t idx = s0 + (int64_t)ps * kSweepThreads + tid;
    const bool valid = idx < s1;  // only the last pass of a frame has idle lanes
    const float2 m = nm;
    const float X0 = nX0, X1 = nX1, X2 = nX2;
    {   // next pass, unconditionally
      const int64_t nidx = idx + kSweepThreads;
      const int64_t ic = nidx < s1 ? nidx : safe0;
      nm = uv2[ic];
      nX0 = P.xyz[ic * 3]; nX1 = P.xyz[ic * 3 + 1]; nX2 = P.xyz[ic * 3 + 2];
    }
    FishCommon oc;
    fisheye_common(kk, R, tt, (double)X0, (double)X1, (double)X2, oc);
    const double ru = kk[0] * oc.xd + kk[2] - (double)m.x, rv = kk[1] * oc.yd + kk[3] - (double)m.y;
    double rho, sr;
    intr_huber(a, ru * ru + rv * rv, rho, sr);
    const double wrow = valid ? sr : 0.0;   // (an idle lane's rows are zero and it adds nothing to the cost)
    hcost += valid ? 0.5 * rho : 0.0;
    double v[16];
    fisheye_row_u(kk, oc, ru, v, wrow);
    stage_row(stage, lane, v);
    wave_lds_fence();
    gram_rows_ahead(stage, lane, acc0, acc1);
    wave_lds_fence();
    fisheye_row_v(kk, oc, rv, v, wrow);
    stage_row(stage, lane, v);
    wave_lds_fence();
    gram_rows_ahead(stage, lane, acc0, acc1);
    wave_lds_fence();
  }
  {
    const double hw = wave_sum(hcost);
    if (lane == 0) sm[176 + wave] = hw;
  }

  // ---- cross-wave reduction of the 16 x 16 block (C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg)
  __syncthreads();  // s_blk aliases the staging buffers
#pragma unroll
  for (int r = 0; r < 4; ++r) s_blk[wave * 256 + ((lane >> 4) + 4 * r) * 16 + (lane & 15)] = acc0[r] + acc1[r];
  __syncthreads();
  const double g = gram_entry_held(mask, tid) ? 0.0 : (s_blk[tid] + s_blk[256 + tid]) + (s_blk[512 + tid] + s_blk[768 + tid]);
  P.blocks[((size_t)dst * Ftot + f) * 256 + tid] = g;
  if (tid == 255) {   // the thread that writes the row in k_intrb_sweep; the cost is the waves' sum of 1/2 rho
    double* st = P.stats + (size_t)f * kStatsCols;
    st[ST_COST] = (sm[176] + sm[177]) + (sm[178] + sm[179]);
    st[ST_QMODEL] = (sm[170] + sm[171]) + (sm[172] + sm[173]);
    st[ST_STEP2] = sm[158];
    st[ST_XNORM2] = sm[159];
  }
  if (phase == 0 && tid < 9 * 17 && tid % 17 == 0) P.hd0[(size_t)f * 16 + tid / 17] = g;
}

}  // namespace cc

namespace cc {

int batch_sweep_fisheye_prepare() {
  CC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_intrb_sweep_fisheye), hipFuncAttributeMaxDynamicSharedMemorySize, kSweepLdsBytes));
  return CC_OK;
}

void batch_sweep_fisheye_launch(const IntrBatchDev& P, const double* huber_a, hipStream_t stream) {
  hipLaunchKernelGGL(k_intrb_sweep_fisheye, dim3((unsigned)P.Ftot), dim3(kSweepThreads), kSweepLdsBytes, stream, P, huber_a);
}

}  // namespace cc
