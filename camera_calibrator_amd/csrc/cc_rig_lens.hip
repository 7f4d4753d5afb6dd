// cc_rig_lens.hip -- kernels of the rig solve with intrinsics for the fisheye pixel model and for a pixel model per camera
// (declarations and the outline: cc_rig_lens.hpp; the models' arithmetic: cc_rig_lens_dev.hpp). A translation unit of its own
// next to cc_rig.hip, whose kernel set is pinned (tests/test_kernel_budgets.py).
#include "cc_common.hpp"
#include "cc_device.hpp"
#include "cc_rig_dev.hpp"
#include "cc_rig_lens.hpp"
#include "cc_rig_lens_dev.hpp"

namespace cc {

// waves per SIMD the sweep is compiled for: three for the radial-tangential rows (<= 168 registers, as k_rig_sweep_adjk), two
// for the fisheye rows. With the library atan2 and the ten quantities of lens_fish_point alive across both rows the compiler
// wants 179 (one wave per group) / 189 (four) registers, and at 168 it spills 2 / 11 with reloads inside the pass loop; at two
// waves per SIMD: no spill, no scratch. One kernel with a uniform branch on the model would put the
// radial-tangential groups at two waves and carry the arctangent's live values through their pass loop.
constexpr int kRigLensWavesRadtan = 3;
constexpr int kRigLensWavesFisheye = 2;
constexpr int kRigLensCompK = 320;  // doubles per group and buffer of the compact record: G (256), M (36) (kRigCompK, cc_rig_sweeps.hpp)

// ---------------------------------------------------------------------------------------------
// k_rig_sweep_adjk (cc_rig_sweeps.hpp) with the rows of MODEL in place of rigk_obs. One workgroup of NW waves per (frame,
// camera) group: the 16 x 16 Gram G of X = [J_cam(6) r J_k(9)] on the matrix pipe, then the three tiles the other kernels
// read, AA = N^T G[0:7, 0:7] N, AB = N^T G[0:7, 7:16], BB = G[7:16, 7:16] with N (7 x 13) = [I6 M 0; 0 0 1], and the compact
// record (G, M) for the next sweep's model-cost term q = 1/2 (e'^T G e' - G[6][6]), e' = [dc + M_old df, 1, dk].
// Workgroup b sweeps group g = b, or with LIST g = glist[b]: the groups of ONE model's cameras. Everything indexed by the group
// -- the wave rotation, the compact record, the tiles, the statistics, the diagonals -- uses g. MODEL and LIST are compile-time
// choices: each instantiation is the text of a kernel written out for it alone.
// ---------------------------------------------------------------------------------------------
template <int NW, int MODEL, bool LIST>
__global__ __launch_bounds__(NW * 64, MODEL == CC_MODEL_FISHEYE ? kRigLensWavesFisheye : kRigLensWavesRadtan)
void k_rig_sweep_lens(RigLensDev P, const int32_t* __restrict__ glist /*not read without LIST*/) {
  constexpr int NT = NW * 64, EPT = 256 / NT;
  __shared__ __attribute__((aligned(16))) double s_stage[NW * kStageDoublesPerWave];   // per wave 64 x 16; then the partial products
  __shared__ double sm[96];        // camera record, frame record, intrinsics record (candidate [0..8], step [16..24])
  __shared__ double s_G[256];      // G
  __shared__ double s_mold[36];    // M of the accepted point
  __shared__ double s_e[16];       // e'
  __shared__ double s_m[36];       // M
  __shared__ double s_w[8];        // per wave: model-cost term, cost
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t g = LIST ? (int64_t)glist[blockIdx.x] : (int64_t)blockIdx.x;
  const int f = P.gframe[g], c = P.gcam[g];
  const int64_t s0 = P.goff[g], s1 = P.goff[g + 1];
  const LmCtl* ctl = P.ctl;
  const int done = ctl->done, phase = ctl->phase, step_valid = ctl->step_valid, cur = ctl->cur;
  if (done) return;
  if (phase != 0 && !step_valid) return;
  const int dst = phase == 0 ? cur : (cur ^ 1);
  const bool fixed = P.cam_fixed[c] != 0;
  const int ks = P.kset[c];
  const int otid = (((tid >> 6) - (int)(g & (NW - 1))) & (NW - 1)) * 64 + lane;
  const int n = (int)(s1 - s0);
  const int wrem = n - (otid >> 6) * 64;
  const int npass = wrem > 0 ? (wrem + NT - 1) / NT : 0;
  const float2* uvg = reinterpret_cast<const float2*>(P.uv) + s0;
  struct F3 { float x, y, z; };
  const F3* xg = reinterpret_cast<const F3*>(P.oxyz) + s0;
  struct ObsRaw { float2 m; F3 X; };
  auto fetch = [&](int k, ObsRaw& r) {   // (unconditional loads: idle slots re-read the group's first observation)
    const int kc = k < n ? k : 0;
    r.m = uvg[kc];
    r.X = xg[kc];
  };
  ObsRaw oa, ob;
  fetch(otid, oa);
  fetch(otid + NT, ob);
  const double* comp_old = P.gcomp + ((size_t)cur * P.NG + g) * kRigLensCompK;
  {
    // records: camera [0..31], frame [32..63], intrinsics [64..95]; M of the accepted point
    const double r0 = tid < 32 ? P.camrec[c * 32 + tid] : (tid < 64 ? P.frec[(size_t)f * 32 + (tid - 32)] : P.krec[ks * 32 + ((tid - 64) & 31)]);
    const double r1 = P.krec[ks * 32 + (tid & 31)];
    const double mo = comp_old[256 + (tid < 36 ? tid : 0)];
    if (tid < 96) sm[tid] = r0;
    if (NW == 1 && tid < 32) sm[64 + tid] = r1;
    if (tid < 36) s_mold[tid] = mo;
  }
  double g_old[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) g_old[e] = comp_old[tid + e * NT];
  __syncthreads();
  // the chain of both poses as one: a = Rc (Rf X + tf) = Rca X + tca. Uniform addresses: scalar loads, values in SGPRs.
  double Rca[9], tca[3], tcs[3], kk[9];
  {
    const double* cr = P.camrec + (size_t)c * 32;
    const double* fr = P.frec + (size_t)f * 32;
    const double* kr = P.krec + (size_t)ks * 32;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) Rca[3 * i + j] = rfl(cr[3 * i] * fr[j] + cr[3 * i + 1] * fr[3 + j] + cr[3 * i + 2] * fr[6 + j]);
      tca[i] = rfl(cr[3 * i] * fr[9] + cr[3 * i + 1] * fr[10] + cr[3 * i + 2] * fr[11]);
      tcs[i] = cr[9 + i];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) kk[i] = kr[i];
  }
  if (tid < 48) {   // M[a][b], a = tid >> 3, b = tid & 7 < 6 (see k_rig_sweep_adj)
    const int a = tid >> 3, b = tid & 7;
    const int a3 = a < 3 ? a : a - 3, b3 = b < 3 ? b : b - 3;
    const int b1 = b3 == 2 ? 0 : b3 + 1, b2 = b3 == 0 ? 2 : b3 - 1;
    const double diag = sm[3 * a3 + (b3 < 3 ? b3 : 0)];
    const double cross = 2.0 * (sm[3 * a3 + b1] * sm[32 + 9 + b2] - sm[3 * a3 + b2] * sm[32 + 9 + b1]);
    const double v = (a < 3) == (b < 3) ? diag : (a >= 3 ? cross : 0.0);
    if (b < 6) s_m[a * 6 + b] = v;
  } else if (tid < 64) {   // e'
    const int t = tid - 48;
    double e = t < 6 ? (fixed ? 0.0 : sm[12 + t]) : (t == 6 ? 1.0 : sm[64 + 16 + (t - 7)]);
    const int row = t < 6 ? t : 0;
#pragma unroll
    for (int b = 0; b < 6; ++b) e = fma(t < 6 ? s_mold[row * 6 + b] : 0.0, sm[32 + 12 + b], e);
    s_e[t] = e;
  }
  __syncthreads();
  double qterm = 0.0;
  if (phase != 0) {
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      const int t = tid + e * NT;
      if (t != 6 * 16 + 6) qterm += 0.5 * s_e[t >> 4] * s_e[t & 15] * g_old[e];
    }
  }
  const double ha = P.huber_a, hb = P.huber_b, h2a = P.huber_2a;
  const uint32_t kmask = P.kmask[ks];
  double* stage = s_stage + wave * kStageDoublesPerWave;
  d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
  double cost = 0.0;
  struct ObsD { double u, v, X0, X1, X2; };
  auto widen = [](const ObsRaw& r, ObsD& d) { d.u = (double)r.m.x; d.v = (double)r.m.y; d.X0 = (double)r.X.x; d.X1 = (double)r.X.y; d.X2 = (double)r.X.z; };
  auto pass = [&](int k, const ObsD& r) {
    const bool valid = k < n;
    const double a0 = Rca[0] * r.X0 + Rca[1] * r.X1 + Rca[2] * r.X2 + tca[0];
    const double a1 = Rca[3] * r.X0 + Rca[4] * r.X1 + Rca[5] * r.X2 + tca[1];
    const double a2 = Rca[6] * r.X0 + Rca[7] * r.X1 + Rca[8] * r.X2 + tca[2];
    if constexpr (MODEL == CC_MODEL_FISHEYE) {
      LensFishPoint q;
      lens_fish_point(kk, a0 + tcs[0], a1 + tcs[1], a2 + tcs[2], q);
      const double fx = kk[0], fy = kk[1];
      const double ru = fx * q.xd + kk[2] - r.u, rv = fy * q.yd + kk[3] - r.v;
      double rho, sr;
      lens_huber(ha, hb, h2a, ru * ru + rv * rv, rho, sr);
      if (valid) cost += 0.5 * rho;
      if (!valid) sr = 0.0;
      double w[16];
      {   // u row: B_u = fx (dxx, dxy, dxz), J_k,u = [xd 0 1 0 | fx ex w, .. w^2, .. w^3, .. w^4 | 0]
        const double b0 = fx * q.dxx, b1 = fx * q.dxy, b2 = fx * q.dxz;
        w[0] = sr * (2.0 * (b2 * a1 - b1 * a2)); w[1] = sr * (2.0 * (b0 * a2 - b2 * a0)); w[2] = sr * (2.0 * (b1 * a0 - b0 * a1));
        w[3] = sr * b0; w[4] = sr * b1; w[5] = sr * b2; w[6] = sr * ru;
        const double j1 = fx * q.ex * q.w, j2 = j1 * q.w, j3 = j2 * q.w, j4 = j3 * q.w;
        const double ju[9] = {q.xd, 0.0, 1.0, 0.0, j1, j2, j3, j4, 0.0};
#pragma unroll
        for (int i = 0; i < 9; ++i) w[7 + i] = (kmask & (1u << i)) ? 0.0 : sr * ju[i];
      }
      stage_row(stage, lane, w);
      wave_lds_fence();
      gram_rows(stage, lane, acc0, acc1);
      wave_lds_fence();
      {   // v row: B_v = fy (dxy, dyy, dyz)
        const double b0 = fy * q.dxy, b1 = fy * q.dyy, b2 = fy * q.dyz;
        w[0] = sr * (2.0 * (b2 * a1 - b1 * a2)); w[1] = sr * (2.0 * (b0 * a2 - b2 * a0)); w[2] = sr * (2.0 * (b1 * a0 - b0 * a1));
        w[3] = sr * b0; w[4] = sr * b1; w[5] = sr * b2; w[6] = sr * rv;
        const double j1 = fy * q.ey * q.w, j2 = j1 * q.w, j3 = j2 * q.w, j4 = j3 * q.w;
        const double jv[9] = {0.0, q.yd, 0.0, 1.0, j1, j2, j3, j4, 0.0};
#pragma unroll
        for (int i = 0; i < 9; ++i) w[7 + i] = (kmask & (1u << i)) ? 0.0 : sr * jv[i];
      }
      stage_row(stage, lane, w);
      wave_lds_fence();
      gram_rows(stage, lane, acc0, acc1);
      wave_lds_fence();
    } else {
      const double iz = recip_depth(a2 + tcs[2]);
      const double x = (a0 + tcs[0]) * iz, y = (a1 + tcs[1]) * iz;
      LensRadtanRows ko;
      lens_radtan_rows(kk, x, y, iz, r.u, r.v, ko);
      double rho, sr;
      lens_huber(ha, hb, h2a, ko.ru * ko.ru + ko.rv * ko.rv, rho, sr);
      if (valid) cost += 0.5 * rho;
      if (!valid) sr = 0.0;
      double w[16];
      w[0] = sr * (2.0 * (ko.Bu2 * a1 - ko.Bu1 * a2)); w[1] = sr * (2.0 * (ko.Bu0 * a2 - ko.Bu2 * a0)); w[2] = sr * (2.0 * (ko.Bu1 * a0 - ko.Bu0 * a1));
      w[3] = sr * ko.Bu0; w[4] = sr * ko.Bu1; w[5] = sr * ko.Bu2; w[6] = sr * ko.ru;
#pragma unroll
      for (int q = 0; q < 9; ++q) w[7 + q] = (kmask & (1u << q)) ? 0.0 : sr * ko.ju[q];
      stage_row(stage, lane, w);
      wave_lds_fence();
      gram_rows(stage, lane, acc0, acc1);
      wave_lds_fence();
      w[0] = sr * (2.0 * (ko.Bv2 * a1 - ko.Bv1 * a2)); w[1] = sr * (2.0 * (ko.Bv0 * a2 - ko.Bv2 * a0)); w[2] = sr * (2.0 * (ko.Bv1 * a0 - ko.Bv0 * a1));
      w[3] = sr * ko.Bv0; w[4] = sr * ko.Bv1; w[5] = sr * ko.Bv2; w[6] = sr * ko.rv;
#pragma unroll
      for (int q = 0; q < 9; ++q) w[7 + q] = (kmask & (1u << q)) ? 0.0 : sr * ko.jv[q];
      stage_row(stage, lane, w);
      wave_lds_fence();
      gram_rows(stage, lane, acc0, acc1);
      wave_lds_fence();
    }
  };
  // Observations are fetched TWO passes ahead (two register sets, the loop unrolled by two); each set is widened to doubles
  // BEFORE it is refilled, so the loaded registers are dead and the refill reuses them.
  int p = 0;
  for (; p + 1 < npass; p += 2) {
    const int k = p * NT + otid;
    ObsD d;
    widen(oa, d);
    fetch(k + 2 * NT, oa);
    pass(k, d);
    widen(ob, d);
    fetch(k + 3 * NT, ob);
    pass(k + NT, d);
  }
  if (p < npass) {
    ObsD d;
    widen(oa, d);
    pass(p * NT + otid, d);
  }
  if (NW > 1) __syncthreads();   // (every wave done with its staging tile before the partial products overwrite them)
  {
    const int slot = (lane >> 4) * 16 + (lane & 15);
    double* dstp = NW > 1 ? s_stage + wave * 256 : s_G;
#pragma unroll
    for (int r = 0; r < 4; ++r) dstp[slot + 64 * r] = acc0[r] + acc1[r];
  }
  const double qw = wave_sum(qterm), cw = wave_sum(cost);
  if (lane == 0) { s_w[wave] = qw; s_w[4 + wave] = cw; }
  __syncthreads();
  if (NW > 1) {
    s_G[tid] = (s_stage[tid] + s_stage[256 + tid]) + (s_stage[512 + tid] + s_stage[768 + tid]);
    __syncthreads();
  }
  double* out = P.gblocks + ((size_t)dst * P.NG + g) * (size_t)P.gstride;
  const int k0 = lane >> 4, j = lane & 15;
  auto role = [&](int what) {
    if (what < 2) {
      const double mv0 = s_m[k0 * 6 + (j >= 6 && j < 12 ? j - 6 : 0)];
      const double mv1 = s_m[(k0 < 2 ? k0 + 4 : 0) * 6 + (j >= 6 && j < 12 ? j - 6 : 0)];
      const double id = fixed ? 0.0 : 1.0;
      const double n0 = j < 6 ? (j == k0 ? id : 0.0) : (j < 12 ? mv0 : 0.0);                       // N[k0][j]
      const double n1 = k0 < 2 ? (j < 6 ? (j == k0 + 4 ? id : 0.0) : (j < 12 ? mv1 : 0.0))       // N[k0 + 4][j]
                               : (k0 == 2 && j == 12 ? 1.0 : 0.0);
      const int k1 = k0 < 3 ? k0 + 4 : 0;
      d4 B = {0.0, 0.0, 0.0, 0.0};
      if (what == 0) {          // AA = N^T (G7 N)
        const int gi = j < 7 ? j : 0;
        const double gv0 = s_G[gi * 16 + k0], gv1 = s_G[gi * 16 + k1];
        const double a0 = j < 7 ? gv0 : 0.0, a1 = (j < 7 && k0 < 3) ? gv1 : 0.0;
        d4 T = {0.0, 0.0, 0.0, 0.0};
        T = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, n0, T, 0, 0, 0);
        T = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, n1, T, 0, 0, 0);
        B = __builtin_amdgcn_mfma_f64_16x16x4f64(n0, T[0], B, 0, 0, 0);
        B = __builtin_amdgcn_mfma_f64_16x16x4f64(n1, T[1], B, 0, 0, 0);
      } else {                  // AB = N^T G[0:7, 7:16]
        const int hj = j < 9 ? 7 + j : 7;
        const double hv0 = s_G[k0 * 16 + hj], hv1 = s_G[k1 * 16 + hj];
        const double h0 = j < 9 ? hv0 : 0.0, h1 = (j < 9 && k0 < 3) ? hv1 : 0.0;
        B = __builtin_amdgcn_mfma_f64_16x16x4f64(n0, h0, B, 0, 0, 0);
        B = __builtin_amdgcn_mfma_f64_16x16x4f64(n1, h1, B, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = k0 + 4 * r;
        out[what * 256 + row * 16 + j] = B[r];
        if (what == 0 && phase == 0 && row < 6 && row == j) P.ghd0[g * 8 + row] = B[r];   // diag of H_cc
      }
    } else if (what == 2) {     // BB = G[7:16, 7:16]
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = k0 + 4 * r;
        const bool in = row < 9 && j < 9;
        const double gv = s_G[(in ? 7 + row : 0) * 16 + (in ? 7 + j : 0)];
        const double val = in ? gv : 0.0;
        out[512 + row * 16 + j] = val;
        if (phase == 0 && row < 9 && row == j) P.ghdk[g * 16 + row] = val;   // diag of H_kk
      }
    } else {
      if (lane == 0) {
        P.gstats[g * 2] = NW > 1 ? (s_w[4] + s_w[5]) + (s_w[6] + s_w[7]) : s_w[4];
        P.gstats[g * 2 + 1] = NW > 1 ? (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]) : s_w[0];
      }
      if (lane < 36) P.gcomp[((size_t)dst * P.NG + g) * kRigLensCompK + 256 + lane] = s_m[lane];
    }
  };
  if (NW > 1) {
    role(wave);
  } else {
    role(0); role(1); role(2); role(3);
  }
#pragma unroll
  for (int e = 0; e < EPT; ++e) P.gcomp[((size_t)dst * P.NG + g) * kRigLensCompK + tid + e * NT] = s_G[tid + e * NT];
}

// per-observation robustified cost at the accepted point: k_rig_obs_cost (cc_rig.hip) with the residual of the model of the
// group's camera -- the poses from their quaternions, the camera-frame point by the two-step chain; the fisheye residual without
// a division by the depth, the radial-tangential one on it, as k_rig_obs_cost forms it. cmodel == nullptr at compile time
// (PER_CAMERA = false): every camera is fisheye
template <bool PER_CAMERA>
__device__ __forceinline__ void rig_lens_obs_cost(const RigLensDev& P, const int32_t* __restrict__ cmodel, int cur, double* out) {
  const int64_t g = blockIdx.x;
  const int f = P.gframe[g], c = P.gcam[g];
  const bool fish = PER_CAMERA ? cmodel[c] == CC_MODEL_FISHEYE : true;
  const double* pc = P.cam + ((size_t)cur * P.C + c) * 8;
  const double* pf = P.pose + ((size_t)cur * P.F + f) * 8;
  double Rc[9], Rf[9];
  quat_to_R(pc, Rc);
  quat_to_R(pf, Rf);
  const float2* uv2 = reinterpret_cast<const float2*>(P.uv);
  const double* kk = P.intr + ((size_t)cur * P.CK + P.kset[c]) * 16;
  for (int64_t idx = P.goff[g] + threadIdx.x; idx < P.goff[g + 1]; idx += blockDim.x) {
    const float2 m = uv2[idx];
    const int64_t w = P.widx[idx];
    const double X0 = (double)P.wxyz[w * 3], X1 = (double)P.wxyz[w * 3 + 1], X2 = (double)P.wxyz[w * 3 + 2];
    const double r0 = Rf[0] * X0 + Rf[1] * X1 + Rf[2] * X2 + pf[4];
    const double r1 = Rf[3] * X0 + Rf[4] * X1 + Rf[5] * X2 + pf[5];
    const double r2 = Rf[6] * X0 + Rf[7] * X1 + Rf[8] * X2 + pf[6];
    const double xc = Rc[0] * r0 + Rc[1] * r1 + Rc[2] * r2 + pc[4];
    const double yc = Rc[3] * r0 + Rc[4] * r1 + Rc[5] * r2 + pc[5];
    const double zc = Rc[6] * r0 + Rc[7] * r1 + Rc[8] * r2 + pc[6];
    double ru, rv;
    if (fish) {
      LensFishPoint q;
      lens_fish_point(kk, xc, yc, zc, q);
      ru = kk[0] * q.xd + kk[2] - (double)m.x;
      rv = kk[1] * q.yd + kk[3] - (double)m.y;
    } else {
      const double iz = 1.0 / zc;
      LensRadtanRows ko;
      lens_radtan_rows(kk, xc * iz, yc * iz, iz, (double)m.x, (double)m.y, ko);
      ru = ko.ru;
      rv = ko.rv;
    }
    double rho, sr;
    lens_huber(P.huber_a, P.huber_b, P.huber_2a, ru * ru + rv * rv, rho, sr);
    out[idx] = 0.5 * rho;
  }
}
__global__ void k_rig_obs_cost_fisheye(RigLensDev P, int cur, double* out /*sorted order*/) { rig_lens_obs_cost<false>(P, nullptr, cur, out); }
__global__ void k_rig_obs_cost_mixed(RigLensDev P, const int32_t* __restrict__ cmodel, int cur, double* out /*sorted order*/) {
  rig_lens_obs_cost<true>(P, cmodel, cur, out);
}

void rig_lens_enqueue_sweep(const RigLensDev& P, hipStream_t s, int waves, int model, const int32_t* glist, int n) {
  if (n <= 0) return;
  const dim3 grid((unsigned)n), block(waves == 1 ? 64 : 256);
  if (!glist) {
    if (waves == 1) hipLaunchKernelGGL((k_rig_sweep_lens<1, CC_MODEL_FISHEYE, false>), grid, block, 0, s, P, nullptr);
    else hipLaunchKernelGGL((k_rig_sweep_lens<4, CC_MODEL_FISHEYE, false>), grid, block, 0, s, P, nullptr);
  } else if (model == CC_MODEL_FISHEYE) {
    if (waves == 1) hipLaunchKernelGGL((k_rig_sweep_lens<1, CC_MODEL_FISHEYE, true>), grid, block, 0, s, P, glist);
    else hipLaunchKernelGGL((k_rig_sweep_lens<4, CC_MODEL_FISHEYE, true>), grid, block, 0, s, P, glist);
  } else {
    if (waves == 1) hipLaunchKernelGGL((k_rig_sweep_lens<1, CC_MODEL_RADTAN, true>), grid, block, 0, s, P, glist);
    else hipLaunchKernelGGL((k_rig_sweep_lens<4, CC_MODEL_RADTAN, true>), grid, block, 0, s, P, glist);
  }
}

void rig_lens_enqueue_obs_cost(const RigLensDev& P, hipStream_t s, const int32_t* cmodel, int cur, double* out) {
  if (P.NG <= 0) return;
  if (cmodel) hipLaunchKernelGGL(k_rig_obs_cost_mixed, dim3((unsigned)P.NG), dim3(256), 0, s, P, cmodel, cur, out);
  else hipLaunchKernelGGL(k_rig_obs_cost_fisheye, dim3((unsigned)P.NG), dim3(256), 0, s, P, cur, out);
}

}  // namespace cc
