// cc_rig_mixed.hip -- kernels of a rig handle whose cameras differ in their pixel model (declarations and the outline:
// cc_rig_mixed.hpp). A translation unit of its own: the kernel sets of cc_rig.hip, cc_rig_fisheye.hip and cc_rigk_start.hip are
// pinned (tests/test_kernel_budgets.py, tests/test_rigk_fisheye_budgets.py), so their device functions are RESTATED here, as
// cc_rig_fisheye.hip restated its own.
#include "cc_common.hpp"
#include "cc_device.hpp"
#include "cc_rig_dev.hpp"
#include "cc_rig_mixed.hpp"

namespace cc {

// waves per SIMD: each instantiation keeps the budget of the homogeneous kernel it restates -- three for the radial-tangential
// rows (k_rig_sweep_adjk, <= 168 registers), two for the fisheye rows (k_rig_sweep_adjk_fisheye). One kernel with a uniform
// branch would put the radial-tangential groups at two waves and carry the arctangent's live values through their pass loop.
constexpr int kRigMixWavesRadtan = 3;
constexpr int kRigMixWavesFisheye = 2;
constexpr int kRigMixCompK = 320;  // doubles per group and buffer of the compact record: G (256), M (36) (kRigCompK, cc_rig_sweeps.hpp)

// ceres::HuberLoss + Corrector: rig_fish_huber (cc_rig_fisheye.hip), which is huber / huber_outlier of cc_rig.hip line for line
// (b = a^2 and a2 = 2 a from the caller: the same bits as the products formed there)
__device__ __forceinline__ void rig_mix_huber(double a, double b, double a2, double s, double& rho, double& sr) {
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

// ---- radial-tangential rows: rigk_obs (cc_rig.hip) on the normalised point (x, y, 1 / z), slots fx fy px py k1 k2 p1 p2 k3 ----
struct RigMixRadtan {
  double ru, rv, Bu0, Bu1, Bu2, Bv0, Bv1, Bv2;
  double ju[9], jv[9];
};
__device__ __forceinline__ void rig_mix_radtan(const double* k, double x, double y, double iz, double u, double v, RigMixRadtan& r) {
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

// ---- fisheye rows: rig_fish_point (cc_rig_fisheye.hip) on the camera-frame point itself, slots fx fy px py k1 k2 k3 k4 - ----
struct RigMixFish {
  double ex, ey, w, xd, yd, dxx, dxy, dyy, dxz, dyz;
};
__device__ __forceinline__ void rig_mix_fish(const double* k, double xc, double yc, double zc, RigMixFish& c) {
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

// ---------------------------------------------------------------------------------------------
// k_rig_sweep_adjk_fisheye (cc_rig_fisheye.hip) over the groups of ONE model's cameras: workgroup b sweeps group
// g = glist[b], and everything indexed by the group -- the wave rotation, the compact record, the tiles, the statistics, the
// diagonals -- uses g. MODEL picks the rows: the fisheye ones as there, or rigk_obs' on the normalised point as
// k_rig_sweep_adjk forms them. Pose chain, order of the sums, model-cost term, M, e', tiles and record are the same text.
// ---------------------------------------------------------------------------------------------
template <int NW, int MODEL>
__global__ __launch_bounds__(NW * 64, MODEL == CC_MODEL_FISHEYE ? kRigMixWavesFisheye : kRigMixWavesRadtan)
void k_rig_sweep_adjk_sel(RigFishDev P, const int32_t* __restrict__ glist) {
  constexpr int NT = NW * 64, EPT = 256 / NT;
  __shared__ __attribute__((aligned(16))) double s_stage[NW * kStageDoublesPerWave];   // per wave 64 x 16; then the partial products
  __shared__ double sm[96];        // camera record, frame record, intrinsics record (candidate [0..8], step [16..24])
  __shared__ double s_G[256];      // G
  __shared__ double s_mold[36];    // M of the accepted point
  __shared__ double s_e[16];       // e'
  __shared__ double s_m[36];       // M
  __shared__ double s_w[8];        // per wave: model-cost term, cost
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t g = glist[blockIdx.x];
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
  const double* comp_old = P.gcomp + ((size_t)cur * P.NG + g) * kRigMixCompK;
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
      RigMixFish q;
      rig_mix_fish(kk, a0 + tcs[0], a1 + tcs[1], a2 + tcs[2], q);
      const double fx = kk[0], fy = kk[1];
      const double ru = fx * q.xd + kk[2] - r.u, rv = fy * q.yd + kk[3] - r.v;
      double rho, sr;
      rig_mix_huber(ha, hb, h2a, ru * ru + rv * rv, rho, sr);
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
      RigMixRadtan ko;
      rig_mix_radtan(kk, x, y, iz, r.u, r.v, ko);
      double rho, sr;
      rig_mix_huber(ha, hb, h2a, ko.ru * ko.ru + ko.rv * ko.rv, rho, sr);
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
      if (lane < 36) P.gcomp[((size_t)dst * P.NG + g) * kRigMixCompK + 256 + lane] = s_m[lane];
    }
  };
  if (NW > 1) {
    role(wave);
  } else {
    role(0); role(1); role(2); role(3);
  }
#pragma unroll
  for (int e = 0; e < EPT; ++e) P.gcomp[((size_t)dst * P.NG + g) * kRigMixCompK + tid + e * NT] = s_G[tid + e * NT];
}

// per-observation robustified cost at the accepted point: k_rig_obs_cost_fisheye (cc_rig_fisheye.hip) with the residual of the
// group's camera model -- the camera-frame point by the two-step chain; the radial-tangential residual on its division by the
// depth, as k_rig_obs_cost (cc_rig.hip) forms it
__global__ void k_rig_obs_cost_mixed(RigFishDev P, const int32_t* __restrict__ cmodel, int cur, double* out /*sorted order*/) {
  const int64_t g = blockIdx.x;
  const int f = P.gframe[g], c = P.gcam[g];
  const bool fish = cmodel[c] == CC_MODEL_FISHEYE;
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
      RigMixFish q;
      rig_mix_fish(kk, xc, yc, zc, q);
      ru = kk[0] * q.xd + kk[2] - (double)m.x;
      rv = kk[1] * q.yd + kk[3] - (double)m.y;
    } else {
      const double iz = 1.0 / zc;
      RigMixRadtan ko;
      rig_mix_radtan(kk, xc * iz, yc * iz, iz, (double)m.x, (double)m.y, ko);
      ru = ko.ru;
      rv = ko.rv;
    }
    double rho, sr;
    rig_mix_huber(P.huber_a, P.huber_b, P.huber_2a, ru * ru + rv * rv, rho, sr);
    out[idx] = 0.5 * rho;
  }
}

// ---- the pixel start: the inverse maps of cc_rigk_start_dev.hpp, restated (that header DEFINES k_rigk_start_unproject: including
// it would put a second copy of the kernel into this object) --------------------------------------------------------------------
__device__ __forceinline__ void rig_mix_radtan_eval(double k1, double k2, double p1, double p2, double k3, double x, double y,
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

constexpr int kRigMixRadtanSteps = 100;      // (kRigkRadtanSteps)
constexpr double kRigMixRootLevel = 256.0;   // (kRigkRootLevel)

__device__ __forceinline__ bool rig_mix_radtan_root(const double* __restrict__ k, double xd, double yd, double* ox, double* oy) {
  const double k1 = k[4], k2 = k[5], p1 = k[6], p2 = k[7], k3 = k[8];
  double x = xd, y = yd, radius = 1e4, dec = 2.0;
  double r[2], J[4];
  rig_mix_radtan_eval(k1, k2, p1, p2, k3, x, y, xd, yd, r, J, nullptr);
  double cost = 0.5 * (r[0] * r[0] + r[1] * r[1]);
  for (int it = 0; it < kRigMixRadtanSteps && cost > 0.0; ++it) {
    const double h00 = J[0] * J[0] + J[2] * J[2], h01 = J[0] * J[1] + J[2] * J[3];
    const double h11 = J[1] * J[1] + J[3] * J[3];
    const double g0 = J[0] * r[0] + J[2] * r[1], g1 = J[1] * r[0] + J[3] * r[1];
    const double a00 = h00 + fmax(h00, 1e-6) / radius, a11 = h11 + fmax(h11, 1e-6) / radius;
    const double det = a00 * a11 - h01 * h01;
    const double dx = -(a11 * g0 - h01 * g1) / det, dy = -(a00 * g1 - h01 * g0) / det;
    if (!(fabs(dx) + fabs(dy) > 1e-17 * (fabs(x) + fabs(y) + 1e-300))) break;
    double rn[2], Jn[4];
    rig_mix_radtan_eval(k1, k2, p1, p2, k3, x + dx, y + dy, xd, yd, rn, Jn, nullptr);
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
  rig_mix_radtan_eval(k1, k2, p1, p2, k3, x, y, xd, yd, r, J, &scale);
  *ox = x; *oy = y;
  return fmax(fabs(r[0]), fabs(r[1])) <= kRigMixRootLevel * 1.1102230246251565e-16 * scale;   // (false for a NaN residual)
}

__device__ __forceinline__ double rig_mix_fisheye_theta_d(const double* __restrict__ k, double th) {
  const double w = th * th;
  return th * (1.0 + w * (k[4] + w * (k[5] + w * (k[6] + w * k[7]))));
}
__device__ __forceinline__ double rig_mix_fisheye_slope(const double* __restrict__ k, double th) {
  const double w = th * th;
  return 1.0 + w * (3.0 * k[4] + w * (5.0 * k[5] + w * (7.0 * k[6] + w * (9.0 * k[7]))));
}
__device__ __forceinline__ bool rig_mix_fisheye_root(const double* __restrict__ k, double td, double* theta) {
  const double top = 1.5707963267948966;   // the double below pi/2
  const bool bracketed = rig_mix_fisheye_theta_d(k, top) - td > 0.0;
  double lo = 0.0, hi = top;
  double th = td < top ? td : 0.5 * top;
  bool found = false;
  for (int it = 0; it < 200; ++it) {
    const double f = rig_mix_fisheye_theta_d(k, th) - td;
    const double fp = rig_mix_fisheye_slope(k, th);
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

// k_rigk_start_unproject (cc_rigk_start_dev.hpp) with the model of the view's camera: one wave per view, the model and the
// intrinsics set the same for every lane
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
        else if (td > 0.0 && rig_mix_fisheye_root(k, td, &th)) {
          const double s = tan(th) / td;
          o = make_float2((float)(xd * s), (float)(yd * s));
        }
      } else {
        double x, y;
        if (rig_mix_radtan_root(k, xd, yd, &x, &y)) o = make_float2((float)x, (float)y);
      }
    }
    if (isnan(o.x) || isnan(o.y)) o = make_float2(nanf_, nanf_);   // (a non-finite coefficient: both coordinates or none)
    out2[i] = o;
  }
}

// The launch for one model's list of groups; the host calls it once per model, one after the other on `s` (a chain in a captured
// graph). An empty list launches nothing: a grid of zero workgroups is a launch error.
void rig_mixed_enqueue_sweep(const RigMixedDev& P, hipStream_t s, int waves, int model) {
  const int n = P.nlist[model];
  if (n <= 0) return;
  const int32_t* gl = P.glist[model];
  if (model == CC_MODEL_FISHEYE) {
    if (waves == 1) hipLaunchKernelGGL((k_rig_sweep_adjk_sel<1, CC_MODEL_FISHEYE>), dim3((unsigned)n), dim3(64), 0, s, P.base, gl);
    else hipLaunchKernelGGL((k_rig_sweep_adjk_sel<4, CC_MODEL_FISHEYE>), dim3((unsigned)n), dim3(256), 0, s, P.base, gl);
  } else {
    if (waves == 1) hipLaunchKernelGGL((k_rig_sweep_adjk_sel<1, CC_MODEL_RADTAN>), dim3((unsigned)n), dim3(64), 0, s, P.base, gl);
    else hipLaunchKernelGGL((k_rig_sweep_adjk_sel<4, CC_MODEL_RADTAN>), dim3((unsigned)n), dim3(256), 0, s, P.base, gl);
  }
}

void rig_mixed_enqueue_obs_cost(const RigMixedDev& P, hipStream_t s, int cur, double* out) {
  if (P.base.NG > 0) hipLaunchKernelGGL(k_rig_obs_cost_mixed, dim3((unsigned)P.base.NG), dim3(256), 0, s, P.base, P.cmodel, cur, out);
}

void rigk_start_enqueue_unproject_cam(const RigkStartCamDev& P, hipStream_t s) {
  if (P.NG > 0) hipLaunchKernelGGL(k_rigk_start_unproject_cam, dim3((unsigned)P.NG), dim3(64), 0, s, P);
}

}  // namespace cc
