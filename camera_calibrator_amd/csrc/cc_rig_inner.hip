// cc_rig_inner.hip -- kernels of Ceres' inner iterations on the rig problem (declarations and the outline: cc_rig_inner.hpp).
// A translation unit of its own next to cc_rig.hip, whose kernel set is pinned (tests/test_kernel_budgets.py).
#include "cc_common.hpp"
#include "cc_device.hpp"
#include "cc_rig_inner.hpp"

namespace cc {

// ReprojectionErrorExtrinsics::operator() and ceres::HuberLoss + Corrector: the arithmetic of rig_common / huber_outlier /
// huber in cc_rig.hip, line for line (residual in normalised coordinates; residual and Jacobian scaled by sqrt(rho'))
struct RigInnerObs {
  double b0, b1, b2, a0, a1, a2, x, y, iz, ru, rv;
};
__device__ __forceinline__ void rig_inner_common(const double* Rf, const double* tf, const double* Rc, const double* tc,
                                                 double X0, double X1, double X2, double u, double v, RigInnerObs& o) {
  o.b0 = Rf[0] * X0 + Rf[1] * X1 + Rf[2] * X2;
  o.b1 = Rf[3] * X0 + Rf[4] * X1 + Rf[5] * X2;
  o.b2 = Rf[6] * X0 + Rf[7] * X1 + Rf[8] * X2;
  const double r0 = o.b0 + tf[0], r1 = o.b1 + tf[1], r2 = o.b2 + tf[2];
  o.a0 = Rc[0] * r0 + Rc[1] * r1 + Rc[2] * r2;
  o.a1 = Rc[3] * r0 + Rc[4] * r1 + Rc[5] * r2;
  o.a2 = Rc[6] * r0 + Rc[7] * r1 + Rc[8] * r2;
  const double xc = o.a0 + tc[0], yc = o.a1 + tc[1], zc = o.a2 + tc[2];
  o.iz = 1.0 / zc;
  o.x = xc * o.iz;
  o.y = yc * o.iz;
  o.ru = o.x - u;
  o.rv = o.y - v;
}
__device__ __forceinline__ void rig_inner_huber(double a, double s, double& rho, double& sr) {
  const double b = a * a;
  if (s > b) {
    const double y = rsqrt_pos(s);
    const double r = s * y;
    const double q = fmax(2.2250738585072014e-308, a * y);
    sr = q * rsqrt_pos(q);
    rho = 2.0 * a * r - b;
  } else {
    rho = s;
    sr = 1.0;
  }
}

// deterministic sum of one value per thread over a workgroup of 256 (every thread after return)
__device__ __forceinline__ double rig_inner_sum256(double v, double* s4) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}
// cost and model term of the last sweep, summed over its rows (one per frame in the frame form, else one per group) -> out[0..1]
__device__ __forceinline__ void rig_inner_stats(const RigInnerDev& P, double* s4, double* out) {
  const int64_t nrows = P.fmode ? P.F : P.NG;
  double c = 0.0, m = 0.0;
  for (int64_t i = threadIdx.x; i < nrows; i += 256) { c += P.gstats[2 * i]; m += P.gstats[2 * i + 1]; }
  c = rig_inner_sum256(c, s4);
  __syncthreads();
  m = rig_inner_sum256(m, s4);
  if (threadIdx.x == 0) { out[0] = c; out[1] = m; }
  __syncthreads();
}

// Ceres' default Solver::Options as the mini-solves use them
__device__ inline LmOpts rig_inner_opts() {
  LmOpts o;
  o.max_iterations = 50; o.use_nonmonotonic_steps = 0; o.max_consecutive_nonmonotonic_steps = 5; o.jacobi_scaling = 1;
  o.max_consecutive_invalid_steps = 5; o.pad0_ = 0;
  o.function_tolerance = 1e-6; o.gradient_tolerance = 1e-10; o.parameter_tolerance = 1e-8;
  o.initial_radius = 1e4; o.max_radius = 1e16; o.min_radius = 1e-32; o.min_relative_decrease = 1e-3;
  o.min_lm_diagonal = 1e-6; o.max_lm_diagonal = 1e32;
  return o;
}

// Cost, tangent gradient (3) and Gram (6: 00 01 02 11 12 22) of block `blk` of group KIND (0 t_cr, 1 q_cr, 2 t_rw, 3 q_rw) at
// the block value xb (LDS), the other blocks taken from buffer `buf`. This thread's share; the caller reduces.
template <int KIND, int NT>
__device__ inline void rig_inner_eval(const RigInnerDev& P, int buf, int blk, const double* xb, double* a) {
#pragma unroll
  for (int k = 0; k < 10; ++k) a[k] = 0.0;
  const float2* uv2 = reinterpret_cast<const float2*>(P.uv);
  double Ro[9], to[3];   // the block's own pose
  {
    const double* own = KIND < 2 ? P.cam + ((size_t)buf * P.C + blk) * 8 : P.pose + ((size_t)buf * P.F + blk) * 8;
    double q[4];
    const bool rot = KIND == 1 || KIND == 3;
    for (int i = 0; i < 4; ++i) q[i] = rot ? xb[i] : own[i];
    for (int i = 0; i < 3; ++i) to[i] = rot ? own[4 + i] : xb[i];
    quat_to_R(q, Ro);
  }
  const int64_t g0 = KIND < 2 ? (int64_t)P.cam_goff[blk] : P.fgoff[blk];
  const int64_t g1 = KIND < 2 ? (int64_t)P.cam_goff[blk + 1] : P.fgoff[blk + 1];
  for (int64_t gi = g0; gi < g1; ++gi) {
    const int64_t g = KIND < 2 ? (int64_t)P.cam_glist[gi] : gi;
    const double* oth = KIND < 2 ? P.pose + ((size_t)buf * P.F + P.gframe[g]) * 8 : P.cam + ((size_t)buf * P.C + P.gcam[g]) * 8;
    double Rt[9], tt[3];
    quat_to_R(oth, Rt);
    for (int i = 0; i < 3; ++i) tt[i] = oth[4 + i];
    const double* Rc = KIND < 2 ? Ro : Rt;
    const double* tc = KIND < 2 ? to : tt;
    const double* Rf = KIND < 2 ? Rt : Ro;
    const double* tf = KIND < 2 ? tt : to;
    for (int64_t idx = P.goff[g] + threadIdx.x; idx < P.goff[g + 1]; idx += NT) {
      const float2 m = uv2[idx];
      RigInnerObs o;
      rig_inner_common(Rf, tf, Rc, tc, (double)P.oxyz[idx * 3], (double)P.oxyz[idx * 3 + 1], (double)P.oxyz[idx * 3 + 2],
                 (double)m.x, (double)m.y, o);
      double rho, sr;
      rig_inner_huber(P.huber_a, o.ru * o.ru + o.rv * o.rv, rho, sr);
      a[0] += 0.5 * rho;
      // rows of d residual / d x_cam, Huber-scaled (k_rig_sweep_frame: pz, qu, qv)
      const double pz = sr * o.iz, qu = -(pz * o.x), qv = -(pz * o.y);
      double ju[3], jv[3];
      if (KIND == 0) { ju[0] = pz; ju[1] = 0.0; ju[2] = qu; jv[0] = 0.0; jv[1] = pz; jv[2] = qv; }
      else {
        double eu[3], ev[3], b[3];   // rows through the rotation that maps the block's tangent into x_cam, and the rotated point
        if (KIND == 1) {
          eu[0] = pz; eu[1] = 0.0; eu[2] = qu; ev[0] = 0.0; ev[1] = pz; ev[2] = qv;
          b[0] = o.a0; b[1] = o.a1; b[2] = o.a2;
        } else {
          for (int k = 0; k < 3; ++k) { eu[k] = pz * Rc[k] + qu * Rc[6 + k]; ev[k] = pz * Rc[3 + k] + qv * Rc[6 + k]; }
          b[0] = o.b0; b[1] = o.b1; b[2] = o.b2;
        }
        if (KIND == 2) { for (int k = 0; k < 3; ++k) { ju[k] = eu[k]; jv[k] = ev[k]; } }
        else {   // QuaternionManifold tangent: d (R p) / d delta = -2 [R p]x
          ju[0] = 2.0 * (eu[2] * b[1] - eu[1] * b[2]); ju[1] = 2.0 * (eu[0] * b[2] - eu[2] * b[0]); ju[2] = 2.0 * (eu[1] * b[0] - eu[0] * b[1]);
          jv[0] = 2.0 * (ev[2] * b[1] - ev[1] * b[2]); jv[1] = 2.0 * (ev[0] * b[2] - ev[2] * b[0]); jv[2] = 2.0 * (ev[1] * b[0] - ev[0] * b[1]);
        }
      }
      const double su = sr * o.ru, sv = sr * o.rv;
      for (int k = 0; k < 3; ++k) a[1 + k] += ju[k] * su + jv[k] * sv;
      a[4] += ju[0] * ju[0] + jv[0] * jv[0]; a[5] += ju[0] * ju[1] + jv[0] * jv[1]; a[6] += ju[0] * ju[2] + jv[0] * jv[2];
      a[7] += ju[1] * ju[1] + jv[1] * jv[1]; a[8] += ju[1] * ju[2] + jv[1] * jv[2]; a[9] += ju[2] * ju[2] + jv[2] * jv[2];
    }
  }
}

// fixed-order workgroup sum of the ten values -> out[10] (LDS, every thread after return)
template <int NT>
__device__ inline void rig_inner_reduce(double* a, double* s_w, double* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 10; ++k) a[k] = wave_sum(a[k]);
  if (lane == 0)
    for (int k = 0; k < 10; ++k) s_w[wave * 10 + k] = a[k];
  __syncthreads();
  if (threadIdx.x < 10) {
    double s = 0.0;
    for (int w = 0; w < NT / 64; ++w) s += s_w[w * 10 + threadIdx.x];
    out[threadIdx.x] = s;
  }
  __syncthreads();
}

// Ceres' gradient_max_norm of the block: || x - Plus(x, -g) ||_inf (pose_grad_proj_max's rule for the quaternion)
template <int KIND>
__device__ inline double rig_inner_gmax(const double* x, const double* g) {
  if (KIND == 1 || KIND == 3) { const double g6[6] = {g[0], g[1], g[2], 0.0, 0.0, 0.0}; return pose_grad_proj_max(x, g6); }
  return fmax(fmax(fabs(g[0]), fabs(g[1])), fabs(g[2]));
}

// One block's mini-solve per workgroup. buf >= 0: on that buffer, unconditionally (cc_rig_inner_pass); buf < 0: on the
// candidate buffers of a solve (ctl->cur ^ 1), when k_rig_inner_begin said so.
template <int KIND, int NT>
__global__ __launch_bounds__(NT) void k_rig_inner_block(RigInnerDev P, int buf) {
  __shared__ double s_w[(NT / 64) * 10];
  __shared__ double s_tot[10];
  __shared__ double s_x[4];
  __shared__ int s_go;
  const int blk = blockIdx.x, tid = threadIdx.x;
  constexpr bool ROT = KIND == 1 || KIND == 3;
  constexpr int NA = ROT ? 4 : 3;
  int32_t* it_out = P.iters + (KIND == 0 ? 0 : KIND == 1 ? P.C : KIND == 2 ? 2 * P.C : 2 * P.C + P.F) + blk;
  if (buf < 0) {
    if (P.st[RIG_IN_RUN] == 0.0) return;
    buf = P.ctl->cur ^ 1;
  }
  const bool live = KIND < 2 ? P.pcol[blk] >= 0 : P.fgoff[blk + 1] > P.fgoff[blk];   // (constant / unobserved: not a block)
  if (!live) { if (tid == 0) *it_out = 0; return; }
  double* xg = (KIND < 2 ? P.cam + ((size_t)buf * P.C + blk) * 8 : P.pose + ((size_t)buf * P.F + blk) * 8) + (ROT ? 0 : 4);
  if (tid < NA) s_x[tid] = xg[tid];
  __syncthreads();
  double a[10];
  rig_inner_eval<KIND, NT>(P, buf, blk, s_x, a);
  rig_inner_reduce<NT>(a, s_w, s_tot);
  // thread 0's state of the mini-solve
  const LmOpts o = rig_inner_opts();
  LmCtl st{};
  double x[4] = {0, 0, 0, 0}, xc[4] = {0, 0, 0, 0}, g[3], A[6], sc[3], qm = 0.0;
  if (tid == 0) {
    for (int i = 0; i < NA; ++i) x[i] = s_x[i];
    for (int k = 0; k < 3; ++k) g[k] = s_tot[1 + k];
    for (int k = 0; k < 6; ++k) A[k] = s_tot[4 + k];
    const double xn = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3]);
    lm_init(st, o, s_tot[0], xn);
    sc[0] = 1.0 / (1.0 + sqrt(A[0])); sc[1] = 1.0 / (1.0 + sqrt(A[3])); sc[2] = 1.0 / (1.0 + sqrt(A[5]));
    st.gmax = rig_inner_gmax<KIND>(x, g);
    if (st.gmax <= o.gradient_tolerance) { st.done = 1; st.term = CC_CONVERGENCE_GRADIENT; }
    s_go = st.done ? 0 : 1;
  }
  __syncthreads();
  for (;;) {
    if (s_go == 0) break;
    __syncthreads();   // (every thread has read s_go before thread 0 writes it again)
    if (tid == 0) {
      // LevenbergMarquardtStrategy::ComputeStep on the Jacobi-scaled block: (A_s + diag(clamp(diag A_s) / radius)) dy = -g_s
      const int ii[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
      double M[3][3], gs[3];
      for (int i = 0; i < 3; ++i) {
        gs[i] = g[i] * sc[i];
        for (int j = 0; j < 3; ++j) M[i][j] = A[ii[i][j]] * sc[i] * sc[j];
      }
      double As[3][3];
      for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) As[i][j] = M[i][j];
      for (int i = 0; i < 3; ++i) M[i][i] += clampd(As[i][i], o.min_lm_diagonal, o.max_lm_diagonal) / st.radius;
      // Cholesky + substitutions
      double L[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
      bool ok = true;
      for (int j = 0; j < 3 && ok; ++j) {
        double d = M[j][j];
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(d > 0.0) || !isfinite(d)) { ok = false; break; }
        L[j][j] = sqrt(d);
        for (int i = j + 1; i < 3; ++i) {
          double s = M[i][j];
          for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
          L[i][j] = s / L[j][j];
        }
      }
      double dy[3] = {0, 0, 0};
      if (ok) {
        double z[3];
        for (int i = 0; i < 3; ++i) { double s = -gs[i]; for (int k = 0; k < i; ++k) s -= L[i][k] * z[k]; z[i] = s / L[i][i]; }
        for (int i = 2; i >= 0; --i) { double s = z[i]; for (int k = i + 1; k < 3; ++k) s -= L[k][i] * dy[k]; dy[i] = s / L[i][i]; }
        ok = isfinite(dy[0]) && isfinite(dy[1]) && isfinite(dy[2]);
      }
      // model cost term: g_s . dy + 1/2 dy' A_s dy (Ceres: -model_residuals . (residuals + model_residuals / 2))
      qm = 0.0;
      for (int i = 0; i < 3; ++i) {
        double Ad = 0.0;
        for (int j = 0; j < 3; ++j) Ad += As[i][j] * dy[j];
        qm += dy[i] * (gs[i] + 0.5 * Ad);
      }
      const double delta[3] = {dy[0] * sc[0], dy[1] * sc[1], dy[2] * sc[2]};
      if (ROT) quat_plus(x, delta, xc);
      else for (int i = 0; i < 3; ++i) xc[i] = x[i] + delta[i];
      st.step_valid = ok ? 1 : 0;
      for (int i = 0; i < NA; ++i) s_x[i] = xc[i];
      s_go = (ok && -qm > 0.0 && isfinite(qm)) ? 1 : 2;   // 2: invalid step, no evaluation
    }
    __syncthreads();
    const bool eval = s_go == 1;
    if (eval) {
      rig_inner_eval<KIND, NT>(P, buf, blk, s_x, a);
      rig_inner_reduce<NT>(a, s_w, s_tot);
    }
    __syncthreads();
    if (tid == 0) {
      double step2 = 0.0, xn2 = 0.0;
      for (int i = 0; i < NA; ++i) { const double d = xc[i] - x[i]; step2 += d * d; xn2 += xc[i] * xc[i]; }
      const int succ0 = st.n_success;
      lm_decide(st, o, nullptr, eval ? s_tot[0] : st.x_cost, qm, step2, xn2);
      if (st.n_success != succ0) {   // accepted: the candidate is the new point, its gradient / Gram come from this evaluation
        for (int i = 0; i < NA; ++i) x[i] = xc[i];
        for (int k = 0; k < 3; ++k) g[k] = s_tot[1 + k];
        for (int k = 0; k < 6; ++k) A[k] = s_tot[4 + k];
        if (!st.done) lm_finalize(st, o, rig_inner_gmax<KIND>(x, g));
      } else if (!st.done && st.radius < o.min_radius) { st.done = 1; st.term = CC_MIN_RADIUS; }
      s_go = st.done ? 0 : 1;
    }
    __syncthreads();
  }
  if (tid == 0) {
    for (int i = 0; i < NA; ++i) xg[i] = x[i];
    *it_out = st.iter;
  }
}

// head of the outer-loop hook: does a pass run this round? (a candidate of a valid step, with a finite cost, while enabled)
__global__ __launch_bounds__(256) void k_rig_inner_begin(RigInnerDev P) {
  __shared__ double s4[4];
  __shared__ double s_tot[2];
  const LmCtl* ctl = P.ctl;
  const bool pending = !ctl->done && ctl->phase != 0 && ctl->cand_pending && ctl->step_valid;
  if (!pending || P.st[RIG_IN_ENABLED] == 0.0) {
    if (threadIdx.x == 0) P.st[RIG_IN_RUN] = 0.0;
    return;
  }
  rig_inner_stats(P, s4, s_tot);
  if (threadIdx.x == 0) {
    const double mcc = -s_tot[1];
    const bool run = mcc > 0.0 && isfinite(mcc) && s_tot[0] < 1.7976931348623157e308;
    P.st[RIG_IN_RUN] = run ? 1.0 : 0.0;
    P.st[RIG_IN_CAND] = s_tot[0];
    P.st[RIG_IN_QMODEL] = s_tot[1];
  }
}

// records of the candidate the pass moved (rotation, translation; the step the model term reads stays)
__global__ __launch_bounds__(256) void k_rig_inner_records(RigInnerDev P) {
  if (P.st[RIG_IN_RUN] == 0.0) return;
  const int dst = P.ctl->cur ^ 1;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)P.C + P.F) return;
  const bool cam = i < P.C;
  const double* x = cam ? P.cam + ((size_t)dst * P.C + i) * 8 : P.pose + ((size_t)dst * P.F + (i - P.C)) * 8;
  double* rec = cam ? P.camrec + (size_t)i * 32 : P.frec + (size_t)(i - P.C) * 32;
  double R[9];
  quat_to_R(x, R);
  for (int k = 0; k < 9; ++k) rec[k] = R[k];
  for (int k = 0; k < 3; ++k) rec[9 + k] = x[4 + k];
}

// the decision with the inner pass (TrustRegionMinimizer::DoInnerIterationsIfNeeded, IsStepSuccessful): candidate cost from
// the second sweep, model term + the pass's reduction, step norm |x - candidate| and |candidate| in the ambient coordinates
__global__ __launch_bounds__(256) void k_rig_inner_decide(RigInnerDev P) {
  __shared__ double s_tot[2];
  __shared__ double s4[4];
  if (P.st[RIG_IN_RUN] == 0.0) return;
  rig_inner_stats(P, s4, s_tot);
  const int cur = P.ctl->cur, tid = threadIdx.x;
  double st2 = 0.0, xn2 = 0.0;
  for (int64_t i = tid; i < (int64_t)P.C + P.F; i += 256) {
    const bool cam = i < P.C;
    if (cam ? P.pcol[i] < 0 : P.fgoff[i - P.C + 1] == P.fgoff[i - P.C]) continue;
    const double* x0 = cam ? P.cam + ((size_t)cur * P.C + i) * 8 : P.pose + ((size_t)cur * P.F + (i - P.C)) * 8;
    const double* x1 = cam ? P.cam + ((size_t)(cur ^ 1) * P.C + i) * 8 : P.pose + ((size_t)(cur ^ 1) * P.F + (i - P.C)) * 8;
    for (int k = 0; k < 7; ++k) { const double d = x1[k] - x0[k]; st2 += d * d; xn2 += x1[k] * x1[k]; }
  }
  st2 = rig_inner_sum256(st2, s4);
  __syncthreads();
  xn2 = rig_inner_sum256(xn2, s4);
  if (tid != 0) return;
  LmCtl c = *P.ctl;
  const LmOpts o = *P.opts;
  const double cand = P.st[RIG_IN_CAND], c_in = s_tot[0];
  const bool useful = c_in < c.x_cost;
  LmTrial t;
  t.valid = 1; t.conv = 0; t.accept = 0;
  t.mcc = -P.st[RIG_IN_QMODEL] + (cand - c_in);
  t.cand_cost = isfinite(c_in) ? c_in : 1.7976931348623157e308;
  t.step_norm = sqrt(st2);
  t.cost_change = c.x_cost - t.cand_cost;
  t.quality = 0.0;
  if (t.step_norm <= o.parameter_tolerance * (c.x_norm + o.parameter_tolerance)) t.conv = 1;
  else if (fabs(t.cost_change) <= o.function_tolerance * c.x_cost) t.conv = 2;
  else {
    const double rel = (c.current_cost - t.cand_cost) / t.mcc;
    const double hist = (c.reference_cost - t.cand_cost) / (c.acc_ref + t.mcc);
    t.quality = fmax(rel, hist);
    t.accept = useful || t.quality > o.min_relative_decrease;
  }
  cc_iteration rec;
  const int len0 = c.log_len;
  lm_apply(c, o, &rec, t, xn2);
  if (c.log_len != len0 && c.log_len <= P.log_cap) P.log[c.log_len - 1] = rec;
  *P.ctl = c;
  *P.ctl_next = c;
  P.st[RIG_IN_PASSES] += 1.0;
  P.st[RIG_IN_USEFUL] += useful ? 1.0 : 0.0;
  P.st[RIG_IN_REMOVED] += cand - c_in;
  if (!(1.0 - c_in / cand > P.st[RIG_IN_TOL])) P.st[RIG_IN_ENABLED] = 0.0;
}

void rig_inner_enqueue_groups(const RigInnerDev& I, hipStream_t s, int buf) {
  hipLaunchKernelGGL((k_rig_inner_block<0, 1024>), dim3((unsigned)I.C), dim3(1024), 0, s, I, buf);
  hipLaunchKernelGGL((k_rig_inner_block<1, 1024>), dim3((unsigned)I.C), dim3(1024), 0, s, I, buf);
  hipLaunchKernelGGL((k_rig_inner_block<2, 256>), dim3((unsigned)I.F), dim3(256), 0, s, I, buf);
  hipLaunchKernelGGL((k_rig_inner_block<3, 256>), dim3((unsigned)I.F), dim3(256), 0, s, I, buf);
}

void rig_inner_enqueue_before_sweep(const RigInnerDev& I, hipStream_t s) {
  hipLaunchKernelGGL(k_rig_inner_begin, dim3(1), dim3(256), 0, s, I);
  rig_inner_enqueue_groups(I, s, -1);
  hipLaunchKernelGGL(k_rig_inner_records, dim3((unsigned)((I.C + I.F + 255) / 256)), dim3(256), 0, s, I);
}

void rig_inner_enqueue_decide(const RigInnerDev& I, hipStream_t s) {
  hipLaunchKernelGGL(k_rig_inner_decide, dim3(1), dim3(256), 0, s, I);
}

}  // namespace cc
