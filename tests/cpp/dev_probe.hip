// dev_probe.hip -- test-only probe of the shared device primitives (tests/test_gpu_dev_primitives.py) and of the stages of Zhang's initialisation (tests/test_gpu_zhang_stages.py). One thin kernel per
// primitive around the inlined helper, one extern "C" entry per kernel: copy in, one launch, synchronise, copy out. Built by
// `make probe` in camera_calibrator_amd/csrc with the product's flags (contraction and fast-math settings decide the
// arithmetic of inlined code); never linked into libcc_hip.so. Nothing here waits or spins: the polling helpers of
// cc_persist_dev.hpp are tested in place (tests/test_gpu_persist.py). Every entry returns the hipError_t of its first
// failing call (0: fine).
#include <type_traits>

#include "cc_common.hpp"
#include "cc_device.hpp"
#include "cc_persist_dev.hpp"
#include "cc_rig_dev.hpp"
#include "cc_zhang_dev.hpp"

namespace {

using namespace cc;

#define PROBE_TRY(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return (int)e_; } while (0)

// device buffers of one entry: freed when the entry returns, whatever the way out
struct Bufs {
  void* p[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int n = 0;
  ~Bufs() { for (int i = 0; i < n; ++i) (void)hipFree(p[i]); }
  template <class T>
  hipError_t in(T** d, const T* h, size_t count) {
    hipError_t e = hipMalloc((void**)d, (count ? count : 1) * sizeof(T));
    if (e != hipSuccess) return e;
    p[n++] = *d;
    return count ? hipMemcpy(*d, h, count * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
  }
  template <class T>
  hipError_t out(T** d, size_t count) {
    hipError_t e = hipMalloc((void**)d, (count ? count : 1) * sizeof(T));
    if (e != hipSuccess) return e;
    p[n++] = *d;
    return hipMemset(*d, 0, (count ? count : 1) * sizeof(T));
  }
};
template <class T>
hipError_t finish(T* h, const T* d, size_t count) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  e = hipDeviceSynchronize();
  if (e != hipSuccess) return e;
  return count ? hipMemcpy(h, d, count * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess;
}

// ---- lane reductions: one wave, one value per lane in, the helper's return value of every lane out
__global__ __launch_bounds__(64) void k_lane_reduce(int which, const double* in, double* out) {
  const int lane = threadIdx.x;
  const double v = in[lane];
  double r = 0.0;
  switch (which) {
    case 0: r = wave_sum_mod<0>(v); break;
    case 1: r = wave_sum_mod<1>(v); break;
    case 2: r = wave_sum_mod<2>(v); break;
    case 3: r = wave_sum_mod<3>(v); break;
    case 4: r = row16_sum(v); break;
    case 5: r = row16_max(v); break;
    case 6: r = row_pair_sum(v); break;
    case 7: r = half_pair_sum(v); break;
    default: break;
  }
  out[lane] = r;
}
template <int N>
__global__ __launch_bounds__(64) void k_scatter(const double* in /*[64][N]*/, double* out /*[64]*/) {
  const int lane = threadIdx.x;
  double p[N];
#pragma unroll
  for (int e = 0; e < N; ++e) p[e] = in[lane * N + e];
  if (N == 32) reduce_scatter32(p, lane); else reduce_scatter64(p, lane);
  out[lane] = p[0];
}
__global__ __launch_bounds__(256) void k_block_sum(const double* in, double* out) {
  __shared__ double s4[4];
  out[threadIdx.x] = block_sum256(in[threadIdx.x], s4);
}

// ---- Gram contraction: one wave, `npass` passes of 64 staged rows into the same accumulators, stored with the
// lane -> entry map of k_zhang_gram (entry ((lane >> 4) + 4 r, lane & 15) = acc0[r] + acc1[r])
__global__ __launch_bounds__(64) void k_gram(int form, int npass, const double* rows /*[npass * 64][16]*/, double* out /*[3][256]*/) {
  __shared__ __attribute__((aligned(16))) double stage[kStageDoublesPerWave];
  const int lane = threadIdx.x;
  d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
  for (int p = 0; p < npass; ++p) {
    double v[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) v[c] = rows[((size_t)p * 64 + lane) * 16 + c];
    stage_row(stage, lane, v);
    wave_lds_fence();
    if (form == 0) {
      gram_rows(stage, lane, acc0, acc1);
    } else if (form == 1) {
      double a[16];
      gram_operands(stage, lane, a);
      gram_products(a, acc0, acc1);
    } else {
      gram_rows_ahead(stage, lane, acc0, acc1);
    }
    wave_lds_fence();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {   // the block, then the two accumulators it is the sum of
    const int e = ((lane >> 4) + 4 * r) * 16 + (lane & 15);
    out[e] = acc0[r] + acc1[r];
    out[256 + e] = acc0[r];
    out[512 + e] = acc1[r];
  }
}

// ---- scalar maps, one block of 256 threads striding over n inputs
__global__ __launch_bounds__(256) void k_scalar(int which, int n, const double* in, double* out) {
  for (int i = threadIdx.x; i < n; i += 256) out[i] = which == 0 ? rsqrt_pos(in[i]) : recip_depth(in[i]);
}
__global__ __launch_bounds__(256) void k_quat_plus(int tab, int n, const double* x, const double* d, double* out) {
  for (int i = threadIdx.x; i < n; i += 256) {
    const double xi[4] = {x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]};
    const double di[3] = {d[3 * i], d[3 * i + 1], d[3 * i + 2]};
    double o[4];
    if (tab) quat_plus_tab(xi, di, o); else quat_plus(xi, di, o);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[4 * i + k] = o[k];
  }
}
__global__ __launch_bounds__(256) void k_quat_to_R(int n, const double* q, double* R) {
  for (int i = threadIdx.x; i < n; i += 256) {
    const double qi[4] = {q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]};
    double r[9];
    quat_to_R(qi, r);
#pragma unroll
    for (int k = 0; k < 9; ++k) R[9 * i + k] = r[k];
  }
}
__global__ __launch_bounds__(256) void k_pose_grad(int tab, int n, const double* q, const double* g, double* out) {
  for (int i = threadIdx.x; i < n; i += 256) {
    const double qi[4] = {q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]};
    const double gi[6] = {g[6 * i], g[6 * i + 1], g[6 * i + 2], g[6 * i + 3], g[6 * i + 4], g[6 * i + 5]};
    out[i] = tab ? pose_grad_proj_max_tab(qi, gi) : pose_grad_proj_max(qi, gi);
  }
}
// words[2 i], words[2 i + 1]: the two granules of bits[i] under tag[i]; back[i]: what ungranule makes of them
__global__ __launch_bounds__(256) void k_granule(int n, const unsigned* tag, const u64* bits, u64* words, u64* back) {
  for (int i = threadIdx.x; i < n; i += 256) {
    const double v = __longlong_as_double((long long)bits[i]);
    const u64 lo = granule(tag[i], v, 0), hi = granule(tag[i], v, 1);
    words[2 * i] = lo;
    words[2 * i + 1] = hi;
    back[i] = (u64)__double_as_longlong(ungranule(lo, hi));
  }
}
// the series table of quat_plus_tab / pose_grad_proj_max_tab as the device holds it
__global__ __launch_bounds__(64) void k_plus_coef(double* out) {
  if (threadIdx.x < 16) out[threadIdx.x] = kPlusCoef[threadIdx.x];
}
__global__ __launch_bounds__(256) void k_untri(int n, int* ij) {
  for (int idx = threadIdx.x; idx < n; idx += 256) {
    int i, j;
    untri(idx, i, j);
    ij[2 * idx] = i;
    ij[2 * idx + 1] = j;
  }
}
// out[2 i]: persist_spec_radius; out[2 i + 1]: the radius lm_apply leaves after an accepted step of quality 1
__global__ __launch_bounds__(256) void k_spec_radius(int n, const double* radius, const double* max_radius, double* out) {
  for (int i = threadIdx.x; i < n; i += 256) {
    out[2 * i] = persist_spec_radius(radius[i], max_radius[i]);
    LmCtl st = {};
    st.radius = radius[i];
    st.decrease_factor = 2.0;
    st.step_valid = 1;
    LmOpts o = {};
    o.max_iterations = 1 << 30;
    o.max_radius = max_radius[i];
    LmTrial t = {};
    t.valid = 1; t.accept = 1; t.quality = 1.0; t.mcc = 1.0; t.cand_cost = 1.0; t.cost_change = 1.0; t.step_norm = 1.0;
    lm_apply(st, o, nullptr, t, 1.0);
    out[2 * i + 1] = st.radius;
  }
}

// ---- chol_solve_rows<S>: one wave per system; lane l hands over a[l][0..S) and b[l] as they are (all 64 lanes, every
// entry: what the contract calls ignored is the caller's to choose), every lane's x and return value come back
template <int S>
__global__ __launch_bounds__(64) void k_chol_rows(const double* a /*[nsys][64][S]*/, const double* b /*[nsys][64]*/,
                                                 double* x /*[nsys][64][S]*/, int* ok /*[nsys][64]*/) {
  const int lane = threadIdx.x;
  const size_t sys = blockIdx.x;
  double ar[S], xr[S];
#pragma unroll
  for (int k = 0; k < S; ++k) ar[k] = a[(sys * 64 + lane) * S + k];
  const bool r = chol_solve_rows<S>(ar, b[sys * 64 + lane], xr);
#pragma unroll
  for (int k = 0; k < S; ++k) x[(sys * 64 + lane) * S + k] = xr[k];
  ok[sys * 64 + lane] = r ? 1 : 0;
}

// ---- chol_block4 + chol_backward<false>: one workgroup of 256 per system, matrix and right-hand side (row S) in LDS with
// the row stride of rig_solve_block; the substitution on wave 0 as rig_solve_block runs it
constexpr int kBlock4MaxS = 63;
__global__ __launch_bounds__(256) void k_chol_block4(int S, const double* M /*[nsys][S + 1][S + 1]*/, double* x /*[nsys][64]*/,
                                                    int* ok /*[nsys][256]*/) {
  __shared__ double A[(kBlock4MaxS + 1) * (kBlock4MaxS + 2)];
  __shared__ double s_inv[64];
  const int tid = threadIdx.x, lane = tid & 63, LD = (S + 1) | 1;
  const size_t sys = blockIdx.x;
  for (int i = tid; i < (kBlock4MaxS + 1) * (kBlock4MaxS + 2); i += 256) A[i] = 0.0;
  if (tid < 64) s_inv[tid] = 0.0;
  __syncthreads();
  for (int e = tid; e < (S + 1) * (S + 1); e += 256) A[(e / (S + 1)) * LD + e % (S + 1)] = M[sys * (S + 1) * (S + 1) + e];
  __syncthreads();
  const bool okb = chol_block4(A, S, LD, s_inv);
  if (tid < 64) {
    const int i0 = lane;
    double b0 = i0 < S ? A[(size_t)S * LD + i0] : 0.0, b1 = 0.0;   // y = L^-1 b (row S of the matrix)
    const double v0 = i0 < S ? s_inv[i0] : 0.0;
    chol_backward<false>(A, S, LD, b0, b1, v0, 0.0);
    x[sys * 64 + lane] = i0 < S ? b0 : 0.0;
  }
  ok[sys * 256 + tid] = okb ? 1 : 0;
}

// ---- Zhang initialisation (cc_zhang_dev.hpp): the four kernels are launched as they are; these two wrap the helpers they
// inline. One thread per matrix, as k_zhang_eig9 has it.
template <int N>
__global__ __launch_bounds__(64) void k_smallest_eigvec(int64_t count, const double* A /*[count][N][N]*/, double* x /*[count][N]*/) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= count) return;
  double a[N][N], v[N];
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) a[i][j] = A[f * N * N + i * N + j];
  smallest_eigvec<N>(a, v);
#pragma unroll
  for (int i = 0; i < N; ++i) x[f * N + i] = v[i];
}
__global__ __launch_bounds__(64) void k_jacobi_eigen3(int64_t count, const double* S /*[count][3][3]*/, double* lam /*[count][3]*/,
                                                      double* V /*[count][3][3]*/) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= count) return;
  double s[3][3], v[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) s[i][j] = S[f * 9 + i * 3 + j];
  jacobi_eigen<3>(s, v, 10);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    lam[f * 3 + i] = s[i][i];
#pragma unroll
    for (int j = 0; j < 3; ++j) V[f * 9 + i * 3 + j] = v[i][j];
  }
}

}  // namespace

extern "C" {

int probe_lane_reduce(int which, const double* in, double* out) {
  if (which < 0 || which > 7) return -1;
  Bufs B; double *d_in, *d_out;
  PROBE_TRY(B.in(&d_in, in, 64)); PROBE_TRY(B.out(&d_out, 64));
  hipLaunchKernelGGL(k_lane_reduce, dim3(1), dim3(64), 0, 0, which, d_in, d_out);
  return (int)finish(out, d_out, 64);
}
int probe_reduce_scatter(int n, const double* in, double* out) {
  if (n != 32 && n != 64) return -1;
  Bufs B; double *d_in, *d_out;
  PROBE_TRY(B.in(&d_in, in, (size_t)64 * n)); PROBE_TRY(B.out(&d_out, 64));
  if (n == 32) hipLaunchKernelGGL(k_scatter<32>, dim3(1), dim3(64), 0, 0, d_in, d_out);
  else hipLaunchKernelGGL(k_scatter<64>, dim3(1), dim3(64), 0, 0, d_in, d_out);
  return (int)finish(out, d_out, 64);
}
int probe_block_sum256(const double* in, double* out) {
  Bufs B; double *d_in, *d_out;
  PROBE_TRY(B.in(&d_in, in, 256)); PROBE_TRY(B.out(&d_out, 256));
  hipLaunchKernelGGL(k_block_sum, dim3(1), dim3(256), 0, 0, d_in, d_out);
  return (int)finish(out, d_out, 256);
}
int probe_gram(int form, int npass, const double* rows, double* out) {
  if (form < 0 || form > 2 || npass < 1 || npass > 64) return -1;
  Bufs B; double *d_in, *d_out;
  PROBE_TRY(B.in(&d_in, rows, (size_t)npass * 64 * 16)); PROBE_TRY(B.out(&d_out, 768));
  hipLaunchKernelGGL(k_gram, dim3(1), dim3(64), 0, 0, form, npass, d_in, d_out);
  return (int)finish(out, d_out, 768);
}
int probe_scalar(int which, int n, const double* in, double* out) {
  if (which < 0 || which > 1 || n < 0) return -1;
  Bufs B; double *d_in, *d_out;
  PROBE_TRY(B.in(&d_in, in, (size_t)n)); PROBE_TRY(B.out(&d_out, (size_t)n));
  hipLaunchKernelGGL(k_scalar, dim3(1), dim3(256), 0, 0, which, n, d_in, d_out);
  return (int)finish(out, d_out, (size_t)n);
}
int probe_quat_plus(int tab, int n, const double* x, const double* d, double* out) {
  if (n < 0) return -1;
  Bufs B; double *d_x, *d_d, *d_out;
  PROBE_TRY(B.in(&d_x, x, (size_t)4 * n)); PROBE_TRY(B.in(&d_d, d, (size_t)3 * n)); PROBE_TRY(B.out(&d_out, (size_t)4 * n));
  hipLaunchKernelGGL(k_quat_plus, dim3(1), dim3(256), 0, 0, tab, n, d_x, d_d, d_out);
  return (int)finish(out, d_out, (size_t)4 * n);
}
int probe_quat_to_R(int n, const double* q, double* R) {
  if (n < 0) return -1;
  Bufs B; double *d_q, *d_R;
  PROBE_TRY(B.in(&d_q, q, (size_t)4 * n)); PROBE_TRY(B.out(&d_R, (size_t)9 * n));
  hipLaunchKernelGGL(k_quat_to_R, dim3(1), dim3(256), 0, 0, n, d_q, d_R);
  return (int)finish(R, d_R, (size_t)9 * n);
}
int probe_pose_grad(int tab, int n, const double* q, const double* g, double* out) {
  if (n < 0) return -1;
  Bufs B; double *d_q, *d_g, *d_out;
  PROBE_TRY(B.in(&d_q, q, (size_t)4 * n)); PROBE_TRY(B.in(&d_g, g, (size_t)6 * n)); PROBE_TRY(B.out(&d_out, (size_t)n));
  hipLaunchKernelGGL(k_pose_grad, dim3(1), dim3(256), 0, 0, tab, n, d_q, d_g, d_out);
  return (int)finish(out, d_out, (size_t)n);
}
int probe_granule(int n, const unsigned* tag, const unsigned long long* bits, unsigned long long* words, unsigned long long* back) {
  if (n < 0) return -1;
  Bufs B; unsigned* d_tag; cc::u64 *d_bits, *d_words, *d_back;
  PROBE_TRY(B.in(&d_tag, tag, (size_t)n)); PROBE_TRY(B.in(&d_bits, (const cc::u64*)bits, (size_t)n));
  PROBE_TRY(B.out(&d_words, (size_t)2 * n)); PROBE_TRY(B.out(&d_back, (size_t)n));
  hipLaunchKernelGGL(k_granule, dim3(1), dim3(256), 0, 0, n, d_tag, d_bits, d_words, d_back);
  PROBE_TRY(finish((cc::u64*)words, d_words, (size_t)2 * n));
  return (int)hipMemcpy(back, d_back, (size_t)n * sizeof(cc::u64), hipMemcpyDeviceToHost);
}
int probe_plus_coef(double* out) {
  Bufs B; double* d_out;
  PROBE_TRY(B.out(&d_out, 16));
  hipLaunchKernelGGL(k_plus_coef, dim3(1), dim3(64), 0, 0, d_out);
  return (int)finish(out, d_out, 16);
}
int probe_untri(int n, int* ij) {
  if (n < 0) return -1;
  Bufs B; int* d_ij;
  PROBE_TRY(B.out(&d_ij, (size_t)2 * n));
  hipLaunchKernelGGL(k_untri, dim3(1), dim3(256), 0, 0, n, d_ij);
  return (int)finish(ij, d_ij, (size_t)2 * n);
}
int probe_spec_radius(int n, const double* radius, const double* max_radius, double* out) {
  if (n < 0) return -1;
  Bufs B; double *d_r, *d_m, *d_out;
  PROBE_TRY(B.in(&d_r, radius, (size_t)n)); PROBE_TRY(B.in(&d_m, max_radius, (size_t)n)); PROBE_TRY(B.out(&d_out, (size_t)2 * n));
  hipLaunchKernelGGL(k_spec_radius, dim3(1), dim3(256), 0, 0, n, d_r, d_m, d_out);
  return (int)finish(out, d_out, (size_t)2 * n);
}
int probe_chol_rows(int S, int nsys, const double* a, const double* b, double* x, int* ok) {
  if (nsys < 1 || nsys > 4096 || (S != 6 && S != 9 && S != 12 && S != 18 && S != 24)) return -1;
  Bufs B; double *d_a, *d_b, *d_x; int* d_ok;
  PROBE_TRY(B.in(&d_a, a, (size_t)nsys * 64 * S)); PROBE_TRY(B.in(&d_b, b, (size_t)nsys * 64));
  PROBE_TRY(B.out(&d_x, (size_t)nsys * 64 * S)); PROBE_TRY(B.out(&d_ok, (size_t)nsys * 64));
  switch (S) {
    case 6: hipLaunchKernelGGL(k_chol_rows<6>, dim3(nsys), dim3(64), 0, 0, d_a, d_b, d_x, d_ok); break;
    case 9: hipLaunchKernelGGL(k_chol_rows<9>, dim3(nsys), dim3(64), 0, 0, d_a, d_b, d_x, d_ok); break;
    case 12: hipLaunchKernelGGL(k_chol_rows<12>, dim3(nsys), dim3(64), 0, 0, d_a, d_b, d_x, d_ok); break;
    case 18: hipLaunchKernelGGL(k_chol_rows<18>, dim3(nsys), dim3(64), 0, 0, d_a, d_b, d_x, d_ok); break;
    default: hipLaunchKernelGGL(k_chol_rows<24>, dim3(nsys), dim3(64), 0, 0, d_a, d_b, d_x, d_ok); break;
  }
  PROBE_TRY(finish(x, d_x, (size_t)nsys * 64 * S));
  return (int)hipMemcpy(ok, d_ok, (size_t)nsys * 64 * sizeof(int), hipMemcpyDeviceToHost);
}
int probe_chol_block4(int S, int nsys, const double* M, double* x, int* ok) {
  if (nsys < 1 || nsys > 4096 || S < 1 || S > kBlock4MaxS) return -1;
  Bufs B; double *d_M, *d_x; int* d_ok;
  PROBE_TRY(B.in(&d_M, M, (size_t)nsys * (S + 1) * (S + 1)));
  PROBE_TRY(B.out(&d_x, (size_t)nsys * 64)); PROBE_TRY(B.out(&d_ok, (size_t)nsys * 256));
  hipLaunchKernelGGL(k_chol_block4, dim3(nsys), dim3(256), 0, 0, S, d_M, d_x, d_ok);
  PROBE_TRY(finish(x, d_x, (size_t)nsys * 64));
  return (int)hipMemcpy(ok, d_ok, (size_t)nsys * 256 * sizeof(int), hipMemcpyDeviceToHost);
}

// k_zhang_gram itself, with its own block size and LDS size: off[F + 1], uv[off[F]][2], xyz[off[F]][3] -> gram[F][256]
int probe_zhang_gram(long long F, const long long* off, const float* uv, const float* xyz, double* gram) {
  if (F < 1 || F > 4096 || !off || off[0] != 0) return -1;
  for (long long f = 0; f < F; ++f)
    if (off[f + 1] <= off[f]) return -1;   // (every frame has a point: the padding lanes re-read point off[f])
  const size_t N = (size_t)off[F];
  if (N > ((size_t)1 << 24)) return -1;
  Bufs B; int64_t* d_off; float *d_uv, *d_xyz; double* d_gram;
  static_assert(sizeof(long long) == sizeof(int64_t), "offsets are passed as they are");
  PROBE_TRY(B.in(&d_off, (const int64_t*)off, (size_t)F + 1)); PROBE_TRY(B.in(&d_uv, uv, N * 2)); PROBE_TRY(B.in(&d_xyz, xyz, N * 3));
  PROBE_TRY(B.out(&d_gram, (size_t)F * 256));
  hipLaunchKernelGGL(k_zhang_gram, dim3((unsigned)F), dim3(kZhangThreads), kZhangLdsBytes, 0, (int64_t)F, d_off, d_uv, d_xyz, d_gram);
  return (int)finish(gram, d_gram, (size_t)F * 256);
}
int probe_smallest_eigvec(int N, long long count, const double* A, double* x) {
  if ((N != 6 && N != 9) || count < 1 || count > (1 << 20)) return -1;
  Bufs B; double *d_A, *d_x;
  PROBE_TRY(B.in(&d_A, A, (size_t)count * N * N)); PROBE_TRY(B.out(&d_x, (size_t)count * N));
  const dim3 grid((unsigned)((count + 63) / 64));
  if (N == 6) hipLaunchKernelGGL(k_smallest_eigvec<6>, grid, dim3(64), 0, 0, (int64_t)count, d_A, d_x);
  else hipLaunchKernelGGL(k_smallest_eigvec<9>, grid, dim3(64), 0, 0, (int64_t)count, d_A, d_x);
  return (int)finish(x, d_x, (size_t)count * N);
}
int probe_zhang_eig9(long long F, const double* gram /*[F][256]*/, float* H /*[F][9]*/) {
  if (F < 1 || F > (1 << 20)) return -1;
  Bufs B; double* d_gram; float* d_H;
  PROBE_TRY(B.in(&d_gram, gram, (size_t)F * 256)); PROBE_TRY(B.out(&d_H, (size_t)F * 9));
  hipLaunchKernelGGL(k_zhang_eig9, dim3((unsigned)((F + 63) / 64)), dim3(64), 0, 0, (int64_t)F, d_gram, d_H);
  return (int)finish(H, d_H, (size_t)F * 9);
}
int probe_zhang_k(long long F, const float* Hs /*[F][9]*/, float* K9) {
  if (F < 1 || F > (1 << 20)) return -1;
  Bufs B; float *d_H, *d_K;
  PROBE_TRY(B.in(&d_H, Hs, (size_t)F * 9)); PROBE_TRY(B.out(&d_K, 9));
  hipLaunchKernelGGL(k_zhang_k, dim3(1), dim3(256), 0, 0, (int64_t)F, d_H, d_K);
  return (int)finish(K9, d_K, 9);
}
int probe_zhang_poses(long long F, const float* Hs /*[F][9]*/, const float* K9, float* q /*[F][4]*/, float* t /*[F][3]*/) {
  if (F < 1 || F > (1 << 20)) return -1;
  Bufs B; float *d_H, *d_K, *d_q, *d_t;
  PROBE_TRY(B.in(&d_H, Hs, (size_t)F * 9)); PROBE_TRY(B.in(&d_K, K9, 9));
  PROBE_TRY(B.out(&d_q, (size_t)F * 4)); PROBE_TRY(B.out(&d_t, (size_t)F * 3));
  hipLaunchKernelGGL(k_zhang_poses, dim3((unsigned)((F + 63) / 64)), dim3(64), 0, 0, (int64_t)F, d_H, d_K, d_q, d_t);
  PROBE_TRY(finish(q, d_q, (size_t)F * 4));
  return (int)hipMemcpy(t, d_t, (size_t)F * 3 * sizeof(float), hipMemcpyDeviceToHost);
}
int probe_jacobi_eigen3(long long count, const double* S /*[count][3][3]*/, double* eigenvalues /*[count][3]*/, double* V /*[count][3][3]*/) {
  if (count < 1 || count > (1 << 20)) return -1;
  Bufs B; double *d_S, *d_l, *d_V;
  PROBE_TRY(B.in(&d_S, S, (size_t)count * 9)); PROBE_TRY(B.out(&d_l, (size_t)count * 3)); PROBE_TRY(B.out(&d_V, (size_t)count * 9));
  hipLaunchKernelGGL(k_jacobi_eigen3, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, 0, (int64_t)count, d_S, d_l, d_V);
  PROBE_TRY(finish(eigenvalues, d_l, (size_t)count * 3));
  return (int)hipMemcpy(V, d_V, (size_t)count * 9 * sizeof(double), hipMemcpyDeviceToHost);
}

}  // extern "C"
