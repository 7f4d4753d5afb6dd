// Bit probe: does an entry of a Gram block get the same bits from a chain of v_mfma_f64_4x4x4_4b_f64 products as from the chain
// of v_mfma_f64_16x16x4_f64 products that gram_products runs -- same staged rows, same order, four terms per product? One wave
// stages TILES tiles of 64 rows (stage_row) and forms, per tile and on the same LDS contents,
//   (1) gram_rows_ahead: two chains of 16 x 16 x 4 products (8 TILES products each);
//   (2) gram_blocks_ahead: the packed operands of cc_gram_blocks.hpp, five products per pair of row sets;
//   (3) the ten upper blocks of each chain in three 4 x 4 x 4 instructions, every block with operands read for it alone;
// and gram_blocks_store's 16 x 16 block against acc0 + acc1. Everything is compared with == on the bit patterns, entry by entry.
// Inputs: mixed signs with cancellation, magnitudes whose products span 1e-300 .. 1e300, subnormal products, and rows with the
// structure and magnitudes of a sweep's (pinhole + distortion Jacobian rows of random board points, residual in column 15).
// Build: hipcc --offload-arch=gfx950 -O3 -I camera_calibrator_amd/csrc -o probe_gram_bits scripts/mfma_probe/probe_gram_bits.hip
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "cc_device.hpp"
using namespace cc;

constexpr int TILES = 16;   // 8 TILES = 128 accumulating products per chain

__host__ __device__ constexpr int plain_bi(int b) { return b < 4 ? 0 : b < 7 ? 1 : b < 9 ? 2 : 3; }
__host__ __device__ constexpr int plain_bj(int b) { return b < 4 ? b : b < 7 ? b - 3 : b < 9 ? b - 5 : 3; }
__host__ __device__ constexpr int plain_block(int q, int slot) { return 4 * q + slot < 10 ? 4 * q + slot : 9; }

__device__ __forceinline__ double staged(const double* stage, int r, int c) { return stage[r * 16 + (((c >> 1) ^ (r & 7)) << 1) + (c & 1)]; }

__global__ __launch_bounds__(64) void k(const double* rows, double* out16, double* outb, double* outp, double* outblk) {
  __shared__ __attribute__((aligned(16))) double stage[1024];
  __shared__ double blk[256];
  const int lane = threadIdx.x;
  d4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
  GramBlocks g;
  gram_blocks_clear(g);
  double pl[2][3] = {{0, 0, 0}, {0, 0, 0}};
  for (int t = 0; t < TILES; ++t) {
    double v[16];
    for (int c = 0; c < 16; ++c) v[c] = rows[((size_t)t * 64 + lane) * 16 + c];
    stage_row(stage, lane, v);
    wave_lds_fence();
    gram_rows_ahead(stage, lane, acc0, acc1);
    gram_blocks_ahead<kGbBatchPairs>(stage, lane, g);
#pragma unroll
    for (int p = 0; p < 8; ++p)
#pragma unroll
      for (int ch = 0; ch < 2; ++ch)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const int b = plain_block(q, gb_slot(lane)), r = 4 * (2 * p + ch) + (lane >> 4);
          const double a = staged(stage, r, 4 * plain_bi(b) + (lane & 3)), bb = staged(stage, r, 4 * plain_bj(b) + (lane & 3));
          pl[ch][q] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, bb, pl[ch][q], 0, 0, 0);
        }
    wave_lds_fence();
  }
  for (int r = 0; r < 4; ++r) {
    out16[((lane >> 4) + 4 * r) * 16 + (lane & 15)] = acc0[r];
    out16[256 + ((lane >> 4) + 4 * r) * 16 + (lane & 15)] = acc1[r];
  }
  for (int n = 0; n < kGbProducts; ++n) outb[n * 64 + lane] = g.c[n];
  for (int ch = 0; ch < 2; ++ch)
    for (int q = 0; q < 3; ++q) outp[(ch * 3 + q) * 64 + lane] = pl[ch][q];
  gram_blocks_store(g, lane, blk);
  __syncthreads();
  for (int e = lane; e < 256; e += 64) outblk[e] = blk[e];
}

static bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

static int run(const char* name, const std::vector<double>& rows, double* d_rows, double* d_out) {
  (void)hipMemcpy(d_rows, rows.data(), rows.size() * 8, hipMemcpyHostToDevice);
  (void)hipMemset(d_out, 0xff, (512 + 320 + 384 + 256) * 8);
  hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, d_rows, d_out, d_out + 512, d_out + 832, d_out + 1216);
  std::vector<double> o(1472);
  if (hipMemcpy(o.data(), d_out, o.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) { printf("%s: copy failed\n", name); return 1; }
  const double *o16 = o.data(), *ob = o16 + 512, *op = o16 + 832, *oblk = o16 + 1216;
  int asym = 0, bad_b = 0, bad_p = 0, bad_blk = 0, nonfinite = 0, subnormal = 0;
  for (int ch = 0; ch < 2; ++ch)
    for (int r = 0; r < 16; ++r)
      for (int c = 0; c < 16; ++c) {
        const double v = o16[ch * 256 + r * 16 + c];
        asym += !same(v, o16[ch * 256 + c * 16 + r]);
        nonfinite += !std::isfinite(v);
        subnormal += v != 0.0 && std::fabs(v) < 2.2250738585072014e-308;
      }
  for (int n = 0; n < kGbProducts; ++n)
    for (int l = 0; l < 64; ++l) bad_b += !same(ob[n * 64 + l], o16[gb_acc_chain(n, l) * 256 + gb_acc_row(n, l) * 16 + gb_acc_col(n, l)]);
  for (int ch = 0; ch < 2; ++ch)
    for (int q = 0; q < 3; ++q)
      for (int l = 0; l < 64; ++l) {
        const int b = plain_block(q, gb_slot(l));
        bad_p += !same(op[(ch * 3 + q) * 64 + l], o16[ch * 256 + (4 * plain_bi(b) + (l >> 4)) * 16 + 4 * plain_bj(b) + (l & 3)]);
      }
  for (int e = 0; e < 256; ++e) bad_blk += !same(oblk[e], o16[e] + o16[256 + e]);
  printf("%-28s 16x16x4 chains: %d asymmetric of 512, %d non-finite, %d subnormal | differing bit patterns: packed scheme %d of 320, "
         "block by block %d of 384, stored block vs acc0 + acc1 %d of 256\n", name, asym, nonfinite, subnormal, bad_b, bad_p, bad_blk);
  return asym + bad_b + bad_p + bad_blk;
}

int main() {
  const size_t n = (size_t)TILES * 64 * 16;
  double *d_rows, *d_out;
  (void)hipMalloc(&d_rows, n * 8); (void)hipMalloc(&d_out, 1472 * 8);
  std::mt19937_64 rng(12345);
  std::normal_distribution<double> nd(0.0, 1.0);
  std::uniform_real_distribution<double> ud(0.0, 1.0);
  std::vector<double> rows(n);
  int bad = 0;
  // 1. mixed signs; every second row nearly cancels the one before it in the off-diagonal sums and doubles it on the diagonal
  for (size_t r = 0; r < n / 16; ++r)
    for (int c = 0; c < 16; ++c)
      rows[r * 16 + c] = (r & 1) ? rows[(r - 1) * 16 + c] * ((c & 1) ? -1.0 : 1.0) * (1.0 + 1e-9 * nd(rng)) : nd(rng) * std::exp(3.0 * nd(rng));
  bad += run("mixed signs, cancellation", rows, d_rows, d_out);
  // 2. magnitudes 1e-149 .. 1e149: products 1e-298 .. 1e298 in one chain
  for (auto& v : rows) v = (ud(rng) < 0.5 ? -1.0 : 1.0) * std::pow(10.0, -149.0 + 298.0 * ud(rng)) * (1.0 + ud(rng));
  bad += run("magnitudes 1e-149 .. 1e149", rows, d_rows, d_out);
  // 3. subnormal products and sums, a few normal rows among them
  for (size_t r = 0; r < n / 16; ++r)
    for (int c = 0; c < 16; ++c) rows[r * 16 + c] = nd(rng) * ((r % 37 == 0 && c < 8) ? 1e-150 : std::pow(10.0, -162.0 + 6.0 * ud(rng)));
  bad += run("subnormal products", rows, d_rows, d_out);
  for (auto& v : rows) v = nd(rng) * std::pow(10.0, -161.0 + 4.0 * ud(rng));
  bad += run("subnormal sums only", rows, d_rows, d_out);
  // 4. rows of a sweep: u rows in the even tiles, v rows in the odd ones; columns fx fy cx cy k1 k2 p1 p2 k3 | rotation | translation | residual
  for (int t = 0; t < TILES; ++t)
    for (int l = 0; l < 64; ++l) {
      const double X = 0.4 * nd(rng), Y = 0.3 * nd(rng), Z = 1.0 + 0.5 * ud(rng), x = X / Z, y = Y / Z, r2 = x * x + y * y, fx = 1200.0, fy = 1190.0;
      const double u[16] = {x, 0, 1, 0, fx * x * r2, fx * x * r2 * r2, fx * 2 * x * y, fx * (r2 + 2 * x * x), fx * x * r2 * r2 * r2,
                            -fx * x * y, fx * (1 + x * x), -fx * y, fx / Z, 0, -fx * x / Z, 0.3 * nd(rng)};
      const double w[16] = {0, y, 0, 1, fy * y * r2, fy * y * r2 * r2, fy * (r2 + 2 * y * y), fy * 2 * x * y, fy * y * r2 * r2 * r2,
                            -fy * (1 + y * y), fy * x * y, fy * x, 0, fy / Z, -fy * y / Z, 0.3 * nd(rng)};
      const bool idle = t >= TILES - 2 && l >= 44;   // a ragged last pass: zero rows
      for (int c = 0; c < 16; ++c) rows[((size_t)t * 64 + l) * 16 + c] = idle ? 0.0 : ((t & 1) ? w[c] : u[c]);
    }
  bad += run("sweep rows", rows, d_rows, d_out);
  printf("%s\n", bad ? "DIFFERENT BITS" : "every entry bit-equal in every form");
  return bad ? 1 : 0;
}
