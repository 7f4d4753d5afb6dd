// The index map of the Gram product on 4 x 4 blocks, on the host (tests/test_gram_blocks_cpu.py builds and runs this).
// cc_gram_blocks.hpp alone -- no device code -- is shown to give, for every pair of row sets of a staged tile:
//   1. coverage: the five products of a pair hold, for each chain, exactly one block of every transposed pair of blocks -- the four
//      diagonal blocks and one of (bi, bj) / (bj, bi) for the six others -- 4 x 4 entries each, and nothing else; gb_entry_acc /
//      gb_entry_lane find every entry of the 16 x 16 block, itself or its transposed twin;
//   2. operands: for every accumulator lane and every k, the A operand lane the hardware multiplies (lane k << 4 | slot << 2 | i)
//      reads component `row` and the B operand lane (k << 4 | slot << 2 | j) component `column` of the SAME staged row
//      4 (2 pair + chain) + k; a pair on is kGbPairRows rows on and leaves row & 7 alone;
//   3. reduction: accumulators 0 and 1, and 2 and 3, hold the same entry of chain 0 and chain 1 in the same lane, lanes l and l ^ 8
//      of accumulator 4 the same entry of chain 0 and chain 1; the stores (entry; entry and mirror; entry, or mirror from the lanes
//      of slots 2, 3) place every one of the 256 entries exactly once;
//   4. bits: a host emulation -- per entry a plain loop of fma over k in order, chains, chain sum and wave sum as specified --
//      reproduces the emulation of gram_products (16 x 16 x 4, acc0 / acc1) + today's reduction bit for bit on random rows of four
//      waves with ragged passes.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "cc_gram_blocks.hpp"

using namespace cc;

static long bad = 0;
#define CHECK(x) do { if (!(x)) { if (++bad <= 10) printf("line %d: %s\n", __LINE__, #x); } } while (0)

static int a_lane(int lane, int k) { return k << 4 | gb_slot(lane) << 2 | (lane >> 4); }
static int b_lane(int lane, int k) { return k << 4 | gb_slot(lane) << 2 | (lane & 3); }

// the 16 x 16 block of one wave from its staged tiles (tiles x 64 rows x 16), today: gram_products + acc0[r] + acc1[r]
static void block_16x16x4(const std::vector<double>& rows, int tiles, double* blk) {
  for (int r = 0; r < 16; ++r)
    for (int c = 0; c < 16; ++c) {
      double acc[2] = {0.0, 0.0};
      for (int t = 0; t < tiles; ++t)
        for (int m = 0; m < 16; ++m)
          for (int k = 0; k < 4; ++k) {
            const double* row = &rows[((size_t)t * 64 + 4 * m + k) * 16];
            acc[m & 1] = std::fma(row[r], row[c], acc[m & 1]);
          }
      blk[r * 16 + c] = acc[0] + acc[1];
    }
}
// the same through the map: five accumulators of 64 lanes, operands by gb_op_row / gb_op_comp, then the reduction's stores
static void block_4x4x4(const std::vector<double>& rows, int tiles, double* blk) {
  double acc[kGbProducts][64] = {};
  for (int t = 0; t < tiles; ++t)
    for (int p = 0; p < kGbPairs; ++p)
      for (int n = 0; n < kGbProducts; ++n)
        for (int lane = 0; lane < 64; ++lane)
          for (int k = 0; k < 4; ++k) {
            const int la = a_lane(lane, k), lb = b_lane(lane, k), oa = gb_prod_a(n), ob = gb_prod_b(n);
            const double a = rows[((size_t)t * 64 + gb_op_row(oa, p, la)) * 16 + gb_op_comp(oa, la)];
            const double b = rows[((size_t)t * 64 + gb_op_row(ob, p, lb)) * 16 + gb_op_comp(ob, lb)];
            acc[n][lane] = std::fma(a, b, acc[n][lane]);
          }
  for (int e = 0; e < 256; ++e) blk[e] = NAN;
  for (int lane = 0; lane < 64; ++lane) {
    blk[gb_acc_row(0, lane) * 16 + gb_acc_col(0, lane)] = acc[0][lane] + acc[1][lane];
    const double s = acc[2][lane] + acc[3][lane];
    blk[gb_acc_row(2, lane) * 16 + gb_acc_col(2, lane)] = s;
    blk[gb_acc_col(2, lane) * 16 + gb_acc_row(2, lane)] = s;
    const double t = acc[4][lane] + acc[4][gb_partner_lane(lane)];
    const int r = gb_acc_row(4, lane), c = gb_acc_col(4, lane);
    blk[gb_store_mirrored(lane) ? c * 16 + r : r * 16 + c] = t;
  }
}

int main() {
  // 1. coverage
  for (int chain = 0; chain < 2; ++chain) {
    int held[16][16] = {};
    for (int n = 0; n < kGbProducts; ++n)
      for (int lane = 0; lane < 64; ++lane)
        if (gb_acc_chain(n, lane) == chain) ++held[gb_acc_row(n, lane)][gb_acc_col(n, lane)];
    for (int r = 0; r < 16; ++r)
      for (int c = 0; c < 16; ++c) {
        if (r / 4 == c / 4) CHECK(held[r][c] == 1);
        else CHECK(held[r][c] + held[c][r] == 1 && held[r][c] == held[4 * (r / 4)][4 * (c / 4)]);   // one block of the pair, whole
        CHECK(gb_entry_held(chain, r, c) == (held[r][c] == 1));
        const int n = gb_entry_acc(chain, r, c), lane = gb_entry_lane(chain, r, c);
        CHECK(n >= 0 && n < kGbProducts && lane >= 0 && lane < 64 && gb_acc_chain(n, lane) == chain);
        if (held[r][c]) CHECK(gb_acc_row(n, lane) == r && gb_acc_col(n, lane) == c);
        else CHECK(gb_acc_row(n, lane) == c && gb_acc_col(n, lane) == r);
      }
  }
  for (int n = 0; n < kGbProducts; ++n) {   // by product: whole blocks, four of one chain or two of each
    int blocks[2][4][4] = {};
    for (int lane = 0; lane < 64; ++lane) {
      CHECK(gb_acc_chain(n, lane) == 0 || gb_acc_chain(n, lane) == 1);
      CHECK(gb_op_set(gb_prod_a(n), gb_slot(lane)) == gb_acc_chain(n, lane));   // both operand blocks of a slot from one row set
      ++blocks[gb_acc_chain(n, lane)][gb_acc_row(n, lane) / 4][gb_acc_col(n, lane) / 4];
    }
    for (int ch = 0; ch < 2; ++ch)
      for (int bi = 0; bi < 4; ++bi)
        for (int bj = 0; bj < 4; ++bj) CHECK(blocks[ch][bi][bj] == 0 || blocks[ch][bi][bj] == 16);
  }
  // 2. operands
  for (int p = 0; p < kGbPairs; ++p)
    for (int n = 0; n < kGbProducts; ++n)
      for (int lane = 0; lane < 64; ++lane)
        for (int k = 0; k < 4; ++k) {
          const int la = a_lane(lane, k), lb = b_lane(lane, k), oa = gb_prod_a(n), ob = gb_prod_b(n);
          const int want = 4 * (2 * p + gb_acc_chain(n, lane)) + k;   // row k of the chain's row set of this pair: gram_products' m = 2 p + chain
          CHECK(gb_op_row(oa, p, la) == want && gb_op_row(ob, p, lb) == want && want < 64);
          CHECK(gb_op_comp(oa, la) == gb_acc_row(n, lane) && gb_op_comp(ob, lb) == gb_acc_col(n, lane));
        }
  for (int o = 0; o < kGbOperands; ++o)
    for (int p = 0; p < kGbPairs; ++p)
      for (int lane = 0; lane < 64; ++lane) {
        const int r = gb_op_row(o, p, lane), c = gb_op_comp(o, lane);
        CHECK(r >= 0 && r < 64 && c >= 0 && c < 16 && r == gb_op_row(o, 0, lane) + kGbPairRows * p && (r & 7) == (gb_op_row(o, 0, lane) & 7));
        if (o <= GB_A1) CHECK(r == 4 * (2 * p + o) + (lane >> 4) && c == (lane & 15));   // gram_operands' a[2p], a[2p + 1]
      }
  // 3. reduction
  {
    int placed[256] = {};
    for (int lane = 0; lane < 64; ++lane) {
      for (int n = 0; n < 4; n += 2)
        CHECK(gb_acc_chain(n, lane) == 0 && gb_acc_chain(n + 1, lane) == 1 && gb_acc_row(n, lane) == gb_acc_row(n + 1, lane) && gb_acc_col(n, lane) == gb_acc_col(n + 1, lane));
      CHECK(gb_acc_row(0, lane) / 4 == gb_acc_col(0, lane) / 4 && gb_acc_row(2, lane) / 4 != gb_acc_col(2, lane) / 4 && gb_acc_row(4, lane) / 4 != gb_acc_col(4, lane) / 4);
      ++placed[gb_acc_row(0, lane) * 16 + gb_acc_col(0, lane)];
      ++placed[gb_acc_row(2, lane) * 16 + gb_acc_col(2, lane)];
      ++placed[gb_acc_col(2, lane) * 16 + gb_acc_row(2, lane)];
      const int q = gb_partner_lane(lane), r = gb_acc_row(4, lane), c = gb_acc_col(4, lane);
      CHECK(q >= 0 && q < 64 && (q >> 4) == (lane >> 4));   // inside the row of sixteen lanes: a DPP row rotation by eight
      CHECK(gb_acc_chain(4, lane) == (gb_slot(lane) >> 1) && gb_acc_chain(4, q) == 1 - gb_acc_chain(4, lane) && gb_acc_row(4, q) == r && gb_acc_col(4, q) == c);
      CHECK(gb_store_mirrored(lane) == (gb_acc_chain(4, lane) == 1));
      ++placed[gb_store_mirrored(lane) ? c * 16 + r : r * 16 + c];
    }
    for (int e = 0; e < 256; ++e) CHECK(placed[e] == 1);
  }
  // 4. bits
  std::mt19937_64 rng(2024);
  std::normal_distribution<double> nd(0.0, 1.0);
  long entries = 0;
  for (int trial = 0; trial < 6; ++trial) {
    double g_old[256], g_new[256], w_old[4][256], w_new[4][256];
    for (int w = 0; w < 4; ++w) {
      const int tiles = 2 * ((trial + w) % 3);   // u and v tile of 0, 1, 2 passes
      std::vector<double> rows((size_t)tiles * 64 * 16 + 1);
      for (int t = 0; t < tiles; ++t)
        for (int l = 0; l < 64; ++l) {
          const bool idle = t >= tiles - 2 && l >= 64 - 9 * (trial + 1);   // ragged last pass: zero rows
          for (int c = 0; c < 16; ++c) rows[((size_t)t * 64 + l) * 16 + c] = idle ? 0.0 : nd(rng) * std::exp(4.0 * nd(rng));
        }
      block_16x16x4(rows, tiles, w_old[w]);
      block_4x4x4(rows, tiles, w_new[w]);
    }
    for (int e = 0; e < 256; ++e) {
      g_old[e] = (w_old[0][e] + w_old[1][e]) + (w_old[2][e] + w_old[3][e]);
      g_new[e] = (w_new[0][e] + w_new[1][e]) + (w_new[2][e] + w_new[3][e]);
      CHECK(std::memcmp(&g_old[e], &g_new[e], 8) == 0);
      for (int w = 0; w < 4; ++w) CHECK(std::memcmp(&w_old[w][e], &w_new[w][e], 8) == 0);
      ++entries;
    }
  }
  printf("%ld entries, %ld mismatches\n", entries, bad);
  return bad != 0;
}
