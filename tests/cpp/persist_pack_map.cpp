// The index map of k_intr_persist's residual-only sweep, on the host (tests/test_persist_pack_cpu.py builds and runs this).
// cc_persist_pack.hpp packs the eight cost chains of a team -- two per wave: the accumulators acc0 / acc1 of gram_products -- into one
// chain of 16 x 16 x 4 products whose diagonal entry i is chain i. Checked here, for frames of 1 .. 1100 observations (waves with
// 0 .. 5 passes, teams of one to four waves with observations):
//   1. the writers' slots are distinct, lie inside the team's tiles, and are exactly the slots the chain wave reads as valid;
//   2. chain 2w + a visits, step by step and sub-row by sub-row, the residuals that accumulator a of wave w adds in the full sweep:
//      passes in order, the u rows before the v rows, products m = a, a + 2, ... of a row set, rows 4m .. 4m + 3 of a product;
//   3. entry (i, i) of the accumulator sits where the kernel reads it.
#include <cstdio>
#include <vector>

#include "cc_persist_pack.hpp"

using namespace cc;

static int passes_of(int n, int wave) {   // the kernel's npass: observations n of the frame, wave of the team
  const int wr = n - wave * 64;
  return wr > 0 ? (wr + 255) / 256 : 0;
}
static long code(int wave, int pass, int rs, int lane) { return 1 + lane + 64L * (rs + 2L * (pass + 16L * wave)); }

int main() {
  long cases = 0, bad = 0;
  for (int n = 1; n <= 1100; ++n) {
    const int np0 = passes_of(n, 0);
    if (np0 > kPackMaxPasses) continue;
    const int slots = pack_chain_steps(np0) * kPackSlotsPerStep;
    std::vector<long> tile((size_t)slots, 0);
    long written = 0;
    for (int w = 0; w < 4; ++w)
      for (int p = 0; p < passes_of(n, w); ++p)
        for (int rs = 0; rs < 2; ++rs)
          for (int lane = 0; lane < 64; ++lane) {
            const int s = pack_write_slot(w, p, rs, lane);
            if (s < 0 || s >= slots || tile[(size_t)s] != 0) { ++bad; continue; }
            tile[(size_t)s] = code(w, p, rs, lane);
            ++written;
          }
    // 1. what the chain wave reads as valid: lane -> (chain, sub-row), steps below its chain's count
    std::vector<char> seen((size_t)slots, 0);
    long read = 0;
    for (int lane = 0; lane < 64; ++lane) {
      const int ch = pack_read_chain(lane);
      const int mine = ch < kPackChains ? pack_chain_steps(passes_of(n, ch >> 1)) : 0;
      for (int s = 0; s < pack_chain_steps(np0); ++s) {
        if (s >= mine) continue;   // (the kernel supplies zero)
        const int at = pack_read_slot(s, lane);
        if (at != pack_slot(s, lane >> 4, ch) || at < 0 || at >= slots || seen[(size_t)at] || tile[(size_t)at] == 0) { ++bad; continue; }
        seen[(size_t)at] = 1;
        ++read;
      }
    }
    if (read != written) ++bad;
    // 2. the order of gram_products
    for (int w = 0; w < 4; ++w)
      for (int a = 0; a < 2; ++a) {
        int step = 0;
        for (int p = 0; p < passes_of(n, w); ++p)
          for (int rs = 0; rs < 2; ++rs)
            for (int m = a; m < 16; m += 2) {
              for (int k = 0; k < 4; ++k)
                if (tile[(size_t)pack_slot(step, k, 2 * w + a)] != code(w, p, rs, 4 * m + k)) ++bad;
              ++step;
            }
        if (step != pack_chain_steps(passes_of(n, w))) ++bad;
      }
    ++cases;
  }
  // 3. row (lane >> 4) + 4 reg, column lane & 15 of the accumulator (the epilogue's layout of acc0 / acc1)
  for (int c = 0; c < kPackChains; ++c) {
    const int lane = pack_diag_lane(c), reg = pack_diag_reg(c);
    if (lane < 0 || lane >= 64 || reg < 0 || reg >= 4 || (lane >> 4) + 4 * reg != c || (lane & 15) != c) ++bad;
  }
  printf("%ld frames, %ld mismatches\n", cases, bad);
  return bad != 0;
}
