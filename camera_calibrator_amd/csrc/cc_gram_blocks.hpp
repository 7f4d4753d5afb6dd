// cc_gram_blocks.hpp -- the index map of the Gram product on ten of the sixteen 4 x 4 blocks of a 16 x 16 block, one of each
// transposed pair, written once: the device code calls these pieces (gram_blocks_ahead, cc_device.hpp;
// scripts/mfma_probe/probe_gram_bits.hip), tests/cpp/gram_blocks_map.cpp compiles them on the host and checks the map against
// gram_products' order. No HIP dependency.
//
// gram_products forms the block of a staged tile (64 rows of 16 components) in two chains of 16 x 16 x 4 products with A = B:
// product m consumes rows 4m .. 4m + 3 and adds into accumulator m & 1. Each product writes 256 entries of a symmetric block that
// has 136 distinct ones. v_mfma_f64_4x4x4_4b_f64 multiplies four independent 4 x 4 x 4 blocks per instruction
//   A, B: lane k << 4 | slot << 2 | i        D: lane i << 4 | slot << 2 | j        (scripts/mfma_probe/probe4x4.hip)
// and output block s is ALWAYS A block s times B block s: on gfx950 the A-broadcast modifiers cbsz / abid change nothing for this
// instruction (probe4x4, profiles/r23/probe4x4.txt), so every block wants its two operand blocks in its own slot.
// Write g0 .. g3 for the component groups (4g .. 4g + 3) and take the row sets in PAIRS: set 2p feeds chain 0, set 2p + 1
// chain 1, as today. Six operand reads and five products give one block of every transposed pair, for both chains, exactly once:
//   operand  slot 0   slot 1   slot 2   slot 3          (a0, a1: the operand registers of gram_operands, read as four blocks)
//   a0       s0 g0    s0 g1    s0 g2    s0 g3           s0 = row set 2p, s1 = row set 2p + 1
//   a1       s1 g0    s1 g1    s1 g2    s1 g3
//   r0       s0 g1    s0 g2    s0 g3    s0 g0           (a0 one block on)
//   r1       s1 g1    s1 g2    s1 g3    s1 g0
//   Z        s0 g0    s0 g1    s1 g0    s1 g1
//   X        s0 g2    s0 g3    s1 g2    s1 g3
//   product  A   B    blocks (row group, column group) in slots 0 .. 3
//   0        a0  a0   (0,0) (1,1) (2,2) (3,3) of chain 0
//   1        a1  a1   the same of chain 1
//   2        a0  r0   (0,1) (1,2) (2,3) (3,0) of chain 0
//   3        a1  r1   the same of chain 1
//   4        Z   X    (0,2) (1,3) of chain 0, (0,2) (1,3) of chain 1
// Entry (r, c) of a block is the sum over the staged rows of component r times component c, four rows per product in the order
// k = 0 .. 3, whichever instruction forms it (scripts/mfma_probe/probe_gram_bits.hip: the same bits as the 16 x 16 x 4 chain);
// (c, r) is the same chain of products of commuting factors, so the other block of a transposed pair is a copy.
#pragma once

#ifdef __HIPCC__
#define CC_GB_FN __host__ __device__ constexpr
#else
#define CC_GB_FN constexpr
#endif

namespace cc {

constexpr int kGbPairs = 8;      // pairs of row sets in a staged tile of 64 rows
constexpr int kGbPairRows = 8;   // staged rows of a pair: gb_op_row(o, pair, lane) = gb_op_row(o, 0, lane) + 8 pair
constexpr int kGbOperands = 6;   // operand reads of a pair: a0, a1, r0, r1, Z, X
constexpr int kGbProducts = 5;   // products of a pair, one accumulator register each
enum { GB_A0 = 0, GB_A1 = 1, GB_R0 = 2, GB_R1 = 3, GB_Z = 4, GB_X = 5 };

CC_GB_FN int gb_slot(int lane) { return (lane >> 2) & 3; }

// ---- operands: block `slot` of operand `o` is component group gb_op_group of row set 2 pair + gb_op_set
CC_GB_FN int gb_op_set(int o, int slot) { return o <= GB_R1 ? (o & 1) : slot >> 1; }
CC_GB_FN int gb_op_group(int o, int slot) {
  return o <= GB_A1 ? slot : o <= GB_R1 ? ((slot + 1) & 3) : o == GB_Z ? (slot & 1) : 2 + (slot & 1);
}
// the staged row and the component that lane `lane` reads for operand `o` of pair `pair`
CC_GB_FN int gb_op_row(int o, int pair, int lane) { return 4 * (2 * pair + gb_op_set(o, gb_slot(lane))) + (lane >> 4); }
CC_GB_FN int gb_op_comp(int o, int lane) { return 4 * gb_op_group(o, gb_slot(lane)) + (lane & 3); }

// ---- products: operands of product n (no modifiers: output block s = A block s x B block s)
CC_GB_FN int gb_prod_a(int n) { return n == 0 || n == 2 ? GB_A0 : n == 1 || n == 3 ? GB_A1 : GB_Z; }
CC_GB_FN int gb_prod_b(int n) { return n == 0 ? GB_A0 : n == 1 ? GB_A1 : n == 2 ? GB_R0 : n == 3 ? GB_R1 : GB_X; }

// ---- accumulators: lane `lane` of accumulator n holds entry (row, column) of chain gb_acc_chain
CC_GB_FN int gb_acc_chain(int n, int lane) { return gb_op_set(gb_prod_b(n), gb_slot(lane)); }
CC_GB_FN int gb_acc_row(int n, int lane) { return 4 * gb_op_group(gb_prod_a(n), gb_slot(lane)) + (lane >> 4); }
CC_GB_FN int gb_acc_col(int n, int lane) { return 4 * gb_op_group(gb_prod_b(n), gb_slot(lane)) + (lane & 3); }

// ---- entries: (accumulator, lane) that holds entry (r, c) of chain `chain`, or -- gb_entry_held false -- its transposed twin
// (c, r). Entries inside a diagonal block are held in both orders.
CC_GB_FN int gb_entry_src(int chain, int r, int c) {
  for (int n = 0; n < kGbProducts; ++n)
    for (int lane = 0; lane < 64; ++lane)
      if (gb_acc_chain(n, lane) == chain && gb_acc_row(n, lane) == r && gb_acc_col(n, lane) == c) return n * 64 + lane;
  return -1;
}
CC_GB_FN bool gb_entry_held(int chain, int r, int c) { return gb_entry_src(chain, r, c) >= 0; }
CC_GB_FN int gb_entry_acc(int chain, int r, int c) { return (gb_entry_held(chain, r, c) ? gb_entry_src(chain, r, c) : gb_entry_src(chain, c, r)) >> 6; }
CC_GB_FN int gb_entry_lane(int chain, int r, int c) { return (gb_entry_held(chain, r, c) ? gb_entry_src(chain, r, c) : gb_entry_src(chain, c, r)) & 63; }

// ---- reduction of a wave's two chains into its 16 x 16 block. Accumulators 0 and 1, and 2 and 3, hold the same entry of chain 0
// and of chain 1 in the same lane; accumulator 4 holds chain 0 in the lanes of slots 0, 1 and chain 1, of the same entry, eight
// lanes on (slots 2, 3), so that v + (v of lane ^ 8) is chain 0 + chain 1 in both. Stores: 0 + 1 entry (row, column) -- the
// diagonal blocks are whole; 2 + 3 entry (row, column) and its mirror (column, row); 4 entry (row, column) from the lanes of
// slots 0, 1 and the mirror from those of slots 2, 3.
CC_GB_FN int gb_partner_lane(int lane) { return lane ^ 8; }
CC_GB_FN bool gb_store_mirrored(int lane) { return gb_slot(lane) >= 2; }   // (accumulator 4)

}  // namespace cc
