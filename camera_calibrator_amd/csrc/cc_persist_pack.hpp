// cc_persist_pack.hpp -- the index map of k_intr_persist's residual-only sweep (cc_intrinsics_persist.hip), written once: the kernel
// calls these pieces, tests/cpp/persist_pack_map.cpp compiles them on the host and checks the map against the full sweep's order.
// No HIP dependency.
//
// The cost of a frame is half of entry (15, 15) of its Gram block. In the full sweep a wave builds it in TWO chains of 16 x 16 x 4
// matrix products (gram_products, cc_device.hpp): product m of a row set consumes the staged rows 4m .. 4m + 3 -- the residuals of
// lanes 4m .. 4m + 3 -- and adds the four squares into accumulator m & 1, the row sets (u, then v) of a pass and the passes in
// order. A team of four waves has eight such chains. Entry (i, i) of a product depends on operand row i alone, so ONE product can
// advance all eight: lane i + 16 k supplies, as both operands, the residual that is sub-row k of step s of chain i (zero for
// i >= 8 and for a step the chain's wave does not have: C + 0 * 0 keeps the bits of a non-negative sum). Entry (i, i) of the
// accumulator then holds, product for product, what entry (15, 15) of chain i's accumulator holds in the full sweep.
//   chain = 2 wave + (m & 1)            wave: of the team, 0..3;  m = lane >> 2: the product of the row set that takes the lane's row
//   step  = (2 pass + row set) 8 + (m >> 1)
//   k     = lane & 3                    sub-row of the product (the lane's row is 4 m + k)
// The residuals travel through the team's staging tiles: slot (step, k, chain) = 32 step + 8 k + chain, so that the chain wave's
// operand read of a step is one run of 32 doubles.
#pragma once

#ifdef __HIPCC__
#define CC_PPACK_FN __host__ __device__ __forceinline__
#else
#define CC_PPACK_FN inline
#endif

namespace cc {

constexpr int kPackChains = 8;       // chains of a team: two per wave
constexpr int kPackStepsPerPass = 16;   // steps a pass adds to each chain of its wave: two row sets of eight
constexpr int kPackSlotsPerStep = 32;   // doubles of a step in the tiles: four sub-rows of eight chains
constexpr int kPackMaxPasses = 8;    // passes (of 256 observations) whose residuals fit a team's four staging tiles (4096 doubles)

// ---- writer: lane `lane` of wave `wave` of the team, row set `rs` (0: u, 1: v) of pass `pass`
CC_PPACK_FN int pack_chain(int wave, int lane) { return 2 * wave + ((lane >> 2) & 1); }
CC_PPACK_FN int pack_step(int pass, int rs, int lane) { return (2 * pass + rs) * 8 + (lane >> 3); }
CC_PPACK_FN int pack_sub(int lane) { return lane & 3; }
CC_PPACK_FN int pack_slot(int step, int k, int chain) { return step * kPackSlotsPerStep + k * kPackChains + chain; }
CC_PPACK_FN int pack_write_slot(int wave, int pass, int rs, int lane) {
  return pack_slot(pack_step(pass, rs, lane), pack_sub(lane), pack_chain(wave, lane));
}

// ---- reader: lane `lane` of the chain wave supplies sub-row lane >> 4 of chain lane & 15 (chains >= kPackChains: zero)
CC_PPACK_FN int pack_read_chain(int lane) { return lane & 15; }
CC_PPACK_FN int pack_read_slot(int step, int lane) { return pack_slot(step, lane >> 4, lane & (kPackChains - 1)); }
// steps of a chain whose wave makes `npass` passes; the team's product count is that of its wave 0
CC_PPACK_FN int pack_chain_steps(int npass) { return npass * kPackStepsPerPass; }

// ---- entry (i, i) of the 16 x 16 accumulator: lane and register (row (lane >> 4) + 4 reg, column lane & 15)
CC_PPACK_FN int pack_diag_lane(int chain) { return (chain & 3) * 16 + chain; }
CC_PPACK_FN int pack_diag_reg(int chain) { return chain >> 2; }

}  // namespace cc
