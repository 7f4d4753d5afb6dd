// cc_persist_publish.hpp -- how k_intr_persist hands the control block of a finished solve to the host (cc_intrinsics_persist.hip
// stores, cc_solve_host.hpp waits), written once: the kernel and the host call these pieces, tests/cpp/persist_publish_words.cpp
// compiles them with the host compiler. No HIP dependency.
//
// The seam idiom of cc_persist_dev.hpp, towards the host: the kPubDoubles 8-byte words of the block travel as 2 kPubDoubles
// self-validating words {tag32 : half}, tag = the solve's sequence number (publish_tag). An aligned 8-byte store is single-copy
// atomic, so a word that carries the expected tag IS that solve's half: the stores need no order among themselves, no release in
// front of them and no flag behind them, and the block is there when every word carries the tag.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define CC_PPUB_FN __host__ __device__ __forceinline__
#else
#define CC_PPUB_FN inline
#endif

namespace cc {

constexpr int kPubDoubles = 18;              // 8-byte words of the control block (LmCtl: asserted where both are known)
constexpr int kPubWords = 2 * kPubDoubles;   // tagged words
constexpr int kPubTaggedAt = 64;             // first tagged word, in 8-byte words from the start of the handle's pinned block

// The tag of sequence number seq >= 1: its low 32 bits, except that the tags skip 0 where the low bits wrap (0xffffffff is followed
// by 1) -- a block of zeros (a fresh handle's) never carries the tag of a solve.
CC_PPUB_FN uint32_t publish_tag(unsigned long long seq) { return (uint32_t)((seq - 1ull) % 0xffffffffull) + 1u; }

// half h (0: low, 1: high) of the 8-byte word `bits`
CC_PPUB_FN uint32_t publish_half(unsigned long long bits, int h) { return (uint32_t)(h ? bits >> 32 : bits); }

CC_PPUB_FN unsigned long long publish_word(uint32_t tag, uint32_t half) { return ((unsigned long long)tag << 32) | half; }

// tagged[0..kPubWords): word 2 i carries the low half of block word i, word 2 i + 1 the high half
CC_PPUB_FN void publish_pack(uint32_t tag, const unsigned long long* block, unsigned long long* tagged) {
  for (int i = 0; i < kPubWords; ++i) tagged[i] = publish_word(tag, publish_half(block[i >> 1], i & 1));
}

// does every word of tagged[0..kPubWords) -- a COPY the caller has taken word by word -- carry `tag`?
CC_PPUB_FN bool publish_ready(const unsigned long long* tagged, uint32_t tag) {
  for (int i = 0; i < kPubWords; ++i)
    if ((uint32_t)(tagged[i] >> 32) != tag) return false;
  return true;
}

CC_PPUB_FN void publish_unpack(const unsigned long long* tagged, unsigned long long* block) {
  for (int i = 0; i < kPubDoubles; ++i) block[i] = (tagged[2 * i + 1] << 32) | (tagged[2 * i] & 0xffffffffull);
}

}  // namespace cc
