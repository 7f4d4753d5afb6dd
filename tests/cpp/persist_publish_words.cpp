// The tagged publication of k_intr_persist (csrc/cc_persist_publish.hpp), compiled with the host compiler: pack / validate / unpack
// as the kernel and the host's wait call them. Prints "N checks, 0 failures"; exit status 1 on any failure.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "cc_persist_publish.hpp"

using cc::kPubDoubles;
using cc::kPubWords;
typedef unsigned long long u64;

static long checks = 0, failures = 0;
#define CHECK(cond) do { ++checks; if (!(cond)) { ++failures; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } } while (0)

static u64 bits_of(double v) { u64 b; std::memcpy(&b, &v, 8); return b; }

// the block as the kernel's lanes store it: lane l takes 32-bit word l of the block
static void pack_like_the_kernel(uint32_t tag, const u64* block, u64* tagged) {
  uint32_t halves[kPubWords];
  std::memcpy(halves, block, sizeof(halves));
  for (int l = 0; l < kPubWords; ++l) tagged[l] = cc::publish_word(tag, halves[l]);
}

int main() {
  static_assert(kPubWords == 36 && kPubDoubles == 18, "18 doubles, 36 words");
  // ---- every class of bit pattern a double can hold goes through unchanged, in every position of the block
  const u64 patterns[] = {
      bits_of(0.0), bits_of(-0.0), bits_of(1.0), bits_of(-1.0), bits_of(0.1), bits_of(-123456.789e200),
      bits_of(std::numeric_limits<double>::denorm_min()), bits_of(-std::numeric_limits<double>::denorm_min()), 0x000fffffffffffffull /* largest subnormal */,
      bits_of(std::numeric_limits<double>::min()), bits_of(std::numeric_limits<double>::max()), bits_of(std::numeric_limits<double>::infinity()),
      bits_of(-std::numeric_limits<double>::infinity()), 0x7ff8000000000000ull /* quiet NaN */, 0xfff8000000000000ull, 0x7ff0000000000001ull /* signalling, payload 1 */,
      0x7ff4000000000000ull, 0xfff7ffffffffffffull, 0x7fffffffffffffffull /* all payload bits */, 0x7ff80000deadbeefull, 0xffffffffffffffffull,
      0x00000000ffffffffull, 0xffffffff00000000ull, 0x0000000100000000ull, 0x0000000400000003ull /* two int32 fields */};
  const int np = (int)(sizeof(patterns) / sizeof(patterns[0]));
  const uint32_t tags[] = {1u, 2u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
  for (uint32_t tag : tags) {
    for (int shift = 0; shift < np; ++shift) {
      u64 block[kPubDoubles], tagged[kPubWords], tagged2[kPubWords], out[kPubDoubles];
      for (int i = 0; i < kPubDoubles; ++i) block[i] = patterns[(i + shift) % np];
      cc::publish_pack(tag, block, tagged);
      pack_like_the_kernel(tag, block, tagged2);
      CHECK(std::memcmp(tagged, tagged2, sizeof(tagged)) == 0);
      CHECK(cc::publish_ready(tagged, tag));
      cc::publish_unpack(tagged, out);
      CHECK(std::memcmp(block, out, sizeof(block)) == 0);
      // a tag is a tag: no other one validates the block
      CHECK(!cc::publish_ready(tagged, tag + 1u));
      CHECK(!cc::publish_ready(tagged, tag - 1u));
    }
  }
  // ---- a block in which any ONE word still carries the previous solve's tag is not ready; nor is a block of all-older tags
  for (u64 seq : {2ull, 77ull, 0xffffffffull, 0x100000000ull, 0x100000001ull}) {
    const uint32_t now = cc::publish_tag(seq), before = cc::publish_tag(seq - 1);
    CHECK(now != before);
    u64 block[kPubDoubles], older[kPubDoubles], tagged[kPubWords], old_tagged[kPubWords];
    for (int i = 0; i < kPubDoubles; ++i) { block[i] = patterns[i % np]; older[i] = patterns[(i + 5) % np]; }
    cc::publish_pack(now, block, tagged);
    cc::publish_pack(before, older, old_tagged);
    CHECK(!cc::publish_ready(old_tagged, now));
    for (int stale = 0; stale < kPubWords; ++stale) {
      u64 mixed[kPubWords];
      std::memcpy(mixed, tagged, sizeof(mixed));
      mixed[stale] = old_tagged[stale];
      CHECK(!cc::publish_ready(mixed, now));
      // ... and the other way round: the new solve's words arriving one by one into the old block
      std::memcpy(mixed, old_tagged, sizeof(mixed));
      mixed[stale] = tagged[stale];
      CHECK(!cc::publish_ready(mixed, now));
    }
    // even when the old payload's halves happen to equal the new tag
    u64 trap[kPubDoubles], trap_tagged[kPubWords];
    for (int i = 0; i < kPubDoubles; ++i) trap[i] = ((u64)now << 32) | now;
    cc::publish_pack(before, trap, trap_tagged);
    CHECK(!cc::publish_ready(trap_tagged, now));
  }
  // ---- the tags: the low 32 bits of the sequence number; where those wrap, 0xffffffff is followed by 1 -- a zeroed block (a fresh
  // handle's; sequence numbers start at 1) never satisfies a wait
  CHECK(cc::publish_tag(1ull) == 1u);
  CHECK(cc::publish_tag(2ull) == 2u);
  CHECK(cc::publish_tag(0x12345678ull) == 0x12345678u);
  CHECK(cc::publish_tag(0xfffffffeull) == 0xfffffffeu);
  CHECK(cc::publish_tag(0xffffffffull) == 0xffffffffu);
  CHECK(cc::publish_tag(0x100000000ull) == 1u);
  CHECK(cc::publish_tag(0x100000001ull) == 2u);
  u64 zeros[kPubWords];
  std::memset(zeros, 0, sizeof(zeros));
  for (u64 seq = 0xfffffff0ull; seq <= 0x100000010ull; ++seq) {
    const uint32_t t = cc::publish_tag(seq);
    CHECK(t != 0u);
    CHECK(!cc::publish_ready(zeros, t));
    CHECK(cc::publish_tag(seq + 1) != t);
  }
  for (u64 seq : {1ull, 2ull, 0x1ffffffffull, 0x200000000ull, 0xfffffffffffffffeull}) CHECK(cc::publish_tag(seq) != 0u && !cc::publish_ready(zeros, cc::publish_tag(seq)));
  // (and a block zeroed AFTER a publication -- a recycled pinned block -- is not ready for the tag it carried)
  {
    u64 block[kPubDoubles], tagged[kPubWords];
    for (int i = 0; i < kPubDoubles; ++i) block[i] = patterns[i % np];
    cc::publish_pack(cc::publish_tag(1ull), block, tagged);
    CHECK(cc::publish_ready(tagged, cc::publish_tag(1ull)));
    std::memset(tagged, 0, sizeof(tagged));
    CHECK(!cc::publish_ready(tagged, cc::publish_tag(1ull)));
  }
  std::printf("%ld checks, %ld failures\n", checks, failures);
  return failures ? 1 : 0;
}
