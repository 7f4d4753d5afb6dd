// Stand-alone driver for the HOST code of cc_intrinsics_batch.hip (argument checks, offset tables, state packing), built with
// AddressSanitizer + UndefinedBehaviorSanitizer by run.sh. It needs no GPU: every path it walks ends before the first kernel.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/cc_solver.h"

namespace cc {
int batch_build_tables(const char* who, int64_t B, const int64_t* problem_offsets, const int64_t* frame_offsets,
                       std::vector<int32_t>* first, std::vector<int32_t>* where);
void batch_pack_state(int64_t B, int64_t Ftot, const double* intr9, const double* q, const double* t, double* intr_out, double* pose_out);
}

static int failures = 0;
#define EXPECT(cond)                                                                  \
  do {                                                                                \
    if (!(cond)) { std::printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, cc_last_error()); ++failures; } \
  } while (0)

int main() {
  // a ragged batch in exactly-sized heap arrays: 3 problems of 3, 1 and 4 frames
  const std::vector<int64_t> poff = {0, 3, 4, 8};
  const std::vector<int64_t> foff = {0, 4, 9, 13, 20, 24, 28, 33, 37};
  const int64_t B = 3, F = 8, N = 37;
  std::vector<float> uv((size_t)N * 2, 1.0f), xyz((size_t)N * 3, 2.0f);
  std::vector<int32_t> first, where;
  EXPECT(cc::batch_build_tables("test", B, poff.data(), foff.data(), &first, &where) == CC_OK);
  EXPECT(first.size() == 4 && where.size() == 16);
  EXPECT(first[0] == 0 && first[1] == 3 && first[2] == 4 && first[3] == 8);
  const int want[16] = {0, 0, 0, 1, 0, 2, 1, 0, 2, 0, 2, 1, 2, 2, 2, 3};
  for (int i = 0; i < 16; ++i) EXPECT(where[(size_t)i] == want[i]);

  std::vector<double> intr9((size_t)B * 9), q((size_t)F * 4), t((size_t)F * 3), intr_out((size_t)B * 32), pose_out((size_t)F * 8);
  for (size_t i = 0; i < intr9.size(); ++i) intr9[i] = 100.0 + (double)i;
  for (size_t i = 0; i < q.size(); ++i) q[i] = 0.5 + (double)i;
  for (size_t i = 0; i < t.size(); ++i) t[i] = -1.0 - (double)i;
  cc::batch_pack_state(B, F, intr9.data(), q.data(), t.data(), intr_out.data(), pose_out.data());
  for (int64_t p = 0; p < B; ++p)
    for (int i = 0; i < 16; ++i) {
      const double w = i < 9 ? intr9[(size_t)(p * 9 + i)] : 0.0;
      EXPECT(intr_out[(size_t)(p * 32 + i)] == w && intr_out[(size_t)(p * 32 + 16 + i)] == w);
    }
  for (int64_t f = 0; f < F; ++f) {
    for (int i = 0; i < 4; ++i) EXPECT(pose_out[(size_t)(f * 8 + i)] == q[(size_t)(f * 4 + i)]);
    for (int i = 0; i < 3; ++i) EXPECT(pose_out[(size_t)(f * 8 + 4 + i)] == t[(size_t)(f * 3 + i)]);
    EXPECT(pose_out[(size_t)(f * 8 + 7)] == 0.0);
  }

  // the bad-argument paths of the three entry points that take a batch's arrays
  cc_intrinsics_batch* h = nullptr;
  const std::vector<int64_t> poff_empty = {0, 3, 3, 8}, poff_down = {0, 5, 4, 8}, poff_late = {1, 3, 4, 8};
  const std::vector<int64_t> foff_down = {0, 4, 9, 8, 20, 24, 28, 33, 37}, foff_late = {1, 4, 9, 13, 20, 24, 28, 33, 37};
  std::vector<cc_summary> ss((size_t)B);
  for (auto& s : ss) { s.log = nullptr; s.log_capacity = 0; }
  struct Case { int64_t B; const int64_t* poff; const int64_t* foff; const float* uv; const float* xyz; };
  const Case bad[] = {
      {0, poff.data(), foff.data(), uv.data(), xyz.data()},      {-2, poff.data(), foff.data(), uv.data(), xyz.data()},
      {B, poff_empty.data(), foff.data(), uv.data(), xyz.data()}, {B, poff_down.data(), foff.data(), uv.data(), xyz.data()},
      {B, poff_late.data(), foff.data(), uv.data(), xyz.data()},  {B, poff.data(), foff_down.data(), uv.data(), xyz.data()},
      {B, poff.data(), foff_late.data(), uv.data(), xyz.data()},  {B, nullptr, foff.data(), uv.data(), xyz.data()},
      {B, poff.data(), nullptr, uv.data(), xyz.data()},           {B, poff.data(), foff.data(), nullptr, xyz.data()},
      {B, poff.data(), foff.data(), uv.data(), nullptr},
  };
  for (const Case& c : bad) {
    EXPECT(cc_intrinsics_batch_create(0, c.B, c.poff, c.foff, c.uv, c.xyz, &h) == CC_ERR_BAD_ARGUMENT && h == nullptr);
    EXPECT(cc_intrinsics_batch_optimize(nullptr, 0, c.B, c.poff, c.foff, c.uv, c.xyz, intr9.data(), nullptr, q.data(), t.data(), ss.data()) == CC_ERR_BAD_ARGUMENT);
    EXPECT(cc_intrinsics_batch_estimate(nullptr, 0, c.B, c.poff, c.foff, c.uv, c.xyz, nullptr, nullptr, nullptr, intr9.data(), q.data(), t.data(), ss.data()) == CC_ERR_BAD_ARGUMENT);
  }
  EXPECT(cc_intrinsics_batch_create(0, B, poff.data(), foff.data(), uv.data(), xyz.data(), nullptr) == CC_ERR_BAD_ARGUMENT);
  EXPECT(cc_intrinsics_batch_optimize(nullptr, 0, B, poff.data(), foff.data(), uv.data(), xyz.data(), nullptr, nullptr, q.data(), t.data(), nullptr) == CC_ERR_BAD_ARGUMENT);
  // Zhang's preconditions: problem 1 has a single frame
  EXPECT(cc_intrinsics_batch_estimate(nullptr, 0, B, poff.data(), foff.data(), uv.data(), xyz.data(), nullptr, nullptr, nullptr, intr9.data(), q.data(), t.data(), nullptr) == CC_ERR_BAD_ARGUMENT);
  EXPECT(cc_intrinsics_batch_set_state(nullptr, intr9.data(), nullptr, q.data(), t.data()) == CC_ERR_BAD_ARGUMENT);
  EXPECT(cc_intrinsics_batch_get_state(nullptr, nullptr, nullptr, nullptr) == CC_ERR_BAD_ARGUMENT);
  EXPECT(cc_intrinsics_batch_solve(nullptr, nullptr, nullptr) == CC_ERR_BAD_ARGUMENT);
  cc_intrinsics_batch_destroy(nullptr);
  // valid arguments: the tables are built, then the device is asked for (none here: CC_ERR_NO_DEVICE; with one, a handle)
  const int rc = cc_intrinsics_batch_create(0, B, poff.data(), foff.data(), uv.data(), xyz.data(), &h);
  EXPECT((rc == CC_ERR_NO_DEVICE && h == nullptr) || (rc == CC_OK && h != nullptr));
  cc_intrinsics_batch_destroy(h);
  std::printf(failures ? "%d check(s) failed\n" : "sanitize_intr_batch: all checks passed (create with valid arguments -> %d)\n", failures ? failures : rc);
  return failures ? 1 : 0;
}
