// cc_intr_start_batch_tables.hpp -- the workgroup tables of the batched fisheye focal-length start (cc_intr_start_batch.hpp),
// written once: cc_intr_start_batch_host.hpp uploads them, tests/cpp/intr_start_batch_tables.cpp compiles them on the host and
// checks them. No HIP dependency.
//
//   searched      [B + 1] prefix sums of S_p, the searched views of problem p: F_p when search_views is 0 or >= F_p, else
//                 search_views -- local searched view k of problem p is its view floor(k F_p / S_p)
//   search_where  [Stot] search workgroup -> {problem, k}, problems in order and k ascending within each (as `where` maps the
//                 sweep's workgroups to frames)
//   extent        extent workgroup -> {first observation, one past the last, problem}: the observations of problem p cut into
//                 runs of at most kIntrStartExtentChunk. A workgroup never holds observations of two problems, so its one
//                 atomic per word lands on its problem's words; a problem without observations has no workgroup.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace cc {

constexpr int64_t kIntrStartExtentChunk = 1024;   // observations of one extent workgroup: four a thread

struct IntrStartExtentWg {
  int64_t begin, end;   // observations [begin, end) of the concatenated uv
  int32_t problem, pad_;
};

struct IntrStartBatchTables {
  std::vector<int64_t> searched;
  std::vector<int32_t> search_where;   // pairs
  std::vector<IntrStartExtentWg> extent;
};

inline int64_t intr_start_batch_searched(int64_t F, int64_t search_views) {
  return search_views <= 0 || search_views >= F ? F : search_views;
}

// problem_offsets [B + 1] into frames, frame_offsets [Ftot + 1] into observations, both checked by the caller (batch_build_tables)
inline void intr_start_batch_tables(int64_t B, const int64_t* problem_offsets, const int64_t* frame_offsets, int64_t search_views,
                                    IntrStartBatchTables* out) {
  out->searched.assign((size_t)B + 1, 0);
  out->search_where.clear();
  out->extent.clear();
  for (int64_t p = 0; p < B; ++p) {
    const int64_t f0 = problem_offsets[p], F = problem_offsets[p + 1] - f0;
    const int64_t S = intr_start_batch_searched(F, search_views);
    out->searched[(size_t)p + 1] = out->searched[(size_t)p] + S;
    for (int64_t k = 0; k < S; ++k) {
      out->search_where.push_back((int32_t)p);
      out->search_where.push_back((int32_t)k);
    }
    const int64_t n0 = frame_offsets[f0], n1 = frame_offsets[f0 + F];
    for (int64_t at = n0; at < n1; at += kIntrStartExtentChunk) {
      const int64_t end = at + kIntrStartExtentChunk < n1 ? at + kIntrStartExtentChunk : n1;
      out->extent.push_back(IntrStartExtentWg{at, end, (int32_t)p, 0});
    }
  }
}

}  // namespace cc
