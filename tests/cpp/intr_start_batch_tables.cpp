// Host check of the workgroup tables of the batched fisheye focal-length start (csrc/cc_intr_start_batch_tables.hpp), compiled with
// g++ by tests/test_intr_batch_start_cpu.py. For each case: every (problem, searched view) appears exactly once and in order, the
// searched views are floor(k F_p / S_p), the prefix sums add up, and the extent workgroups tile each problem's observations in
// order without one of them spanning two problems or exceeding the chunk.
#include "cc_intr_start_batch_tables.hpp"

#include <cstdio>
#include <set>
#include <utility>

using namespace cc;

static int check(const char* name, const std::vector<int64_t>& views_per_problem, const std::vector<int64_t>& points_per_view, int64_t search_views) {
  const int64_t B = (int64_t)views_per_problem.size();
  std::vector<int64_t> poff(1, 0), foff(1, 0);
  size_t at = 0;
  for (int64_t p = 0; p < B; ++p) {
    for (int64_t v = 0; v < views_per_problem[(size_t)p]; ++v) foff.push_back(foff.back() + points_per_view[at++ % points_per_view.size()]);
    poff.push_back((int64_t)foff.size() - 1);
  }
  IntrStartBatchTables t;
  intr_start_batch_tables(B, poff.data(), foff.data(), search_views, &t);
  int bad = 0;
  auto expect = [&](bool ok, const char* what) { if (!ok) { ++bad; std::printf("%s: %s\n", name, what); } };
  expect((int64_t)t.searched.size() == B + 1 && t.searched[0] == 0, "prefix sums: size or start");
  expect((int64_t)t.search_where.size() == 2 * t.searched[(size_t)B], "search_where: size");
  std::set<std::pair<int64_t, int64_t>> seen;
  int64_t w = 0;
  for (int64_t p = 0; p < B; ++p) {
    const int64_t F = views_per_problem[(size_t)p];
    const int64_t S = search_views <= 0 || search_views >= F ? F : search_views;
    expect(t.searched[(size_t)p + 1] - t.searched[(size_t)p] == S, "searched views of a problem");
    int64_t last_view = -1;
    for (int64_t k = 0; k < S; ++k, ++w) {
      expect(w == t.searched[(size_t)p] + k, "workgroup index");
      expect(t.search_where[(size_t)w * 2] == p && t.search_where[(size_t)w * 2 + 1] == k, "{problem, k} out of order");
      const int64_t view = (k * F) / S;   // (what the view kernel makes of k)
      expect(view > last_view && view < F, "searched view");
      expect(seen.insert({p, view}).second, "a (problem, view) twice");
      last_view = view;
    }
  }
  expect((int64_t)seen.size() == t.searched[(size_t)B], "every (problem, searched view) once");
  // extent: in order, contiguous within a problem, inside it, never empty, never above the chunk
  size_t e = 0;
  for (int64_t p = 0; p < B; ++p) {
    const int64_t n0 = foff[(size_t)poff[(size_t)p]], n1 = foff[(size_t)poff[(size_t)p + 1]];
    int64_t cursor = n0;
    while (e < t.extent.size() && t.extent[e].problem == p) {
      const IntrStartExtentWg& g = t.extent[e];
      expect(g.begin == cursor && g.end > g.begin && g.end <= n1 && g.end - g.begin <= kIntrStartExtentChunk, "extent workgroup");
      cursor = g.end;
      ++e;
    }
    expect(cursor == n1, "a problem's observations are not covered");
  }
  expect(e == t.extent.size(), "extent workgroups out of problem order");
  std::printf("%s: %lld problems, %lld searched, %lld extent workgroups, %d mismatches\n", name, (long long)B, (long long)t.searched[(size_t)B],
              (long long)t.extent.size(), bad);
  return bad;
}

int main() {
  int bad = 0;
  const std::vector<int64_t> ragged_points = {4, 9, 25, 64, 65, 144, 0, 1030, 2048, 2049};
  for (int64_t S : {0, 5, 40}) {
    bad += check("one problem", {12}, {36}, S);
    bad += check("ragged", {6, 1, 12, 3, 41, 5, 40, 39}, ragged_points, S);
    bad += check("seventy of three", std::vector<int64_t>(70, 3), {9}, S);
  }
  std::printf("total: %d mismatches\n", bad);
  return bad != 0;
}
