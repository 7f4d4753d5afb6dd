// Stage T of the rig start on hand-made co-visibility tables: the product's host-only header (csrc/cc_rig_tree.hpp) compiled
// into a stand-alone program (tests/test_rig_start_tree_cpu.py builds it with -fsanitize=address,undefined). The tables and the
// expected roots and parents are those of tests/test_rig_start_ref_cpu.py (TREE_CASES), which runs the numpy reference on them.
#include <cstdio>
#include <vector>

#include "cc_rig_tree.hpp"

struct Case {
  const char* name;
  int C;
  std::vector<int64_t> covis;
  std::vector<uint8_t> frozen;
  int root, at_identity;
  std::vector<int32_t> parent;
  std::vector<int32_t> order;
};

int main() {
  const std::vector<Case> cases = {
      {"chain", 4, {9, 5, 0, 0, 5, 9, 4, 0, 0, 4, 9, 3, 0, 0, 3, 9}, {1, 0, 0, 0}, 0, 0, {-1, 0, 1, 2}, {1, 2, 3}},
      {"tie", 4, {6, 4, 0, 4, 4, 8, 2, 4, 0, 2, 8, 0, 4, 4, 0, 6}, {0, 0, 0, 0}, 1, 1, {1, -1, 1, 0}, {0, 3, 2}},
      {"disconnected", 5, {7, 3, 2, 0, 0, 3, 7, 0, 0, 0, 2, 0, 7, 0, 0, 0, 0, 0, 5, 0, 0, 0, 0, 0, 0}, {1, 0, 0, 0, 0}, 0, 0, {-1, 0, 0, -1, -1}, {1, 2}},
      {"two_frozen", 4, {5, 4, 1, 0, 4, 6, 2, 1, 1, 2, 8, 3, 0, 1, 3, 4}, {1, 0, 1, 0}, 2, 0, {-1, 0, -1, 2}, {1, 3}},
      {"nothing_observed", 3, {0, 0, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 0}, -1, 0, {-1, -1, -1}, {}},
  };
  int bad = 0;
  for (const Case& c : cases) {
    const cc::RigStartTree t = cc::rig_start_tree(c.C, c.covis.data(), c.frozen.data());
    bool ok = t.root == c.root && (int)t.root_at_identity == c.at_identity && t.parent == c.parent && t.order == c.order;
    int placed = 0;
    for (int k = 0; k < c.C; ++k) {
      const bool want = c.frozen[(size_t)k] || k == c.root || c.parent[(size_t)k] >= 0;
      ok = ok && (t.placed[(size_t)k] != 0) == want;
      placed += want;
    }
    ok = ok && t.n_placed == placed && t.n_unplaced == c.C - placed;
    std::printf("%s: root %d, %d placed, %d unplaced: %s\n", c.name, t.root, t.n_placed, t.n_unplaced, ok ? "ok" : "MISMATCH");
    bad += !ok;
  }
  // no freeze flags at all (NULL) is "none frozen"
  {
    const Case& c = cases[1];
    const cc::RigStartTree t = cc::rig_start_tree(c.C, c.covis.data(), nullptr);
    const bool ok = t.root == c.root && t.parent == c.parent;
    std::printf("tie, NULL flags: %s\n", ok ? "ok" : "MISMATCH");
    bad += !ok;
  }
  std::printf("%zu cases, %d mismatches\n", cases.size() + 1, bad);
  return bad ? 1 : 0;
}
