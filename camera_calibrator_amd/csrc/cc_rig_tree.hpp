// cc_rig_tree.hpp -- stage T of the rig start (cc_rig_estimate_start): the spanning tree over the cameras along which the
// camera poses are composed. Host code only, no HIP in it: cc_rig.hip calls it between the view kernel and the pose kernels,
// tests/cpp/rig_start_tree.cpp compiles it on its own.
//
// Input: the C x C table of co-visible VALID views -- covis[a * C + b] = frames in which cameras a and b both have a valid
// view, covis[a * C + a] = valid views of camera a -- and the caller's freeze flags. A camera is OBSERVED when it has a valid view.
//   root    among observed frozen cameras the one with the most valid views; if no frozen camera is observed, the observed
//           camera with the most valid views, which is then placed at the identity
//   frozen  cameras are placed at the pose the caller gave and never estimated (they may be parents)
//   then    repeatedly the (unplaced camera, placed camera) pair with the most co-visible frames is taken: the unplaced
//           camera is placed with the placed one as its parent
//   ties    go to the lowest index everywhere (of the unplaced camera first, then of the parent)
// Cameras without a path to a placed camera stay unplaced: they keep the caller's pose.
#pragma once
#include <cstdint>
#include <vector>

namespace cc {

struct RigStartTree {
  int32_t root = -1;                  // -1: no camera is observed
  bool root_at_identity = false;      // the root is not frozen: it defines the rig frame
  std::vector<int32_t> parent;        // [C] parent of an estimated camera, -1: root, frozen or unplaced
  std::vector<uint8_t> placed;        // [C] root, frozen or reached
  std::vector<int32_t> order;         // estimated cameras in the order they were placed (parents before children)
  int32_t n_placed = 0, n_unplaced = 0;
};

inline RigStartTree rig_start_tree(int C, const int64_t* covis, const uint8_t* frozen) {
  RigStartTree t;
  t.parent.assign((size_t)C, -1);
  t.placed.assign((size_t)C, 0);
  int64_t best = 0;
  for (int pass = 0; pass < 2 && t.root < 0; ++pass)   // pass 0: frozen cameras only
    for (int c = 0; c < C; ++c) {
      if (pass == 0 && !(frozen && frozen[c])) continue;
      const int64_t n = covis[(size_t)c * C + c];
      if (n > best) { best = n; t.root = c; }
    }
  if (t.root >= 0) {
    t.root_at_identity = !(frozen && frozen[t.root]);
    t.placed[(size_t)t.root] = 1;
  }
  for (int c = 0; c < C; ++c) if (frozen && frozen[c]) t.placed[(size_t)c] = 1;
  for (;;) {
    int bu = -1, bp = -1;
    int64_t bn = 0;
    for (int u = 0; u < C; ++u) {
      if (t.placed[(size_t)u]) continue;
      for (int p = 0; p < C; ++p) {
        if (!t.placed[(size_t)p]) continue;
        const int64_t n = covis[(size_t)u * C + p];
        if (n > bn) { bn = n; bu = u; bp = p; }
      }
    }
    if (bu < 0) break;
    t.placed[(size_t)bu] = 1;
    t.parent[(size_t)bu] = bp;
    t.order.push_back(bu);
  }
  for (int c = 0; c < C; ++c) (t.placed[(size_t)c] ? t.n_placed : t.n_unplaced) += 1;
  return t;
}

}  // namespace cc
