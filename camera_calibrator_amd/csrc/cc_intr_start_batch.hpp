#pragma once
#include "cc_intr_start.hpp"
#include "cc_intr_start_batch_tables.hpp"

// cc_intr_start_batch.hpp / cc_intr_start_batch.hip -- EXTENSION: the fisheye focal-length start (cc_intr_start.hpp)
// for every problem of a batch handle at once (cc_intrinsics_batch_estimate_start_fisheye): seven launches whatever
// the number of problems, one host wait behind them.
//   hipMemsetAsync         the boxes of all problems
//   k_intrb_start_extent   pass 0 / pass 1: one workgroup per run of observations of ONE problem (cc_intr_start_batch_tables.hpp),
//                          the bounding box and r_max under atomicMax on that problem's words; pass 2: one wave per problem, its
//                          centre, r_max and candidates
//   k_intrb_start_view     grid (searched views of all problems, candidates), one wave each: a table maps the workgroup to
//                          {problem, local searched view}; the wave's lines are k_intr_start_view's (cc_intr_start_view_body.hpp)
//   k_intrb_start_pick     one wave per problem, lane per candidate, a serial sum over the problem's searched views in index order
//   k_intrb_start_view     once more over all views of all problems (the handle's `where` maps them) at each problem's winner
// Problem p is an IntrStartDev of its own in a device table: the handle's concatenated off (from its first frame) / uv / xyz and
// its own slices of box, ext, f, score, qualified, best, srec, skind, view, kind. Every sum of a problem runs over its own data
// in an order fixed by its own indices; the only atomics are the integer maxima of the extent. A problem's bits do not depend
// on the batch it sits in, nor on where.

namespace cc {

struct IntrStartBatchDev {
  int32_t B, C;                       // problems; candidates (the same for every problem)
  int64_t Ftot, Stot, E;              // views, searched views and extent workgroups of all problems
  const IntrStartDev* prob;           // [B]
  const int2* search_where;           // [Stot] search workgroup -> {problem, local searched view}
  const int2* view_where;             // [Ftot] pose-pass workgroup -> {problem, local view}
  const IntrStartExtentWg* extent;    // [E]
  unsigned long long* box;            // [B][8]: problem p's box is prob[p].box = box + 8 p; zeroed before the launch
};

// Everything of one batched start on the stream, not waited for.
void intr_start_batch_enqueue(const IntrStartBatchDev& T, hipStream_t s, int refine_iterations);

}  // namespace cc
