// cc_persist_sum.hpp -- the ORDER in which k_intr_persist adds the workers' elimination rows (cc_intrinsics_persist.hip),
// written once: the kernel's column owners call these pieces, tests/cpp/persist_sum_order.cpp compiles them on the host and
// compares them, bit for bit, with the two-level gather the order comes from. No HIP dependency.
//
// A column of G values (one per worker) is cut into groups of kPSumRows consecutive rows. A group's rows r = g, g + NG, ... are
// added in that order from +0.0 into NG partial sums, the NG partials -- the empty ones too -- are added in order from +0.0:
// that is the group's sum L[j]. The ceil(G / kPSumRows) <= kPSumRows group sums are added by the SAME rule: the column's total.
// NG = threads of a workgroup / kPartialCols (12 / 6 / 3 with four / two / one team). The column of the pose gradients' maximum
// takes fmax in the place of every addition, from 0.0 (a NaN counts as missing).
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define CC_PSUM_FN __host__ __device__ __forceinline__
#else
#define CC_PSUM_FN inline
#endif

namespace cc {

constexpr int kPSumRows = 16;   // rows of a group

CC_PSUM_FN int persist_sum_groups(int G) { return (G + kPSumRows - 1) / kPSumRows; }
CC_PSUM_FN int persist_sum_group_rows(int G, int j) { return G - j * kPSumRows < kPSumRows ? G - j * kPSumRows : kPSumRows; }

// the sum (IS_MAX: maximum) of v[0..n), 1 <= n <= kPSumRows, in the order above. v[n..kPSumRows) must be READABLE (whatever it
// holds). Straight-line: all sixteen values are read at once (on the GPU they come out of LDS: sixteen reads in flight, not a
// round trip per addition) and a row beyond n is replaced by +0.0 where it is read instead of being skipped where it would be
// added -- the same bits: a partial that starts from +0.0 is never -0.0 (in round-to-nearest x + y is -0.0 only when both are), and
// a + (+0.0) is a for every other a; a maximum that starts from 0.0 is never negative and never a NaN, and fmax(a, +0.0) is a.
template <int NG, bool IS_MAX>
CC_PSUM_FN double persist_sum_group_of(const double* v, int n) {
  constexpr int kPer = (kPSumRows + NG - 1) / NG;   // rows of a partial sum, at most
  double x[kPSumRows];
#pragma unroll
  for (int r = 0; r < kPSumRows; ++r) x[r] = v[r];
#pragma unroll
  for (int r = 0; r < kPSumRows; ++r) x[r] = r < n ? x[r] : 0.0;
  double total = 0.0;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    double a = 0.0;
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int r = g + u * NG;
      if (r < kPSumRows) a = IS_MAX ? fmax(a, x[r]) : a + x[r];
    }
    total = IS_MAX ? fmax(total, a) : total + a;
  }
  return total;
}

template <int NG>
CC_PSUM_FN double persist_sum_group(const double* v, int n, bool is_max) {
  return is_max ? persist_sum_group_of<NG, true>(v, n) : persist_sum_group_of<NG, false>(v, n);
}

}  // namespace cc
