// The order of the elimination-row sums of k_intr_persist, on the host (tests/test_persist_sum_order_cpu.py builds and runs this).
// csrc/cc_persist_sum.hpp holds the order as the pieces the kernel's column owners call; here they are composed as the kernel
// composes them and compared, as raw bits, with a literal transcription of the two-level gather the order comes from: a leader
// workgroup's gather_rows<80, NG, BATCH> over its (at most) sixteen rows, then the control's gather_rows over the leaders' rows.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "cc_persist_sum.hpp"

namespace {

constexpr int NC = 80;           // columns of an elimination row
constexpr int kLeaderRows = 16;  // rows a leader added up

// gather_rows<NC, NG, BATCH> without its waits: thread -> (column, row group), rows grp, grp + NG, ... BATCH at a time,
// the NG group sums through s_part, added in group order
template <int NG, int BATCH>
void gather_rows_ref(const double* box, int G, int ncols, int maxcol, double* out) {
  std::vector<double> s_part(NG * NC, 0.0);
  for (int tid = 0; tid < NG * NC; ++tid) {
    const int col = tid % NC, grp = tid / NC;
    if (grp < NG && col < ncols) {
      double acc = 0.0;
      for (int r0 = grp; r0 < G; r0 += BATCH * NG) {
        double v_[BATCH];
        for (int u = 0; u < BATCH; ++u) {
          const int r = r0 + u * NG;
          v_[u] = box[(size_t)(r < G ? r : r0) * NC + col];
        }
        for (int u = 0; u < BATCH; ++u) {
          if (r0 + u * NG < G) {
            const double v = v_[u];
            acc = col == maxcol ? fmax(acc, v) : acc + v;
          }
        }
      }
      s_part[grp * NC + col] = acc;
    }
  }
  for (int tid = 0; tid < ncols; ++tid) {
    double a = 0.0;
    if (tid == maxcol) { for (int g = 0; g < NG; ++g) a = fmax(a, s_part[g * NC + tid]); }
    else { for (int g = 0; g < NG; ++g) a += s_part[g * NC + tid]; }
    out[tid] = a;
  }
}

// the two levels: every sixteenth worker is a leader and adds its sixteen rows, the control adds the leaders' rows
template <int NG>
void two_level_ref(const std::vector<double>& rows, int G, int maxcol, double* out) {
  constexpr int BATCH = (kLeaderRows + NG - 1) / NG;
  const int nl = (G + kLeaderRows - 1) / kLeaderRows;
  std::vector<double> lbox((size_t)nl * NC);
  for (int g0 = 0; g0 < G; g0 += kLeaderRows) {
    const int n = G - g0 < kLeaderRows ? G - g0 : kLeaderRows;
    gather_rows_ref<NG, BATCH>(rows.data() + (size_t)g0 * NC, n, NC, maxcol, lbox.data() + (size_t)(g0 / kLeaderRows) * NC);
  }
  gather_rows_ref<NG, BATCH>(lbox.data(), nl, NC, maxcol, out);
}

// the kernel's composition: the owner of column c has the column's G values in a row, a lane per group forms the group's sum,
// one lane the total
template <int NG>
double owner_total(const double* col, int G, bool is_max) {
  // (the pieces read sixteen values whatever the group holds: in the kernel what lies behind a short group is the next column
  // or stale LDS -- here NaNs, which would show in every total if they were ever used)
  double L[cc::kPSumRows], grp[cc::kPSumRows];
  const int nL = cc::persist_sum_groups(G);
  for (int j = 0; j < cc::kPSumRows; ++j) L[j] = std::numeric_limits<double>::quiet_NaN();
  for (int j = 0; j < nL; ++j) {
    const int n = cc::persist_sum_group_rows(G, j);
    for (int r = 0; r < cc::kPSumRows; ++r) grp[r] = r < n ? col[j * cc::kPSumRows + r] : std::numeric_limits<double>::quiet_NaN();
    L[j] = cc::persist_sum_group<NG>(grp, n, is_max);
  }
  return cc::persist_sum_group<NG>(L, nL, is_max);
}

uint64_t bits(double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; }

template <int NG>
int check(int G, int maxcol, int fill, std::mt19937_64& rng) {
  std::vector<double> rows((size_t)G * NC);
  std::uniform_real_distribution<double> mant(-1.0, 1.0), dec(-15.0, 15.0);
  std::uniform_int_distribution<int> pick(0, 9);
  for (int r = 0; r < G; ++r) {
    for (int c = 0; c < NC; ++c) {
      double v = mant(rng) * std::pow(10.0, dec(rng));   // mixed signs, thirty decades
      if (fill == 1) {
        // exact cancellations and signed zeros: a value, its negative somewhere behind it, and -0.0
        const int k = pick(rng);
        if (k < 3 && r > 0) v = -rows[(size_t)(r - 1) * NC + c];
        else if (k == 3) v = -0.0;
        else if (k == 4) v = 0.0;
      } else if (fill == 2) {
        v = -0.0;   // every row -0.0: the sums start from +0.0
      }
      if (c == maxcol) {
        v = std::fabs(v);   // (the column of the pose gradients' maximum holds magnitudes)
        if (fill == 1 && pick(rng) == 0) v = std::numeric_limits<double>::quiet_NaN();
        if (fill == 3) v = std::numeric_limits<double>::quiet_NaN();   // nothing but NaN: fmax keeps 0.0
      }
      rows[(size_t)r * NC + c] = v;
    }
  }
  double want[NC];
  two_level_ref<NG>(rows, G, maxcol, want);
  int bad = 0;
  std::vector<double> col(G);
  for (int c = 0; c < NC; ++c) {
    for (int r = 0; r < G; ++r) col[r] = rows[(size_t)r * NC + c];
    const double got = owner_total<NG>(col.data(), G, c == maxcol);
    if (bits(got) != bits(want[c])) {
      if (!bad) std::printf("MISMATCH G=%d NG=%d fill=%d column %d: got %.17g (%016llx) want %.17g (%016llx)\n", G, NG, fill, c, got,
                            (unsigned long long)bits(got), want[c], (unsigned long long)bits(want[c]));
      ++bad;
    }
  }
  return bad;
}

}  // namespace

int main() {
  const int Gs[] = {1, 5, 10, 16, 17, 19, 37, 79, 80, 81, 203, 250, 256};
  const int maxcol = 73;   // PC_GMAXP
  std::mt19937_64 rng(20261019);
  int bad = 0, cases = 0;
  for (int G : Gs) {
    for (int fill = 0; fill < 4; ++fill) {
      for (int rep = 0; rep < (fill < 2 ? 4 : 1); ++rep) {
        bad += check<3>(G, maxcol, fill, rng);
        bad += check<6>(G, maxcol, fill, rng);
        bad += check<12>(G, maxcol, fill, rng);
        cases += 3;
      }
    }
  }
  std::printf("%d cases of 80 columns, %d mismatches\n", cases, bad);
  return bad ? 1 : 0;
}
