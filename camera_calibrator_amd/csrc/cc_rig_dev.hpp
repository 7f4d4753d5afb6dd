// cc_rig_dev.hpp -- the helpers of the rig path that need nothing of its problem description (RigDev): index
// arithmetic, the depth reciprocal, the lane-swap / DPP reductions, the block sum, and the medium-size Cholesky with its
// backward substitution. Device code only; cc_rig.hip includes this ahead of cc_rig_sweeps.hpp / cc_rig_steps.hpp, and
// the primitive probe (tests/cpp/dev_probe.hip) includes it on its own.
#pragma once
#include "cc_device.hpp"

namespace cc {

__device__ __forceinline__ void untri(int idx, int& i, int& j) {  // packed lower index -> (i >= j)
  i = 0;
  while (tri(i + 1, 0) <= idx) ++i;
  j = idx - tri(i, 0);
}
// 1 / z for the depth of a point in front of the camera (z far from the ends of the exponent range): the hardware
// estimate and two Newton steps, five instructions instead of the twelve of the IEEE division sequence (scaling, fix-up).
// Not correctly rounded: within an ulp or two of 1 / z, so the adjoint sweeps (the default) are not bit-identical to
// the division form that k_rig_obs_cost and the oracle keep (parity is to the stated tolerances under either;
// the division form is kept as a variant, scripts/variants/exact_arith.patch). Degenerate depths: z = 0 (and z = +-inf) give NaN here (0 * inf inside
// the first fma) where the division gives +-inf / 0. Both are "not finite" to everything downstream -- the candidate
// cost fails isfinite() in lm_trial and counts as DBL_MAX, a Gram block holding either fails the Cholesky's
// `d > 0 && isfinite(d)` test -> invalid step -> the radius shrinks -- so a point that lands on the camera plane is
// rejected the same way in both forms; a select on the result would cost three instructions per observation of ~165.
// A point BEHIND the camera (z < 0) is an ordinary finite value in both.
__device__ __forceinline__ double recip_depth(double z) {
  double r = __builtin_amdgcn_rcp(z);
  r = fma(fma(-z, r, 1.0), r, r);
  r = fma(fma(-z, r, 1.0), r, r);
  return r;
}

// 32 per-lane values -> their 64-lane sums, value e left in lanes 2e and 2e + 1. Each exchange halves the values a lane
// carries (31 exchanges and adds instead of 32 x 6), and none of them goes through the LDS crossbar: the two widest
// are the lane-swap instructions of gfx950 (v_permlane32_swap: lanes 32..63 of the first register <-> lanes 0..31 of the
// second; v_permlane16_swap: odd 16-lane rows of the first <-> even rows of the second -- after either, first + second
// is the pairwise sum of the first register's values in the lower lanes / even rows and of the second's in the others),
// the rest DPP moves inside a row. Partner masks 32, 16, 8, 7 (half-row mirror), 2, 1 are independent, so every value
// collects all 64 lanes; the lane bit that picks the half kept in each step (5, 4, 3, 2, 1) differs between partners and
// all earlier ones agree.
template <int N>
__device__ __forceinline__ void reduce_swap32(double* p) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const auto l = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(p[i]), (unsigned)__double2loint(p[i + N]), false, false);
    const auto h = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(p[i]), (unsigned)__double2hiint(p[i + N]), false, false);
    p[i] = __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
  }
}
template <int N>
__device__ __forceinline__ void reduce_swap16(double* p) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const auto l = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(p[i]), (unsigned)__double2loint(p[i + N]), false, false);
    const auto h = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(p[i]), (unsigned)__double2hiint(p[i + N]), false, false);
    p[i] = __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
  }
}
template <int N, int CTRL, int BIT>
__device__ __forceinline__ void reduce_dpp(double* p, int lane) {
  const bool up = (lane & BIT) != 0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double lo = p[i], hi = p[i + N];
    const double send = up ? lo : hi, keep = up ? hi : lo;
    p[i] = keep + dpp_f64<CTRL>(send);
  }
}
__device__ __forceinline__ void reduce_scatter32(double* p, int lane) {
  reduce_swap32<16>(p);
  reduce_swap16<8>(p);
  reduce_dpp<4, 0x128, 8>(p, lane);   // row_ror:8
  reduce_dpp<2, 0x141, 4>(p, lane);   // row_half_mirror
  reduce_dpp<1, 0x4E, 2>(p, lane);    // quad_perm:[2,3,0,1]
  p[0] += dpp_f64<0xB1>(p[0]);        // quad_perm:[1,0,3,2]
}
// 64 per-lane values -> their 64-lane sums, value e in lane e (reduce_scatter32 with one more halving in front and the last
// step a halving too)
__device__ __forceinline__ void reduce_scatter64(double* p, int lane) {
  reduce_swap32<32>(p);
  reduce_swap16<16>(p);
  reduce_dpp<8, 0x128, 8>(p, lane);   // row_ror:8
  reduce_dpp<4, 0x141, 4>(p, lane);   // row_half_mirror
  reduce_dpp<2, 0x4E, 2>(p, lane);    // quad_perm:[2,3,0,1]
  reduce_dpp<1, 0xB1, 1>(p, lane);    // quad_perm:[1,0,3,2]
}

// deterministic block-wide sum of one value per thread (256 threads); result valid for thread 0
__device__ __forceinline__ double block_sum256(double v, double* s4) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}

// Backward substitution L^T x = y on the same wave (lane i: rows i and, TWO, i + 64; v = 1 / L_ii). The factor entries
// a lane needs do not depend on the running solution: they are fetched eight steps ahead and pre-multiplied by
// 1 / L_jj, so that a step is one lane read and one FMA on the dependent chain; x_i = b_i / L_ii is formed at the end.
template <bool TWO>
__device__ __forceinline__ void chol_backward(const double* A, int S, int LD, double& b0, double& b1, double v0, double v1) {
  const int lane = threadIdx.x & 63, i0 = lane, i1 = lane + 64;
  if (TWO) {
    // Rows S - 1 .. 64 first: their pivots live in b1 and nowhere else, so a step is two lane reads + two FMAs with nothing to
    // select (round 6: one loop over all rows chose between b0 and b1 on every step -- four lane reads and two scalar selects on
    // the dependent chain, 114 times). Same products, same order: same bits.
    for (int j0 = S - 1; j0 >= 64; j0 -= 8) {
      double a0[8], a1[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int j = j0 - u, jr = j >= 64 ? j : 64;
        const double x0 = A[(size_t)jr * LD + i0];
        const double x1 = A[(size_t)jr * LD + (i1 < LD ? i1 : 0)];
        const double vj = lane_bcast(v1, jr - 64);
        a0[u] = j >= 64 ? x0 * vj : 0.0;              // (every row i0 < 64 <= j)
        a1[u] = (j >= 64 && i1 < j) ? x1 * vj : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int jr = j0 - u >= 64 ? j0 - u : 64;   // (steps below row 64 multiply by the zeros selected above)
        const double bj = lane_bcast(b1, jr - 64);
        b0 -= a0[u] * bj;
        b1 -= a1[u] * bj;
      }
    }
    b1 *= v1;
  }
  for (int j0 = TWO ? 63 : S - 1; j0 >= 0; j0 -= 8) {
    double a0[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int j = j0 - u, jr = j >= 0 ? j : 0;
      // (unconditional loads from row jr, then a select: a conditional load is a branch and a wait of its own)
      const double x0 = A[(size_t)jr * LD + i0];
      const double vj = lane_bcast(v0, jr);
      a0[u] = (j >= 0 && i0 < j) ? x0 * vj : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int jr = j0 - u >= 0 ? j0 - u : 0;   // (steps below row 0 multiply by the zeros selected above)
      const double bj = lane_bcast(b0, jr);      // final: rows > j are done
      b0 -= a0[u] * bj;
    }
  }
  b0 *= v0;
}

// Cholesky of the damped reduced system FOUR columns at a time with LOOK-AHEAD (round 4; medium systems, 24 < S <= 63:
// BASELINE configs[4] is S = 42), the right-hand side riding along as row S of the matrix. One barrier per block of four:
//   wave 0 owns the serial chain. Lane l holds the four entries of row j0 + l in the block's columns, fully updated; a
//     column is pivot (lane read) -> rsqrt -> scale -> up to three updates of (lane read + FMA) -- no LDS round trip and
//     no barrier on the chain. It stores the panel, and behind the barrier applies THIS panel's rank-4 update to the NEXT
//     block's four columns itself (sixteen FMAs per row, multipliers by uniform LDS reads) and goes straight on factoring;
//   waves 1..3 meanwhile give the REST of the trailing matrix (columns beyond the next block, the right-hand side's row
//     included) the same rank-4 update on the matrix pipe: one v_mfma_f64_16x16x4_f64 per 16 x 16 tile, operands straight
//     from LDS, tiles fixed for the whole factorisation (addresses and validity computed once per lane).
// What was measured on the way (scripts/time_chol.py, one workgroup, hot, S = 42, shader cycles at 2.41 GHz): round 3's
// eight-column panels on wave 0 + trailing updates 32.2 k (13.4 us; in the solving block 9.0 + 4.8 us); sixteen-column
// register-row panels with lane reads 13.0 + 3.0 us in the solving block (360 dependent lane-read / FMA triples per panel
// on one wave); four-column blocks with the 4 x 4 diagonal block in closed form on every thread, two barriers and the
// trailing update on all four waves 38.1 k, of which the trailing update 20 k (tiles re-anchored per step) / 15 k (fixed
// tiles) -- a dependent fp64 instruction costs ~20 cycles when a SIMD has one wave to run, so what counts is the LENGTH of
// the dependent chain (~12 instructions per column: 42 x 240 cycles = 4.2 us is the floor), and everything that can
// leave the chain's wave must. s_inv[j] receives 1 / L_jj (backward substitution). All 256 threads call; returns whether
// every pivot was positive and finite (valid in every thread).
__device__ __forceinline__ bool chol_block4(double* A, int S, int LD, double* s_inv) {
  const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63, kq = ln >> 4, c16 = ln & 15;
  __shared__ int s_okb;
  if (tid == 0) s_okb = 1;
  // ---- waves 1..3: the tiles of the trailing update, dealt round robin; fixed rows / columns 16 ti.. / 16 tj.. (ti >= tj)
  const int n16 = (S + 1 + 15) >> 4, ntile = n16 * (n16 + 1) / 2;
  constexpr int kMaxT = 4;   // tiles per wave: ntile <= 10 over three waves (S <= 63)
  int ra[kMaxT], rb[kMaxT], rowmin[kMaxT], colmin[kMaxT], e0[kMaxT];
  bool ina[kMaxT], inb[kMaxT], live[kMaxT];
#pragma unroll
  for (int u = 0; u < kMaxT; ++u) {
    const int t = (wv - 1) + 3 * u;
    live[u] = wv > 0 && t < ntile;
    const int tc = live[u] ? t : 0;
    int ti = (int)((sqrtf(8.0f * (float)tc + 1.0f) - 1.0f) * 0.5f);
    ti = ti * (ti + 1) / 2 > tc ? ti - 1 : ti;
    ti = (ti + 1) * (ti + 2) / 2 <= tc ? ti + 1 : ti;
    const int tj = tc - ti * (ti + 1) / 2;
    const int R = 16 * ti, Cc = 16 * tj;
    ina[u] = live[u] && R + c16 <= S;
    inb[u] = live[u] && Cc + c16 < S;
    ra[u] = (ina[u] ? R + c16 : S) * LD;
    rb[u] = (inb[u] ? Cc + c16 : S - 1) * LD;
    rowmin[u] = R;                        // tile rows R + kq + 4 r, column Cc + c16
    colmin[u] = Cc + c16;
    e0[u] = (R + kq) * LD + Cc + c16;     // element r of this lane: e0 + 4 r LD
  }
  // ---- wave 0: lane l is ROW l of the matrix for the whole factorisation (row S: the right-hand side); x = its entries in the
  // current block's columns, fully updated
  double x[4] = {0.0, 0.0, 0.0, 0.0};
  bool ok = true;
  const double* Row = A + (size_t)(ln <= S ? ln : S) * LD;
  if (wv == 0) {
    const int nb0 = S < 4 ? S : 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const double v = Row[c < nb0 ? c : 0];
      x[c] = (ln <= S && c < nb0 && c <= ln) ? v : 0.0;
    }
  }
  for (int j0 = 0; j0 < S; j0 += 4) {
    const int nb = S - j0 < 4 ? S - j0 : 4, t0 = j0 + nb;
    const int nbn = S - t0 < 4 ? S - t0 : 4;   // width of the next block (<= 0: there is none)
    if (wv == 0) {
      // ---- the block's columns, one after the other
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (c < nb) {   // (uniform)
          const double d = lane_bcast(x[c], j0 + c);
          ok = ok && (d > 0.0) && isfinite(d);
          const double inv = rsqrt_pos(d);
          const double y = x[c] * inv;            // lane j0 + c: d * inv = L_cc; lanes above it: not part of the column
          x[c] = y;
          if (ln == j0 + c) s_inv[j0 + c] = inv;
#pragma unroll
          for (int c2 = c + 1; c2 < 4; ++c2) x[c2] = fma(-y, lane_bcast(y, (j0 + c2) & 63), x[c2]);
        }
      }
      if (ln <= S) {
        double* W = A + (size_t)ln * LD + j0;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < nb && j0 + c <= ln) W[c] = x[c];
      }
    }
    __syncthreads();   // panel j0 is in LDS; waves 1..3 have finished the previous block's trailing update
    if (t0 >= S) break;
    if (wv == 0) {
      // ---- look-ahead: this panel's update of the NEXT block's columns. The row's entries there (final but for this
      // panel: the barrier) and the sixteen multipliers L[t0 + c][j0 + k] (uniform addresses) come in ONE LDS round trip; the
      // row's own panel entries are the registers x[] (lane = row for the whole factorisation). (Multipliers by lane reads
      // instead, with the products under the round trip of the four entries: 21.4 k cycles against 19.9 k -- a lane read
      // into a scalar register followed by its use costs more than a broadcast LDS read.)
      double xn[4], m[4][4];
#pragma unroll
      for (int c = 0; c < 4; ++c) xn[c] = Row[(c < nbn ? t0 + c : 0)];
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) m[c][k] = A[(size_t)(t0 + (c < nbn ? c : 0)) * LD + j0 + (k < nb ? k : 0)];   // L[t0 + c][j0 + k]: uniform address, one round trip for all twenty
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        double a = xn[c];
#pragma unroll
        for (int k = 0; k < 4; ++k) a = fma(-(k < nb ? x[k] : 0.0), m[c][k], a);
        xn[c] = a;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) x[c] = (ln <= S && c < nbn && t0 + c <= ln) ? xn[c] : 0.0;
    } else if (t0 + 4 < S) {
      // ---- waves 1..3: rank-nb update of the rest, columns >= t0 + 4 (the next block's are wave 0's), rows up to S
      const int kc = j0 + (kq < nb ? kq : 0);   // the lane's panel column (one k-step: column kq)
#pragma unroll
      for (int u0 = 0; u0 < kMaxT; u0 += 2) {
        if ((live[u0] && rowmin[u0] + 15 >= t0 + 4) || (u0 + 1 < kMaxT && live[u0 + 1] && rowmin[u0 + 1] + 15 >= t0 + 4)) {   // (uniform; tiles wholly above the corner are finished)
          double am[2], bm[2], old[2][4];
#pragma unroll
          for (int v = 0; v < 2; ++v) {
            const int u = u0 + v;
            const double xa = A[ra[u] + kc], xb = A[rb[u] + kc];
            am[v] = (ina[u] && kq < nb) ? xa : 0.0;
            bm[v] = (inb[u] && kq < nb) ? xb : 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int e = e0[u] + 4 * r * LD;
              old[v][r] = A[(live[u] && e < (S + 1) * LD) ? e : 0];
            }
          }
          d4 T0 = {0.0, 0.0, 0.0, 0.0}, T1 = {0.0, 0.0, 0.0, 0.0};
          T0 = __builtin_amdgcn_mfma_f64_16x16x4f64(am[0], bm[0], T0, 0, 0, 0);
          T1 = __builtin_amdgcn_mfma_f64_16x16x4f64(am[1], bm[1], T1, 0, 0, 0);
#pragma unroll
          for (int v = 0; v < 2; ++v) {
            const int u = u0 + v;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = rowmin[u] + kq + 4 * r, col = colmin[u];
              if (live[u] && col >= t0 + 4 && col < S && row <= S && col <= row) A[e0[u] + 4 * r * LD] = old[v][r] - (v == 0 ? T0[r] : T1[r]);
            }
          }
        }
      }
    }
  }
  if (wv == 0 && ln == 0 && !ok) s_okb = 0;
  __syncthreads();
  return s_okb != 0;
}

}  // namespace cc
