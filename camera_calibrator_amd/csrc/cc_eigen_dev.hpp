// cc_eigen_dev.hpp -- small symmetric eigen-problems in registers (device): the cyclic Jacobi decomposition and the inverse
// iteration for the smallest eigenvector. Shared by the kernels of Zhang's initialisation (cc_zhang_dev.hpp) and of the rig
// start (cc_rig_start_dev.hpp).
#pragma once

#include "cc_common.hpp"

namespace cc {

// Cyclic Jacobi eigen-decomposition of a symmetric N x N matrix held in registers. On return the
// diagonal of A holds the eigenvalues and the columns of V the eigenvectors.
template <int N>
__device__ __forceinline__ void jacobi_eigen(double (&A)[N][N], double (&V)[N][N], int sweeps) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sw = 0; sw < sweeps; ++sw) {
#pragma unroll
    for (int p = 0; p < N - 1; ++p)
#pragma unroll
      for (int q = p + 1; q < N; ++q) {
        const double apq = A[p][q];
        const bool skip = apq == 0.0;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * (skip ? 1.0 : apq));
        double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        if (skip) t = 0.0;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        A[p][p] -= t * apq;
        A[q][q] += t * apq;
        A[p][q] = 0.0;
        A[q][p] = 0.0;
#pragma unroll
        for (int r = 0; r < N; ++r) {
          if (r != p && r != q) {
            const double arp = A[r][p], arq = A[r][q];
            const double np = c * arp - s * arq, nq = s * arp + c * arq;
            A[r][p] = np; A[p][r] = np;
            A[r][q] = nq; A[q][r] = nq;
          }
          const double vrp = V[r][p], vrq = V[r][q];
          V[r][p] = c * vrp - s * vrq;
          V[r][q] = s * vrp + c * vrq;
        }
      }
  }
}

// Unit eigenvector of the SMALLEST eigenvalue of a symmetric positive semi-definite N x N matrix (registers):
// inverse iteration x <- A^-1 x with A^-1 applied as S (S A S + mu I)^-1 S, S = diag(A)^-1/2. The equilibration
// matters: DLT Gram matrices are badly graded (no Hartley normalisation in the reference, geometry.cpp:70-105; a
// nearly edge-on board gives world coordinates of 1e5 and eigenvalues from 1e-1 to 1e16), and a Cholesky of the raw
// matrix loses the small eigen-space entirely there, while the unit-diagonal one keeps it to ~1e-6 (float32, the
// precision H is stored in). mu = 1e-14 N keeps the pivots positive when the smallest eigenvalue is zero up to
// rounding (exact data, four-point homographies). The smallest eigenvalue is noise-sized and the next one is not,
// so the iteration gains many digits per step; 12 steps, ~1.5 kflop in ~70 registers, against ~26 kflop and 162
// live doubles (spilling) for the full Jacobi decomposition it replaces.
// What comes out is the eigenvector of A + mu diag(A), not of A: off by ~mu |A| / (gap to the next eigenvalue), ~1e-11 on DLT
// systems -- nothing next to the float32 H of Zhang's initialisation. A caller that keeps the vector in fp64 (the rig start)
// passes shift = 0: the pivots then stay positive by the 1e-30 floor alone, which moves the last pivot of a matrix that is
// singular up to rounding by a rounding error, and the iteration converges to the eigenvector of A itself.
// (smallest_eigvec_settled in cc_intr_start_dev.hpp is a copy of this function at shift 0 that iterates until the vector settles:
// a fix here belongs there too.)
template <int N>
__device__ __forceinline__ void smallest_eigvec(const double (&A)[N][N], double (&x)[N], double shift = 1e-14) {
  double sc[N];
#pragma unroll
  for (int i = 0; i < N; ++i) sc[i] = A[i][i] > 0.0 ? rsqrt(A[i][i]) : 1.0;
  const double mu = shift * N;
  double L[N][N], inv[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double d = sc[j] * A[j][j] * sc[j] + mu;
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    d = fmax(d, 1e-30);
    const double r = rsqrt(d);
    inv[j] = r;
    L[j][j] = d * r;
#pragma unroll
    for (int i = j + 1; i < N; ++i) {
      double a = sc[i] * A[i][j] * sc[j];
#pragma unroll
      for (int k = 0; k < j; ++k) a -= L[i][k] * L[j][k];
      L[i][j] = a * r;
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) x[i] = (i & 1) ? 0.7 : 1.0;   // not orthogonal to anything in particular
  for (int it = 0; it < 12; ++it) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      double a = x[i] * sc[i];
#pragma unroll
      for (int k = 0; k < i; ++k) a -= L[i][k] * x[k];
      x[i] = a * inv[i];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
      double a = x[i];
#pragma unroll
      for (int k = i + 1; k < N; ++k) a -= L[k][i] * x[k];
      x[i] = a * inv[i];
    }
    double n2 = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) { x[i] *= sc[i]; n2 += x[i] * x[i]; }
    const double rn = rsqrt(n2);
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] *= rn;
  }
}

}  // namespace cc
