// cc_intr_start_view_body.hpp -- the body of one (view, candidate) wave of the fisheye focal-length start, as TEXT: included
// inside k_intr_start_view (cc_intr_start_dev.hpp) and inside k_intrb_start_view (cc_intr_start_batch_dev.hpp), not a function.
// As a force-inlined function that both kernels call, k_intr_start_view does not keep its gfx950 text; as text
// included where it stood, it does, and the batch's kernel is compiled from the same lines. No include guard: each kernel
// includes it once, inside its braces. In scope at the include:
//   P                  an IntrStartDev (value or reference): uv, xyz, off, ext, f are read
//   v, j               the view (index into P.off) and the candidate (index into P.f)
//   out, kind_out      where the record and the kind go
//   lane, s_stage, refine_iterations
// Stages V and R of k_rig_start_view_bearing, unchanged in arithmetic: classification, centring / scaling, board basis, the Gram
// of the tangent rows on the staged matrix contraction, its null vector (iterated until it settles), the sign from sum b . (H y~), the rotation fix and
// Levenberg-Marquardt on the chord. The record is that kernel's, with the chord cost at the returned pose in slot 17 and the kind in slot 18.
  const IntrStartLens lens{P.uv, P.ext[0], P.ext[1], P.f[j]};
  const int64_t s0 = P.off[v], s1 = P.off[v + 1];
  const int64_t n = s1 - s0;
  const float* xyz = P.xyz;
  int kind = RIG_VIEW_INVALID;

  // centroid; a non-finite coordinate anywhere makes every sum non-finite
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, bad = 0.0;
  for (int64_t i = s0 + lane; i < s1; i += 64) {
    a0 += xyz[i * 3]; a1 += xyz[i * 3 + 1]; a2 += xyz[i * 3 + 2];
    bad += (double)lens.uv[i * 2] * 0.0 + (double)lens.uv[i * 2 + 1] * 0.0;
  }
  const double inv_n = 1.0 / (double)(n > 0 ? n : 1);
  const double c[3] = {wsum0(a0) * inv_n, wsum0(a1) * inv_n, wsum0(a2) * inv_n};
  bad = wsum0(bad) + (c[0] + c[1] + c[2]) * 0.0 + (lens.cx + lens.cy + lens.f) * 0.0;
  // scatter about the centroid
  double sc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = s0 + lane; i < s1; i += 64) {
    const double d0 = xyz[i * 3] - c[0], d1 = xyz[i * 3 + 1] - c[1], d2 = xyz[i * 3 + 2] - c[2];
    sc[0] += d0 * d0; sc[1] += d0 * d1; sc[2] += d0 * d2; sc[3] += d1 * d1; sc[4] += d1 * d2; sc[5] += d2 * d2;
  }
#pragma unroll
  for (int e = 0; e < 6; ++e) sc[e] = wsum0(sc[e]);
  const double s2 = (sc[0] + sc[3] + sc[5]) * inv_n;   // mean squared radius
  const bool finite_in = bad == 0.0 && isfinite(s2) && s2 > 0.0 && n >= 4 && lens.f > 0.0;
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
  if (finite_in) {
    const double s = sqrt(s2), is = 1.0 / s, w = inv_n / s2;
    double A[3][3] = {{sc[0] * w, sc[1] * w, sc[2] * w}, {sc[1] * w, sc[3] * w, sc[4] * w}, {sc[2] * w, sc[4] * w, sc[5] * w}}, V[3][3];
    jacobi_eigen<3>(A, V, 10);
    double l[3] = {A[0][0], A[1][1], A[2][2]}, e[3][3];   // e[k] = eigenvector k
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int r = 0; r < 3; ++r) e[k][r] = V[r][k];
    auto order = [&](int i, int j2) {   // ascending, stable
      const bool sw = l[j2] < l[i];
      const double li = sw ? l[j2] : l[i], lj = sw ? l[i] : l[j2];
      l[i] = li; l[j2] = lj;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double ei = sw ? e[j2][r] : e[i][r], ej = sw ? e[i][r] : e[j2][r];
        e[i][r] = ei; e[j2][r] = ej;
      }
    };
    order(0, 1); order(1, 2); order(0, 1);
    const double l0 = fmax(l[0], 0.0), l1 = fmax(l[1], 0.0), l2 = l[2];
    if (l2 > 0.0 && sqrt(l1 / l2) >= kPlanarTol) kind = sqrt(l0 / l1) < kPlanarTol ? RIG_VIEW_PLANAR : RIG_VIEW_GENERAL;
    if (kind == RIG_VIEW_GENERAL && n < 6) kind = RIG_VIEW_INVALID;

    if (kind != RIG_VIEW_INVALID) {
      // basis of the normalised points y = B^T (X - c) / s: the board's own axes (planar) or the world's (general)
      double B[3][3];   // columns
      if (kind == RIG_VIEW_PLANAR) {
        const double n0 = e[2][1] * e[1][2] - e[2][2] * e[1][1], n1 = e[2][2] * e[1][0] - e[2][0] * e[1][2], n2 = e[2][0] * e[1][1] - e[2][1] * e[1][0];
#pragma unroll
        for (int r = 0; r < 3; ++r) { B[r][0] = e[2][r]; B[r][1] = e[1][r]; }
        B[0][2] = n0; B[1][2] = n1; B[2][2] = n2;
      } else {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int k = 0; k < 3; ++k) B[r][k] = r == k ? 1.0 : 0.0;
      }
      // Gram of the tangent rows, 64 observations a pass on the staged matrix contraction
      d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
      const int npass = (int)((n + 63) / 64);
      for (int p = 0; p < npass; ++p) {
        const int64_t idx = s0 + (int64_t)p * 64 + lane;
        const bool valid = idx < s1;
        const int64_t ic = valid ? idx : s0;
        const double d0 = xyz[ic * 3] - c[0], d1 = xyz[ic * 3 + 1] - c[1], d2 = xyz[ic * 3 + 2] - c[2];
        const double y0 = (B[0][0] * d0 + B[1][0] * d1 + B[2][0] * d2) * is, y1 = (B[0][1] * d0 + B[1][1] * d1 + B[2][1] * d2) * is;
        const double y2 = (B[0][2] * d0 + B[1][2] * d1 + B[2][2] * d2) * is;
        double b[3];
        intr_start_bearing_of(lens, ic, b);
        // an orthonormal pair next to b without a branch on its direction (Duff et al. 2017): sg + b2 is never inside (-1, 1)
        const double sg = b[2] < 0.0 ? -1.0 : 1.0, ka = -1.0 / (sg + b[2]), kb = b[0] * b[1] * ka;
        const double e1[3] = {1.0 + sg * b[0] * b[0] * ka, sg * kb, -sg * b[0]}, e2[3] = {kb, sg + b[1] * b[1] * ka, -b[1]};
        double row[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) row[k] = 0.0;
        if (valid) {
          if (kind == RIG_VIEW_PLANAR) {
#pragma unroll
            for (int r = 0; r < 3; ++r) { row[r * 3] = e1[r] * y0; row[r * 3 + 1] = e1[r] * y1; row[r * 3 + 2] = e1[r]; }
          } else {
#pragma unroll
            for (int r = 0; r < 3; ++r) { row[r * 4] = e1[r] * y0; row[r * 4 + 1] = e1[r] * y1; row[r * 4 + 2] = e1[r] * y2; row[r * 4 + 3] = e1[r]; }
          }
        }
        stage_row(s_stage, lane, row);
        wave_lds_fence();
        gram_rows(s_stage, lane, acc0, acc1);
        wave_lds_fence();
#pragma unroll
        for (int k = 0; k < 16; ++k) row[k] = 0.0;
        if (valid) {
          if (kind == RIG_VIEW_PLANAR) {
#pragma unroll
            for (int r = 0; r < 3; ++r) { row[r * 3] = e2[r] * y0; row[r * 3 + 1] = e2[r] * y1; row[r * 3 + 2] = e2[r]; }
          } else {
#pragma unroll
            for (int r = 0; r < 3; ++r) { row[r * 4] = e2[r] * y0; row[r * 4 + 1] = e2[r] * y1; row[r * 4 + 2] = e2[r] * y2; row[r * 4 + 3] = e2[r]; }
          }
        }
        stage_row(s_stage, lane, row);
        wave_lds_fence();
        gram_rows(s_stage, lane, acc0, acc1);
        wave_lds_fence();
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) s_stage[((lane >> 4) + 4 * r) * 16 + (lane & 15)] = acc0[r] + acc1[r];
      wave_lds_fence();
      double Rp[3][3], tp[3];
      if (kind == RIG_VIEW_PLANAR) {
        double G[9][9], h[9];
#pragma unroll
        for (int i = 0; i < 9; ++i)
#pragma unroll
          for (int k = 0; k < 9; ++k) G[i][k] = s_stage[i * 16 + k];
        smallest_eigvec_settled<9>(G, h);
        // the sign that puts the points along their bearings: sum b . (H y~) > 0 (t_z > 0 is wrong for a board the camera's
        // plane cuts); r0, r1 and t are odd in h
        double along = 0.0;
        for (int64_t i = s0 + lane; i < s1; i += 64) {
          const double d0 = xyz[i * 3] - c[0], d1 = xyz[i * 3 + 1] - c[1], d2 = xyz[i * 3 + 2] - c[2];
          const double y0 = (B[0][0] * d0 + B[1][0] * d1 + B[2][0] * d2) * is, y1 = (B[0][1] * d0 + B[1][1] * d1 + B[2][1] * d2) * is;
          double b[3];
          intr_start_bearing_of(lens, i, b);
          along += b[0] * (h[0] * y0 + h[1] * y1 + h[2]) + b[1] * (h[3] * y0 + h[4] * y1 + h[5]) + b[2] * (h[6] * y0 + h[7] * y1 + h[8]);
        }
        along = wsum0(along);
        double lh = 1.0 / sqrt(h[0] * h[0] + h[3] * h[3] + h[6] * h[6]);
        if (along < 0.0) lh = -lh;
        const double r0[3] = {lh * h[0], lh * h[3], lh * h[6]}, r1[3] = {lh * h[1], lh * h[4], lh * h[7]};
        tp[0] = lh * h[2]; tp[1] = lh * h[5]; tp[2] = lh * h[8];
        const double r2[3] = {r0[1] * r1[2] - r0[2] * r1[1], r0[2] * r1[0] - r0[0] * r1[2], r0[0] * r1[1] - r0[1] * r1[0]};
#pragma unroll
        for (int r = 0; r < 3; ++r) { Rp[r][0] = r0[r]; Rp[r][1] = r1[r]; Rp[r][2] = r2[r]; }
      } else {
        double G[12][12], p[12];
#pragma unroll
        for (int i = 0; i < 12; ++i)
#pragma unroll
          for (int k = 0; k < 12; ++k) G[i][k] = s_stage[i * 16 + k];
        smallest_eigvec_settled<12>(G, p);
        // det P_3x3 > 0 after the division: the determinant fixes the sign, there is no mirror solution
        const double det = p[0] * (p[5] * p[10] - p[6] * p[9]) - p[1] * (p[4] * p[10] - p[6] * p[8]) + p[2] * (p[4] * p[9] - p[5] * p[8]);
        const double ia = 1.0 / cbrt(det);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int k = 0; k < 3; ++k) Rp[r][k] = p[r * 4 + k] * ia;
          tp[r] = p[r * 4 + 3] * ia;
        }
      }
      start_fix_rotation(Rp);
      // R = R_p B^T, t = s t_p - R c
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) R[r * 3 + k] = Rp[r][0] * B[k][0] + Rp[r][1] * B[k][1] + Rp[r][2] * B[k][2];
        t[r] = s * tp[r] - (R[r * 3] * c[0] + R[r * 3 + 1] * c[1] + R[r * 3 + 2] * c[2]);
      }
    }
  }

  double rms2 = 0.0, chord = 0.0;
  if (kind != RIG_VIEW_INVALID) {
    // stage R: Levenberg-Marquardt on the six pose coordinates; no depth test, the chord has no singularity short of p = 0
    double H[21], gr[6], cost;
    start_view_sums_bearing(lens, xyz, s0, s1, lane, R, t, H, gr, cost);
    double lambda = 1e-4;
    for (int it = 0; it < refine_iterations; ++it) {
      double d[6], Rn[9], tn[3], Hn[21], gn[6], cn = 0.0;
      bool accept = start_solve6(H, gr, lambda, d);
      if (accept) {
        start_rotate(d, R, Rn);
        tn[0] = t[0] + d[3]; tn[1] = t[1] + d[4]; tn[2] = t[2] + d[5];
        start_view_sums_bearing(lens, xyz, s0, s1, lane, Rn, tn, Hn, gn, cn);
        accept = cn < cost && isfinite(cn);
      }
      if (accept) {
#pragma unroll
        for (int e = 0; e < 21; ++e) H[e] = Hn[e];
#pragma unroll
        for (int e = 0; e < 6; ++e) gr[e] = gn[e];
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = Rn[e];
        t[0] = tn[0]; t[1] = tn[1]; t[2] = tn[2];
        cost = cn;
        lambda *= 0.1;
      } else {
        lambda *= 10.0;
      }
    }
    chord = cost;
    rms2 = cost / (2.0 * (double)n);   // a squared angle for small errors
    if (!isfinite(rms2) || !isfinite(t[0] + t[1] + t[2])) kind = RIG_VIEW_INVALID;
  }
  if (lane == 0) {
    *kind_out = kind;
    if (kind == RIG_VIEW_INVALID) {
#pragma unroll
      for (int i = 0; i < kRigViewStride; ++i) out[i] = 0.0;
    } else {
      double q[4];
      start_quat_of(R, q);
#pragma unroll
      for (int i = 0; i < 4; ++i) out[i] = q[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) out[4 + i] = t[i];
      out[7] = rms2;
#pragma unroll
      for (int i = 0; i < 9; ++i) out[8 + i] = R[i];
#pragma unroll
      for (int i = 17; i < kRigViewStride; ++i) out[i] = 0.0;
      out[kIntrStartCostSlot] = chord;
      out[kIntrStartKindSlot] = (double)kind;
    }
  }
