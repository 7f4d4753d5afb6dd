// cc_intr_start_batch_host.hpp -- the host side of the batched fisheye focal-length start (cc_intrinsics_batch_estimate_start_fisheye,
// cc_intrinsics_batch_start_scores; intr_start_batch_run also serves the one-shot pipeline): a part of cc_intrinsics_batch.hip,
// included there once, behind the handle and its helpers, ahead of the one-shot calls. The kernels: cc_intr_start_batch.hpp.
#pragma once

#include "cc_intr_start_batch.hpp"

#include <string>

namespace cc {

// the start's device scratch, one block: on a handle a hipMalloc of its own, grown on demand; in a one-shot call a part of the
// arena. The tables the host builds (prob, search_where, extent) are one run of bytes: one upload.
struct IntrStartBatchLayout {
  size_t o_prob, o_where, o_extent, tables_bytes, o_box, o_ext, o_f, o_score, o_qual, o_best, o_srec, o_skind, o_view, o_kind, bytes;
  IntrStartBatchLayout(int64_t B, int64_t Ftot, int64_t Stot, int64_t E, int64_t C) {
    ArenaCursor cur;
    o_prob = cur.take((size_t)B * sizeof(IntrStartDev)); o_where = cur.take((size_t)Stot * 2 * sizeof(int32_t));
    o_extent = cur.take((size_t)E * sizeof(IntrStartExtentWg));
    tables_bytes = cur.bytes;
    o_box = cur.take((size_t)B * 8 * sizeof(unsigned long long)); o_ext = cur.take((size_t)B * 4 * sizeof(double));
    o_f = cur.take((size_t)B * kIntrStartMaxCandidates * sizeof(double)); o_score = cur.take((size_t)B * kIntrStartMaxCandidates * sizeof(double));
    o_qual = cur.take((size_t)B * kIntrStartMaxCandidates * sizeof(int32_t)); o_best = cur.take((size_t)B * 2 * sizeof(int32_t));
    o_srec = cur.take((size_t)C * Stot * kRigViewStride * sizeof(double)); o_skind = cur.take((size_t)C * Stot * sizeof(int32_t));
    o_view = cur.take((size_t)Ftot * kRigViewStride * sizeof(double)); o_kind = cur.take((size_t)Ftot * sizeof(int32_t));
    bytes = cur.bytes;
  }
};

// What one batched start leaves on the host besides the caller's arrays.
struct IntrStartBatchOutcome {
  int64_t no_winner = -1;                          // the first problem without a qualified candidate, -1: none
  int64_t invalid_problem = -1, invalid_view = -1; // the first view without a pose at its problem's winner (local index), -1: none
};

// The start of every problem of the handle on its device observations, in `work` (IntrStartBatchLayout bytes; `tables` built from
// the handle's offsets and o.search_views). Writes nothing to the handle's state. One wait.
static int intr_start_batch_run(cc_intrinsics_batch* h, char* work, const IntrStartBatchTables& tables, const IntrStartBatchLayout& L,
                                const cc_intr_start_options& o, const char* who, double* intr9, double* q, double* t,
                                cc_intr_start_report* reports, IntrStartBatchOutcome* outcome) {
  const int64_t B = h->B, Ftot = h->Ftot, C = o.candidates;
  const int64_t Stot = tables.searched[(size_t)B], E = (int64_t)tables.extent.size();
  if (E >= ((int64_t)1 << 31) || Stot >= ((int64_t)1 << 31)) return fail(CC_ERR_BAD_ARGUMENT, "%s: too many observations or searched views for one launch", who);
  auto at = [&](size_t off) { return work + off; };
  std::vector<char> staged(L.tables_bytes, 0);
  IntrStartDev* prob = reinterpret_cast<IntrStartDev*>(staged.data() + L.o_prob);
  for (int64_t p = 0; p < B; ++p) {
    const int64_t f0 = h->first[(size_t)p], s0 = tables.searched[(size_t)p];
    IntrStartDev& P = prob[p];
    P.F = h->first[(size_t)p + 1] - f0; P.N = h->N; P.S = tables.searched[(size_t)p + 1] - s0; P.C = (int32_t)C;
    P.centre[0] = o.centre[0]; P.centre[1] = o.centre[1];
    P.theta_lo = o.theta_lo; P.theta_hi = o.theta_hi;
    P.off = h->d.off + f0; P.uv = h->d.uv; P.xyz = h->d.xyz;
    P.box = reinterpret_cast<unsigned long long*>(at(L.o_box)) + p * 8; P.ext = reinterpret_cast<double*>(at(L.o_ext)) + p * 4;
    P.f = reinterpret_cast<double*>(at(L.o_f)) + p * kIntrStartMaxCandidates;
    P.score = reinterpret_cast<double*>(at(L.o_score)) + p * kIntrStartMaxCandidates;
    P.qualified = reinterpret_cast<int32_t*>(at(L.o_qual)) + p * kIntrStartMaxCandidates;
    P.best = reinterpret_cast<int32_t*>(at(L.o_best)) + p * 2;
    P.srec = reinterpret_cast<double*>(at(L.o_srec)) + C * s0 * kRigViewStride; P.skind = reinterpret_cast<int32_t*>(at(L.o_skind)) + C * s0;
    P.view = reinterpret_cast<double*>(at(L.o_view)) + f0 * kRigViewStride; P.kind = reinterpret_cast<int32_t*>(at(L.o_kind)) + f0;
  }
  if (Stot) std::memcpy(staged.data() + L.o_where, tables.search_where.data(), (size_t)Stot * 2 * sizeof(int32_t));
  if (E) std::memcpy(staged.data() + L.o_extent, tables.extent.data(), (size_t)E * sizeof(IntrStartExtentWg));
  CC_HIP(hipMemcpyAsync(work, staged.data(), staged.size(), hipMemcpyHostToDevice, h->stream));   // (`staged` lives until the wait below)
  IntrStartBatchDev T{};
  T.B = (int32_t)B; T.C = (int32_t)C; T.Ftot = Ftot; T.Stot = Stot; T.E = E;
  T.prob = reinterpret_cast<const IntrStartDev*>(at(L.o_prob));
  T.search_where = reinterpret_cast<const int2*>(at(L.o_where));
  T.view_where = h->d.where;
  T.extent = reinterpret_cast<const IntrStartExtentWg*>(at(L.o_extent));
  T.box = reinterpret_cast<unsigned long long*>(at(L.o_box));
  intr_start_batch_enqueue(T, h->stream, o.refine_iterations);
  CC_HIP(hipGetLastError());
  std::vector<double> ext((size_t)B * 4), view((size_t)Ftot * kRigViewStride);
  std::vector<int32_t> best((size_t)B * 2), kind((size_t)Ftot);
  CC_HIP(hipMemcpyAsync(ext.data(), at(L.o_ext), ext.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  CC_HIP(hipMemcpyAsync(best.data(), at(L.o_best), best.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  CC_HIP(hipMemcpyAsync(view.data(), at(L.o_view), view.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  CC_HIP(hipMemcpyAsync(kind.data(), at(L.o_kind), kind.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  CC_HIP(hipStreamSynchronize(h->stream));
  IntrStartBatchOutcome out;
  std::vector<int64_t> invalid((size_t)B, 0);
  for (int64_t p = 0; p < B; ++p) {
    if (best[(size_t)p * 2] < 0) { if (out.no_winner < 0) out.no_winner = p; continue; }   // (the pose pass wrote nothing for it)
    for (int64_t f = h->first[(size_t)p]; f < h->first[(size_t)p + 1]; ++f)
      if (kind[(size_t)f] == RIG_VIEW_INVALID) {
        ++invalid[(size_t)p];
        if (out.invalid_problem < 0) { out.invalid_problem = p; out.invalid_view = f - h->first[(size_t)p]; }
      }
  }
  if (reports)
    for (int64_t p = 0; p < B; ++p) {
      cc_intr_start_report& r = reports[p];
      const double* e = ext.data() + p * 4;
      r.centre[0] = e[0]; r.centre[1] = e[1]; r.r_max = e[2]; r.focal = e[3];
      r.best_candidate = best[(size_t)p * 2]; r.candidates_qualified = best[(size_t)p * 2 + 1];
      r.views = h->first[(size_t)p + 1] - h->first[(size_t)p]; r.views_searched = tables.searched[(size_t)p + 1] - tables.searched[(size_t)p];
      r.views_invalid = invalid[(size_t)p];
    }
  if (outcome) *outcome = out;
  if (out.no_winner >= 0) {
    const double* e = ext.data() + out.no_winner * 4;
    return fail(CC_ERR_STATE, "%s: problem %lld: no candidate focal length places every searched view (centre %.6g %.6g, r_max %.6g): nothing but the reports was written",
                who, (long long)out.no_winner, e[0], e[1], e[2]);
  }
  for (int64_t f = 0; f < Ftot; ++f) {
    const double* r = view.data() + f * kRigViewStride;
    const bool ok = kind[(size_t)f] != RIG_VIEW_INVALID;
    if (q) { for (int i = 0; i < 4; ++i) q[f * 4 + i] = ok ? r[i] : (i == 0 ? 1.0 : 0.0); }
    if (t) { for (int i = 0; i < 3; ++i) t[f * 3 + i] = ok ? r[4 + i] : 0.0; }
  }
  if (intr9)
    for (int64_t p = 0; p < B; ++p) {
      double* k = intr9 + p * 9;
      const double* e = ext.data() + p * 4;
      for (int i = 0; i < 9; ++i) k[i] = 0.0;
      k[0] = e[3]; k[1] = e[3]; k[2] = e[0]; k[3] = e[1];
    }
  return CC_OK;
}

}  // namespace cc

extern "C" {

int cc_intrinsics_batch_estimate_start_fisheye(cc_intrinsics_batch* h, const cc_intr_start_options* opt, double* intr9, double* q, double* t,
                                               cc_intr_start_report* reports) {
  using namespace cc;
  const char* who = "cc_intrinsics_batch_estimate_start_fisheye";
  if (!h) return fail(CC_ERR_BAD_ARGUMENT, "%s: NULL handle", who);
  if (h->model != CC_MODEL_FISHEYE) return fail(CC_ERR_STATE, "%s: the handle's model is not CC_MODEL_FISHEYE (cc_intrinsics_batch_set_model; the start is the equidistant lens)", who);
  cc_intr_start_options o;
  if (opt) o = *opt; else cc_intr_start_options_init(&o);
  if (int rc = intr_start_check(o, who)) return rc;
  CC_HIP(hipSetDevice(h->device));
  IntrStartBatchTables tables;
  {
    const std::vector<int64_t> poff(h->first.begin(), h->first.end());
    intr_start_batch_tables(h->B, poff.data(), h->foff.data(), o.search_views, &tables);
  }
  const IntrStartBatchLayout L(h->B, h->Ftot, tables.searched[(size_t)h->B], (int64_t)tables.extent.size(), o.candidates);
  if (h->start_work_bytes < L.bytes) {
    CC_HIP(hipStreamSynchronize(h->stream));
    if (h->start_work) (void)hipFree(h->start_work);
    h->start_work = nullptr; h->start_work_bytes = 0; h->start_candidates = 0;
    CC_HIP(hipMalloc(&h->start_work, L.bytes));
    h->start_work_bytes = L.bytes;
  }
  h->start_candidates = 0;
  char* work = static_cast<char*>(h->start_work);
  h->start_f = reinterpret_cast<const double*>(work + L.o_f); h->start_score = reinterpret_cast<const double*>(work + L.o_score);
  h->start_qualified = reinterpret_cast<const int32_t*>(work + L.o_qual);
  const int rc = intr_start_batch_run(h, work, tables, L, o, who, intr9, q, t, reports, nullptr);
  if (rc == CC_OK || rc == CC_ERR_STATE) h->start_candidates = o.candidates;   // (the search ran: its scores say why nothing qualified)
  return rc;
}

int cc_intrinsics_batch_start_scores(cc_intrinsics_batch* h, double* f, double* score, int32_t* qualified) {
  using namespace cc;
  const char* who = "cc_intrinsics_batch_start_scores";
  if (!h) return fail(CC_ERR_BAD_ARGUMENT, "%s: NULL handle", who);
  if (h->start_candidates < 1) return fail(CC_ERR_STATE, "%s: cc_intrinsics_batch_estimate_start_fisheye has not run on this handle", who);
  CC_HIP(hipSetDevice(h->device));
  CC_HIP(hipStreamSynchronize(h->stream));
  const size_t B = (size_t)h->B, C = (size_t)h->start_candidates, M = kIntrStartMaxCandidates;
  std::vector<double> df(B * M), ds(B * M);
  std::vector<int32_t> dq(B * M);
  CC_HIP(hipMemcpy(df.data(), h->start_f, df.size() * sizeof(double), hipMemcpyDeviceToHost));
  CC_HIP(hipMemcpy(ds.data(), h->start_score, ds.size() * sizeof(double), hipMemcpyDeviceToHost));
  CC_HIP(hipMemcpy(dq.data(), h->start_qualified, dq.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (size_t p = 0; p < B; ++p)
    for (size_t j = 0; j < C; ++j) {
      if (f) f[p * C + j] = df[p * M + j];
      if (score) score[p * C + j] = ds[p * M + j];
      if (qualified) qualified[p * C + j] = dq[p * M + j];
    }
  return CC_OK;
}

}  // extern "C"
