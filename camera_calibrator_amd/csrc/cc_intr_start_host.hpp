// cc_intr_start_host.hpp -- the host side of the fisheye focal-length start (cc_intrinsics_estimate_start_fisheye,
// cc_intrinsics_start_scores; intr_start_run also serves the one-shot pipeline): a part of cc_intrinsics.hip, included there once,
// behind the handle and its helpers, ahead of the one-shot calls. The kernels: cc_intr_start.hpp.
#pragma once

#include "cc_intr_start.hpp"

namespace cc {

// the start's device scratch, one block: on a handle a hipMalloc of its own, grown on demand; in a one-shot call a part of the arena
struct IntrStartLayout {
  size_t o_box, o_ext, o_f, o_score, o_qual, o_best, o_srec, o_skind, o_view, o_kind, bytes;
  IntrStartLayout(int64_t F, int64_t C, int64_t S) {
    ArenaCursor cur;
    o_box = cur.take(8 * sizeof(unsigned long long)); o_ext = cur.take(4 * sizeof(double));
    o_f = cur.take(kIntrStartMaxCandidates * sizeof(double)); o_score = cur.take(kIntrStartMaxCandidates * sizeof(double));
    o_qual = cur.take(kIntrStartMaxCandidates * sizeof(int32_t)); o_best = cur.take(2 * sizeof(int32_t));
    o_srec = cur.take((size_t)C * S * kRigViewStride * sizeof(double)); o_skind = cur.take((size_t)C * S * sizeof(int32_t));
    o_view = cur.take((size_t)F * kRigViewStride * sizeof(double)); o_kind = cur.take((size_t)F * sizeof(int32_t));
    bytes = cur.bytes;
  }
};

// (intr_start_searched, intr_start_check: cc_intr_start.hpp -- the batch's host side, cc_intr_start_batch_host.hpp, takes them too)

// The start on the handle's device observations, in `work` (IntrStartLayout(F, candidates, searched views) bytes). Writes nothing
// to the handle's state. first_invalid (may be NULL): the first view without a pose, -1: none. `timed` (scripts: cc_intrinsics_debug_start_marks): hipEvents
// round the three phases; cc_last_call_timing's slots then receive the device times of the extent, the search with its pick and
// the pose pass, and the call's host time. Off, the call creates no event and leaves cc_last_call_timing alone.
static int intr_start_run(cc_intrinsics* h, char* work, const cc_intr_start_options& o, const char* who, double* intr9, double* q, double* t,
                          cc_intr_start_report* report, int64_t* first_invalid, bool timed) {
  const auto t0 = std::chrono::steady_clock::now();
  const int64_t F = h->F, S = intr_start_searched(o, F);
  const IntrStartLayout L(F, o.candidates, S);
  IntrStartDev P{};
  P.F = F; P.N = h->N; P.S = S; P.C = o.candidates;
  P.centre[0] = o.centre[0]; P.centre[1] = o.centre[1];
  P.theta_lo = o.theta_lo; P.theta_hi = o.theta_hi;
  P.off = h->d.off; P.uv = h->d.uv; P.xyz = h->d.xyz;
  P.box = reinterpret_cast<unsigned long long*>(work + L.o_box); P.ext = reinterpret_cast<double*>(work + L.o_ext);
  P.f = reinterpret_cast<double*>(work + L.o_f); P.score = reinterpret_cast<double*>(work + L.o_score);
  P.qualified = reinterpret_cast<int32_t*>(work + L.o_qual); P.best = reinterpret_cast<int32_t*>(work + L.o_best);
  P.srec = reinterpret_cast<double*>(work + L.o_srec); P.skind = reinterpret_cast<int32_t*>(work + L.o_skind);
  P.view = reinterpret_cast<double*>(work + L.o_view); P.kind = reinterpret_cast<int32_t*>(work + L.o_kind);
  hipEvent_t marks[4] = {nullptr, nullptr, nullptr, nullptr};
  struct Marks { hipEvent_t* m; ~Marks() { for (int i = 0; i < 4; ++i) if (m[i]) hipEventDestroy(m[i]); } } marks_guard{marks};
  bool have_marks = timed;
  for (int i = 0; i < 4 && have_marks; ++i)
    if (hipEventCreate(&marks[i]) != hipSuccess) { (void)hipGetLastError(); marks[i] = nullptr; have_marks = false; }
  intr_start_enqueue(P, h->stream, o.refine_iterations, have_marks ? marks : nullptr);
  CC_HIP(hipGetLastError());
  double ext[4];
  int32_t best[2];
  std::vector<double> view((size_t)F * kRigViewStride);
  std::vector<int32_t> kind((size_t)F);
  CC_HIP(hipMemcpyAsync(ext, P.ext, sizeof(ext), hipMemcpyDeviceToHost, h->stream));
  CC_HIP(hipMemcpyAsync(best, P.best, sizeof(best), hipMemcpyDeviceToHost, h->stream));
  CC_HIP(hipStreamSynchronize(h->stream));
  if (timed) {
    double* tm = last_timing();
    for (int i = 0; i < 5; ++i) tm[i] = 0.0;
    for (int i = 0; i < 3 && have_marks; ++i) {
      float ms = 0.0f;
      if (hipEventElapsedTime(&ms, marks[i], marks[i + 1]) == hipSuccess) tm[i] = ms; else (void)hipGetLastError();
    }
  }
  if (best[0] < 0)
    return fail(CC_ERR_STATE, "%s: no candidate focal length places every searched view (centre %.6g %.6g, r_max %.6g): nothing was written", who, ext[0], ext[1], ext[2]);
  CC_HIP(hipMemcpy(view.data(), P.view, view.size() * sizeof(double), hipMemcpyDeviceToHost));
  CC_HIP(hipMemcpy(kind.data(), P.kind, kind.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  int64_t invalid = 0, first = -1;
  for (int64_t f = 0; f < F; ++f) {
    const double* r = view.data() + f * kRigViewStride;
    const bool ok = kind[(size_t)f] != RIG_VIEW_INVALID;
    if (!ok) { ++invalid; if (first < 0) first = f; }
    if (q) { for (int i = 0; i < 4; ++i) q[f * 4 + i] = ok ? r[i] : (i == 0 ? 1.0 : 0.0); }
    if (t) { for (int i = 0; i < 3; ++i) t[f * 3 + i] = ok ? r[4 + i] : 0.0; }
  }
  if (intr9) {
    for (int i = 0; i < 9; ++i) intr9[i] = 0.0;
    intr9[0] = ext[3]; intr9[1] = ext[3]; intr9[2] = ext[0]; intr9[3] = ext[1];
  }
  if (first_invalid) *first_invalid = first;
  if (report) {
    report->centre[0] = ext[0]; report->centre[1] = ext[1]; report->r_max = ext[2]; report->focal = ext[3];
    report->best_candidate = best[0]; report->candidates_qualified = best[1];
    report->views = F; report->views_searched = S; report->views_invalid = invalid;
  }
  if (timed) last_timing()[3] = ms_since(t0);
  return CC_OK;
}

}  // namespace cc

extern "C" {

void cc_intr_start_options_init(cc_intr_start_options* o) {
  if (!o) return;
  o->centre[0] = o->centre[1] = __builtin_nan("");
  o->theta_lo = 0.3; o->theta_hi = 3.0;
  o->candidates = 24; o->search_views = 32; o->refine_iterations = 3;
}

int cc_intrinsics_estimate_start_fisheye(cc_intrinsics* h, const cc_intr_start_options* opt, double* intr9, double* q, double* t,
                                         cc_intr_start_report* report) {
  using namespace cc;
  const char* who = "cc_intrinsics_estimate_start_fisheye";
  if (!h) return fail(CC_ERR_BAD_ARGUMENT, "%s: NULL handle", who);
  if (h->model != CC_MODEL_FISHEYE) return fail(CC_ERR_STATE, "%s: the handle's model is not CC_MODEL_FISHEYE (cc_intrinsics_set_model; the start is the equidistant lens)", who);
  // (a guard, not a path: cc_intrinsics_set_model refuses a handle with an exchange or a communicator and both refuse a fisheye
  // handle, so no handle gets here with one today)
  if (h->exchange || h->comm) return fail(CC_ERR_STATE, "%s: one device only (the handle has an exchange or a communicator)", who);
  cc_intr_start_options o;
  if (opt) o = *opt; else cc_intr_start_options_init(&o);
  if (int rc = intr_start_check(o, who)) return rc;
  CC_HIP(hipSetDevice(h->device));
  const IntrStartLayout L(h->F, o.candidates, intr_start_searched(o, h->F));
  if (h->start_work_bytes < L.bytes) {
    CC_HIP(hipStreamSynchronize(h->stream));
    if (h->start_work) (void)hipFree(h->start_work);
    h->start_work = nullptr; h->start_work_bytes = 0; h->start_candidates = 0;
    CC_HIP(hipMalloc(&h->start_work, L.bytes));
    h->start_work_bytes = L.bytes;
  }
  h->start_candidates = 0;
  h->start_searched = intr_start_searched(o, h->F);
  h->start_srec = reinterpret_cast<const double*>(static_cast<char*>(h->start_work) + L.o_srec);
  h->start_view = reinterpret_cast<const double*>(static_cast<char*>(h->start_work) + L.o_view);
  if (int rc = intr_start_run(h, static_cast<char*>(h->start_work), o, who, intr9, q, t, report, nullptr, h->start_marks)) {
    if (rc == CC_ERR_STATE) h->start_candidates = o.candidates;   // (the search ran: its scores say why nothing qualified)
    return rc;
  }
  h->start_candidates = o.candidates;
  return CC_OK;
}

// Scripts only (not in the public header): hipEvents round the phases of this handle's later starts, read through cc_last_call_timing
int cc_intrinsics_debug_start_marks(cc_intrinsics* h, int32_t on) {
  if (!h) return cc::fail(CC_ERR_BAD_ARGUMENT, "cc_intrinsics_debug_start_marks: NULL handle");
  h->start_marks = on != 0;
  return CC_OK;
}

int cc_intrinsics_start_scores(cc_intrinsics* h, double* f, double* score, int32_t* qualified) {
  using namespace cc;
  if (!h) return fail(CC_ERR_BAD_ARGUMENT, "cc_intrinsics_start_scores: NULL handle");
  if (h->start_candidates < 1) return fail(CC_ERR_STATE, "cc_intrinsics_start_scores: cc_intrinsics_estimate_start_fisheye has not run on this handle");
  CC_HIP(hipSetDevice(h->device));
  CC_HIP(hipStreamSynchronize(h->stream));
  const IntrStartLayout L(1, 1, 1);   // (the tables sit in front of the parts whose size depends on the problem)
  char* work = static_cast<char*>(h->start_work);
  const size_t C = (size_t)h->start_candidates;
  if (f) CC_HIP(hipMemcpy(f, work + L.o_f, C * sizeof(double), hipMemcpyDeviceToHost));
  if (score) CC_HIP(hipMemcpy(score, work + L.o_score, C * sizeof(double), hipMemcpyDeviceToHost));
  if (qualified) CC_HIP(hipMemcpy(qualified, work + L.o_qual, C * sizeof(int32_t), hipMemcpyDeviceToHost));
  return CC_OK;
}

}  // extern "C"
