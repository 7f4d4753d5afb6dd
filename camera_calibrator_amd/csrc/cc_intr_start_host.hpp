// cc_intr_start_host.hpp -- the host side of the fisheye focal-length start (cc_intrinsics_estimate_start_fisheye,
// cc_intrinsics_start_scores, cc_intrinsics_estimate_views_start): a part of cc_intrinsics.hip, included there once, behind the
// handle, its helpers and the one-shot calls. The kernels: cc_intr_start.hpp.
#pragma once

#include "cc_intr_start.hpp"

namespace cc {

// the start's device scratch, one block: on a handle a hipMalloc of its own, grown on demand; in a one-shot call a part of the arena
struct IntrStartLayout {
  size_t o_box, o_ext, o_f, o_score, o_qual, o_best, o_srec, o_skind, o_view, o_kind, bytes;
  IntrStartLayout(int64_t F, int64_t C, int64_t S) {
    size_t cursor = 0;
    auto take = [&](size_t b) { const size_t at = cursor; cursor += (b + 255) & ~(size_t)255; return at; };
    o_box = take(8 * sizeof(unsigned long long)); o_ext = take(4 * sizeof(double));
    o_f = take(kIntrStartMaxCandidates * sizeof(double)); o_score = take(kIntrStartMaxCandidates * sizeof(double));
    o_qual = take(kIntrStartMaxCandidates * sizeof(int32_t)); o_best = take(2 * sizeof(int32_t));
    o_srec = take((size_t)C * S * kRigViewStride * sizeof(double)); o_skind = take((size_t)C * S * sizeof(int32_t));
    o_view = take((size_t)F * kRigViewStride * sizeof(double)); o_kind = take((size_t)F * sizeof(int32_t));
    bytes = cursor;
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

// cc_intrinsics_estimate_views_model with the start chosen: NULL -> that call (Zhang); else the focal search on the fisheye model
int cc_intrinsics_estimate_views_start(const cc_options* opt, int32_t device, int64_t F, const float* const* uv_views,
                                       const float* const* xyz_views, const int64_t* counts, const double* distortion5, uint32_t mask,
                                       float* K_init9, double* intr9, double* q, double* t, cc_summary* summary, double huber_a, int32_t model,
                                       const cc_intr_start_options* start) {
  if (!start)
    return cc_intrinsics_estimate_views_model(opt, device, F, uv_views, xyz_views, counts, distortion5, mask, K_init9, intr9, q, t, summary, huber_a, model);
  cc::last_call_status_reset();
  using namespace cc;
  const char* who = "cc_intrinsics_estimate_views_start";
  if (F < 3 || !uv_views || !xyz_views || !counts || !intr9 || !q || !t) return fail(CC_ERR_BAD_ARGUMENT, "%s: needs >= 3 views and non-NULL arrays", who);
  if (huber_a != huber_a) return fail(CC_ERR_BAD_ARGUMENT, "%s: huber_a is NaN", who);
  if (model != CC_MODEL_FISHEYE) return fail(CC_ERR_BAD_ARGUMENT, "%s: the focal-length search is a start of the fisheye model (model %d)", who, (int)model);
  if (int rc = intr_start_check(*start, who)) return rc;
  if (int rc = select_device(device)) return rc;
  const IntrStartLayout L(F, start->candidates, intr_start_searched(*start, F));
  double* tm = last_timing();
  for (int i = 0; i < 5; ++i) tm[i] = 0.0;
  ViewsUpload up;
  if (int rc = up.open(who, device, F, uv_views, xyz_views, counts, 0, L.bytes)) return rc;
  if (huber_a > 0.0) up.h->huber_a = huber_a;
  up.h->model = model;
  auto t0 = std::chrono::steady_clock::now();
  int64_t first_invalid = -1;
  int rc = intr_start_run(up.h, up.h->extra, *start, who, intr9, q, t, nullptr, &first_invalid, false);
  tm[2] = ms_since(t0); t0 = std::chrono::steady_clock::now();
  if (rc == CC_ERR_STATE) {   // (the data admit no start: the caller's arguments, not a state of a handle the caller has)
    const std::string why = last_error();
    rc = fail(CC_ERR_BAD_ARGUMENT, "%s", why.c_str());
  }
  if (!rc && first_invalid >= 0) rc = fail(CC_ERR_BAD_ARGUMENT, "%s: view %lld has no pose at any candidate focal length (fewer than 4 points, collinear points, or a non-finite pixel or point)", who, (long long)first_invalid);
  if (!rc) {
    if (K_init9) {
      const float K9[9] = {(float)intr9[0], 0.0f, (float)intr9[2], 0.0f, (float)intr9[1], (float)intr9[3], 0.0f, 0.0f, 1.0f};
      std::memcpy(K_init9, K9, sizeof(K9));
    }
    for (int i = 0; i < 4; ++i) intr9[4 + i] = distortion5 ? distortion5[i] : 0.0;   // the distortion starts from the caller's, as after Zhang
    rc = cc_intrinsics_set_state(up.h, intr9, mask, q, t);
  }
  cc_options o;
  if (opt) o = *opt; else cc_options_init(&o);
  o.use_graph = 0;
  if (!rc) rc = cc_intrinsics_solve(up.h, &o, summary);
  tm[3] = ms_since(t0); t0 = std::chrono::steady_clock::now();
  if (!rc) rc = cc_intrinsics_get_state(up.h, intr9, q, t);
  tm[4] = ms_since(t0);
  if (rc) (void)hipStreamSynchronize(up.h->stream);   // (an early return may have left copies from the staging block in flight)
  return rc;
}

}  // extern "C"
