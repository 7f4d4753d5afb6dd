// cc_rig_start_host.hpp -- the host side of the rig start (cc_rig_estimate_start, cc_rigk_estimate_start, cc_rigk_estimate_start_bearing
// and their read-backs): a part of cc_rig.hip, included there once, behind the handle and its helpers.
#pragma once

// ---- start poses from the observations (cc_rig_start.hpp: the kernels; cc_rig_tree.hpp: the tree) -----------------------------
namespace cc {
static int rig_start_alloc(cc_rig* h) {
  RigStartDev& s = h->st;
  const RigDev& d = h->d;
  s.F = h->F; s.NG = h->NG; s.C = (int32_t)h->C; s.CO = d.CO;
  s.uv = d.uv; s.oxyz = d.oxyz; s.goff = d.goff; s.fslot = d.fslot; s.obs_cam = d.obs_cam;
  s.cam = h->init_cam; s.pose = h->init_pose;
  if (h->st_alloc) return CC_OK;
  std::vector<int32_t> cobs((size_t)h->C, -1);
  int32_t j = 0;
  for (int64_t c = 0; c < h->C; ++c) if (h->seen_any[(size_t)c]) cobs[(size_t)c] = j++;
  if (int rc = dev_upload(h, &s.cobs, cobs)) return rc;
  if (int rc = dev_alloc(h, &s.view, (size_t)h->NG * kRigViewStride)) return rc;
  if (int rc = dev_alloc(h, &s.kind, (size_t)h->NG)) return rc;
  if (int rc = dev_alloc(h, &h->st_edges, (size_t)h->C * 2)) return rc;
  if (int rc = dev_alloc(h, &s.rel, (size_t)h->C * 8)) return rc;
  if (int rc = dev_alloc(h, &h->st_placed, (size_t)h->C)) return rc;
  if (int rc = dev_zeroed(h, &s.fplaced, (size_t)h->F)) return rc;
  s.edges = h->st_edges; s.placed = h->st_placed;
  h->st_alloc = true;
  return CC_OK;
}
}  // namespace cc

extern "C" {

void cc_rig_start_options_init(cc_rig_start_options* o) { if (o) o->refine_iterations = 10; }

}  // extern "C"

// The start of the three entry points (`who` names the caller in the messages). RIG_START_PIXELS: the handle's observations go
// through k_rigk_start_unproject first and the start reads its output; RIG_START_BEARINGS: through k_rigk_start_bearing, and
// stages V and R are k_rig_start_view_bearing on its output; otherwise the start reads the handle's observations themselves.
enum { RIG_START_POINTS = 0, RIG_START_PIXELS = 1, RIG_START_BEARINGS = 2 };
static int rig_start_run(cc_rig* h, const char* who, int mode, const cc_rig_start_options* opt, const double* cam_q, const double* cam_t,
                         const double* frame_q, const double* frame_t, cc_rig_start_report* report) {
  using namespace cc;
  if (h->exchange || h->comm) return fail(CC_ERR_STATE, "%s: one device only (the handle has an exchange or a communicator)", who);
  if (h->d.CO < 1 || h->NG < 1) return fail(CC_ERR_STATE, "%s: no camera is observed", who);
  const int iters = opt ? opt->refine_iterations : 10;
  if (iters < 0 || iters > 1000) return fail(CC_ERR_BAD_ARGUMENT, "%s: refine_iterations must be in 0 .. 1000", who);
  CC_HIP(hipSetDevice(h->device));
  if (int rc = rig_start_alloc(h)) return rc;
  if (mode == RIG_START_PIXELS) {
    if (!h->st_points) {   // (once per handle)
      if (int rc = dev_alloc(h, &h->st_points, (size_t)h->N * 2)) return rc;
    }
    const RigDev& d = h->d;
    h->st_have_points = false;
    h->st_have_bearings = false;   // (each of the two read-backs serves its own start only)
    if (h->model == CC_MODEL_MIXED) rigk_start_enqueue_unproject_cam(RigkStartCamDev{h->NG, h->d_cmodel, d.uv, d.goff, d.gcam, d.kset, h->init_intr, h->st_points}, h->stream);
    else rigk_start_enqueue_unproject(RigkStartDev{h->NG, (int32_t)h->model, d.uv, d.goff, d.gcam, d.kset, h->init_intr, h->st_points}, h->stream);
    CC_HIP(hipGetLastError());
    h->st.uv = h->st_points;
    h->st_have_points = true;
  } else if (mode == RIG_START_BEARINGS) {
    if (!h->st_bearings) {   // (once per handle)
      if (int rc = dev_alloc(h, &h->st_bearings, (size_t)h->N * 3)) return rc;
    }
    const RigDev& d = h->d;
    h->st_have_points = false;
    h->st_have_bearings = false;
    rigk_start_enqueue_bearing(RigkBearingDev{h->NG, (int32_t)h->model, h->model == CC_MODEL_MIXED ? h->d_cmodel : nullptr, d.uv, d.goff, d.gcam,
                                              d.kset, h->init_intr, h->st_bearings}, h->stream);
    CC_HIP(hipGetLastError());
    h->st_have_bearings = true;
  }
  const int64_t C = h->C, F = h->F, NG = h->NG;
  // stages V and R; the kinds come back for the tree
  h->st_views = false;
  if (mode == RIG_START_BEARINGS) rig_start_enqueue_views_bearing(h->st, h->st_bearings, h->stream, iters);
  else rig_start_enqueue_views(h->st, h->stream, iters);
  CC_HIP(hipGetLastError());
  std::vector<int32_t> kind((size_t)NG);
  CC_HIP(hipMemcpyAsync(kind.data(), h->st.kind, (size_t)NG * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  CC_HIP(hipStreamSynchronize(h->stream));
  h->st_views = true;
  // stage T: co-visible valid views of every pair of cameras (the groups are sorted by frame)
  std::vector<int64_t> covis((size_t)C * C, 0);
  int64_t n_planar = 0, n_general = 0;
  for (int64_t f = 0; f < F; ++f) {
    const int64_t a = h->fgoff_h[(size_t)f], b = h->fgoff_h[(size_t)f + 1];
    for (int64_t g = a; g < b; ++g) {
      if (kind[(size_t)g] == RIG_VIEW_INVALID) continue;
      (kind[(size_t)g] == RIG_VIEW_PLANAR ? n_planar : n_general) += 1;
      for (int64_t g2 = a; g2 < b; ++g2)
        if (kind[(size_t)g2] != RIG_VIEW_INVALID) covis[(size_t)h->gcam_h[(size_t)g] * C + h->gcam_h[(size_t)g2]] += 1;
    }
  }
  std::vector<uint8_t> frozen((size_t)C, 0);
  for (int64_t c = 0; c < C && c < (int64_t)h->frozen.size(); ++c) frozen[(size_t)c] = h->frozen[(size_t)c];
  const RigStartTree tree = rig_start_tree((int)C, covis.data(), frozen.data());
  // the caller's poses; the root defines the rig frame when no frozen camera is observed
  std::vector<double> cam((size_t)C * 8, 0.0), pose((size_t)F * 8, 0.0);
  for (int64_t c = 0; c < C; ++c) {
    cam[c * 8] = 1.0;
    if (cam_q && !(tree.root_at_identity && c == tree.root)) for (int i = 0; i < 4; ++i) cam[c * 8 + i] = cam_q[c * 4 + i];
    if (cam_t && !(tree.root_at_identity && c == tree.root)) for (int i = 0; i < 3; ++i) cam[c * 8 + 4 + i] = cam_t[c * 3 + i];
  }
  for (int64_t f = 0; f < F; ++f) {
    pose[f * 8] = 1.0;
    if (frame_q) for (int i = 0; i < 4; ++i) pose[f * 8 + i] = frame_q[f * 4 + i];
    if (frame_t) for (int i = 0; i < 3; ++i) pose[f * 8 + 4 + i] = frame_t[f * 3 + i];
  }
  std::vector<int32_t> edges((size_t)C * 2, 0);
  const int n_edges = (int)tree.order.size();
  for (int k = 0; k < n_edges; ++k) { edges[(size_t)k * 2] = tree.order[(size_t)k]; edges[(size_t)k * 2 + 1] = tree.parent[(size_t)tree.order[(size_t)k]]; }
  CC_HIP(hipMemcpy(h->init_cam, cam.data(), cam.size() * sizeof(double), hipMemcpyHostToDevice));
  CC_HIP(hipMemcpy(h->init_pose, pose.data(), pose.size() * sizeof(double), hipMemcpyHostToDevice));
  CC_HIP(hipMemcpy(h->st_edges, edges.data(), edges.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  CC_HIP(hipMemcpy(h->st_placed, tree.placed.data(), (size_t)C, hipMemcpyHostToDevice));
  // stages C and F, into the starting point of the handle
  rig_start_enqueue_poses(h->st, h->stream, n_edges);
  CC_HIP(hipGetLastError());
  std::vector<uint8_t> fplaced((size_t)F, 0);
  CC_HIP(hipMemcpyAsync(fplaced.data(), h->st.fplaced, (size_t)F, hipMemcpyDeviceToHost, h->stream));
  CC_HIP(hipStreamSynchronize(h->stream));
  h->have_state = true;
  if (report) {
    report->views_planar = n_planar; report->views_general = n_general;
    report->views_valid = n_planar + n_general; report->views_invalid = NG - report->views_valid;
    report->frames_placed = 0;
    for (uint8_t p : fplaced) report->frames_placed += p;
    report->frames_unplaced = F - report->frames_placed;
    report->cameras_placed = tree.n_placed; report->cameras_unplaced = tree.n_unplaced;
    report->root_camera = tree.root; report->root_at_identity = tree.root_at_identity ? 1 : 0;
    if (report->parent) for (int64_t c = 0; c < C; ++c) report->parent[c] = tree.parent[(size_t)c];
  }
  return cc_rig_reset(h);
}

extern "C" {

int cc_rig_estimate_start(cc_rig* h, const cc_rig_start_options* opt, const double* cam_q, const double* cam_t, const double* frame_q,
                          const double* frame_t, cc_rig_start_report* report) {
  using namespace cc;
  if (!h) return fail(CC_ERR_BAD_ARGUMENT, "cc_rig_estimate_start: NULL handle");
  if (h->d.kmode) return fail(CC_ERR_STATE, "cc_rig_estimate_start: a cc_rigk_* handle holds pixel observations (the start needs normalised image points: cc_rigk_estimate_start)");
  return rig_start_run(h, "cc_rig_estimate_start", RIG_START_POINTS, opt, cam_q, cam_t, frame_q, frame_t, report);
}

// EXTENSION: the same start for a handle with intrinsics, from its pixels and its start intrinsics (cc_rigk_start.hpp)
int cc_rigk_estimate_start(cc_rig* h, const cc_rig_start_options* opt, const double* cam_q, const double* cam_t, const double* frame_q,
                           const double* frame_t, cc_rig_start_report* report) {
  using namespace cc;
  if (!h) return fail(CC_ERR_BAD_ARGUMENT, "cc_rigk_estimate_start: NULL handle");
  if (!h->d.kmode) return fail(CC_ERR_STATE, "cc_rigk_estimate_start: the handle was created without intrinsics (cc_rig_create: its observations are normalised image points, cc_rig_estimate_start)");
  if (!h->have_intr) return fail(CC_ERR_STATE, "cc_rigk_estimate_start: cc_rigk_set_intrinsics has not been called (or not since cc_rigk_set_model changed the model): the pixels need the start intrinsics");
  return rig_start_run(h, "cc_rigk_estimate_start", RIG_START_PIXELS, opt, cam_q, cam_t, frame_q, frame_t, report);
}

int cc_rigk_start_points(cc_rig* h, float* uv_normalised, int64_t* n_without_root) {
  using namespace cc;
  if (!h) return fail(CC_ERR_BAD_ARGUMENT, "cc_rigk_start_points: NULL handle");
  if (h->st_have_bearings) return fail(CC_ERR_STATE, "cc_rigk_start_points: the handle's last start was cc_rigk_estimate_start_bearing (it makes bearings, not points: cc_rigk_start_bearings)");
  if (!h->st_have_points) return fail(CC_ERR_STATE, "cc_rigk_start_points: cc_rigk_estimate_start has not run on this handle");
  CC_HIP(hipSetDevice(h->device));
  CC_HIP(hipStreamSynchronize(h->stream));
  std::vector<float> sorted((size_t)h->N * 2);
  if (h->N > 0) CC_HIP(hipMemcpy(sorted.data(), h->st_points, sorted.size() * sizeof(float), hipMemcpyDeviceToHost));
  int64_t bad = 0;
  for (int64_t i = 0; i < h->N; ++i) bad += (sorted[(size_t)2 * i] != sorted[(size_t)2 * i]) ? 1 : 0;   // (NaN comes in pairs)
  if (n_without_root) *n_without_root = bad;
  if (uv_normalised) {
    if (h->perm_inverse) {   // (a handle made from columns: positions inside the frame)
      const int32_t* rel = reinterpret_cast<const int32_t*>(h->perm.data());
      for (int64_t f = 0; f < h->F; ++f) {
        const int64_t a = h->goff_h[(size_t)h->fgoff_h[(size_t)f]], b = h->goff_h[(size_t)h->fgoff_h[(size_t)f + 1]];
        for (int64_t i = a; i < b; ++i) for (int j = 0; j < 2; ++j) uv_normalised[2 * i + j] = sorted[(size_t)2 * (a + rel[i]) + j];
      }
    } else {
      const int64_t* perm = h->perm.data();
      for (int64_t i = 0; i < h->N; ++i) for (int j = 0; j < 2; ++j) uv_normalised[2 * perm[i] + j] = sorted[(size_t)2 * i + j];
    }
  }
  return CC_OK;
}

// EXTENSION: the pixel start on unit bearings, for points at and beyond 90 degrees off the axis (cc_rigk_start.hpp)
int cc_rigk_estimate_start_bearing(cc_rig* h, const cc_rig_start_options* opt, const double* cam_q, const double* cam_t, const double* frame_q,
                                   const double* frame_t, cc_rig_start_report* report) {
  using namespace cc;
  if (!h) return fail(CC_ERR_BAD_ARGUMENT, "cc_rigk_estimate_start_bearing: NULL handle");
  if (!h->d.kmode) return fail(CC_ERR_STATE, "cc_rigk_estimate_start_bearing: the handle was created without intrinsics (cc_rig_create: its observations are normalised image points, cc_rig_estimate_start)");
  if (!h->have_intr) return fail(CC_ERR_STATE, "cc_rigk_estimate_start_bearing: cc_rigk_set_intrinsics has not been called (or not since cc_rigk_set_model changed the model): the pixels need the start intrinsics");
  return rig_start_run(h, "cc_rigk_estimate_start_bearing", RIG_START_BEARINGS, opt, cam_q, cam_t, frame_q, frame_t, report);
}

int cc_rigk_start_bearings(cc_rig* h, float* bearing_xyz, int64_t* n_without_root) {
  using namespace cc;
  if (!h) return fail(CC_ERR_BAD_ARGUMENT, "cc_rigk_start_bearings: NULL handle");
  if (!h->st_have_bearings) return fail(CC_ERR_STATE, "cc_rigk_start_bearings: cc_rigk_estimate_start_bearing has not run on this handle (or cc_rigk_estimate_start has since)");
  CC_HIP(hipSetDevice(h->device));
  CC_HIP(hipStreamSynchronize(h->stream));
  std::vector<float> sorted((size_t)h->N * 3);
  if (h->N > 0) CC_HIP(hipMemcpy(sorted.data(), h->st_bearings, sorted.size() * sizeof(float), hipMemcpyDeviceToHost));
  int64_t bad = 0;
  for (int64_t i = 0; i < h->N; ++i) bad += (sorted[(size_t)3 * i] != sorted[(size_t)3 * i]) ? 1 : 0;   // (NaN comes in threes)
  if (n_without_root) *n_without_root = bad;
  if (bearing_xyz) {
    if (h->perm_inverse) {   // (a handle made from columns: positions inside the frame)
      const int32_t* rel = reinterpret_cast<const int32_t*>(h->perm.data());
      for (int64_t f = 0; f < h->F; ++f) {
        const int64_t a = h->goff_h[(size_t)h->fgoff_h[(size_t)f]], b = h->goff_h[(size_t)h->fgoff_h[(size_t)f + 1]];
        for (int64_t i = a; i < b; ++i) for (int j = 0; j < 3; ++j) bearing_xyz[3 * i + j] = sorted[(size_t)3 * (a + rel[i]) + j];
      }
    } else {
      const int64_t* perm = h->perm.data();
      for (int64_t i = 0; i < h->N; ++i) for (int j = 0; j < 3; ++j) bearing_xyz[3 * perm[i] + j] = sorted[(size_t)3 * i + j];
    }
  }
  return CC_OK;
}

int cc_rig_start_views(cc_rig* h, int64_t* n_views, int32_t* view_cam, int64_t* view_frame, int32_t* kind, double* q, double* t, double* rms2) {
  using namespace cc;
  if (!h || !n_views) return fail(CC_ERR_BAD_ARGUMENT, "cc_rig_start_views: NULL argument");
  if (!h->st_views) return fail(CC_ERR_STATE, "cc_rig_start_views: cc_rig_estimate_start has not run on this handle");
  *n_views = h->NG;
  CC_HIP(hipSetDevice(h->device));
  CC_HIP(hipStreamSynchronize(h->stream));
  if (kind) CC_HIP(hipMemcpy(kind, h->st.kind, (size_t)h->NG * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (q || t || rms2) {
    std::vector<double> v((size_t)h->NG * kRigViewStride);
    CC_HIP(hipMemcpy(v.data(), h->st.view, v.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t g = 0; g < h->NG; ++g) {
      const double* r = v.data() + g * kRigViewStride;
      if (q) for (int i = 0; i < 4; ++i) q[g * 4 + i] = r[i];
      if (t) for (int i = 0; i < 3; ++i) t[g * 3 + i] = r[4 + i];
      if (rms2) rms2[g] = r[7];
    }
  }
  for (int64_t g = 0; g < h->NG; ++g) {
    if (view_cam) view_cam[g] = h->gcam_h[(size_t)g];
    if (view_frame) view_frame[g] = h->gframe_h[(size_t)g];
  }
  return CC_OK;
}

}  // extern "C"
