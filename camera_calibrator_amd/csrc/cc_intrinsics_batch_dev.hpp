// cc_intrinsics_batch_dev.hpp -- what the translation units of the batched intrinsics solve share: the device view of a
// batch (cc_intrinsics_batch.hip, which owns it) and the interfaces of the robust form of its sweep
// (cc_intrinsics_batch_huber.hip) and of the fisheye model's sweep (cc_intrinsics_batch_fisheye.hip).
#pragma once
#include "cc_common.hpp"

namespace cc {

struct IntrBatchDev {
  int64_t N;               // observations of all problems
  int32_t B, Ftot;         // problems, frames of all problems
  const float* uv;
  const float* xyz;
  const int64_t* off;      // [Ftot + 1] frame -> observations
  const int2* where;       // [Ftot] sweep workgroup -> {problem, local frame}
  const int32_t* first;    // [B + 1] problem -> frames
  const uint32_t* mask;    // [B]
  double* intr;            // [B][2][16]
  double* pose;            // [2][Ftot][8]
  double* blocks;          // [2][Ftot][256]
  double* stats;           // [Ftot][4]
  double* hd0;             // [Ftot][16] diag of H_ss at the initial point (Jacobi scaling)
  double* sp;              // [Ftot][8]  Jacobi scale of the pose block
  double* Y;               // [Ftot][64]
  double* ds;              // [B][16] scaled shared step
  double* ss;              // [B][16] Jacobi scale of the shared block
  LmCtl* ctl;              // [B]
  const LmOpts* opts;      // one set of options for the whole batch
  cc_iteration* log;       // [log_cap][B]: record r of problem p at r * B + p (one transfer reads the used rows of all)
  int32_t log_cap, pad_;
};

// EXTENSION (cc_intrinsics_batch_huber.hip): the batch sweep with ceres::HuberLoss(huber_a[p]) for problem p, huber_a [B] in
// device memory; the workgroups of a problem with huber_a[p] <= 0 return at once (k_intrb_sweep sweeps those). Same grid, block
// and LDS as k_intrb_sweep.
int batch_sweep_huber_prepare();   // once per handle, behind the device selection
void batch_sweep_huber_launch(const IntrBatchDev& P, const double* huber_a, hipStream_t stream);

// EXTENSION (cc_intrinsics_batch_fisheye.hip): the batch sweep of the fisheye model, for a handle whose model is
// CC_MODEL_FISHEYE. It sweeps EVERY problem (huber_a[p] <= 0: the loss with a = +inf, weight exactly 1), so such a handle
// launches it alone each round. Same grid, block and LDS as k_intrb_sweep.
int batch_sweep_fisheye_prepare();   // once per handle, behind the device selection
void batch_sweep_fisheye_launch(const IntrBatchDev& P, const double* huber_a, hipStream_t stream);

}  // namespace cc
