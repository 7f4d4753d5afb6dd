#pragma once
#include "cc_common.hpp"

// cc_rig_inner.hpp / cc_rig_inner.hip -- Ceres' inner iterations (CoordinateDescentMinimizer) on the rig problem, poses only.
// The kernels are a translation unit of their own; cc_rig.hip launches them through the functions declared here.
//
// One inner pass visits the parameter blocks group by group, in the order Ceres' CreateOrdering gives for this graph
// (DESIGN.md section 2): every camera's t_cr, every camera's q_cr, every frame's t_rw, every frame's q_rw. Blocks of a group
// share no residual, so each is minimised on its own with the others held: a trust-region LM with Ceres' default
// Solver::Options (monotonic, 50 iterations, Jacobi scaling taken at its first iteration) over the residuals that touch it.
// Ceres solves each block with DENSE_QR; here the 3 x 3 normal equations (the same step up to rounding).
//
// One workgroup per block runs that block's whole mini-solve: every evaluation sweeps the block's observations (residual,
// 2 x 3 Jacobian, Huber corrector: the arithmetic of rig_common / huber and of the rows of k_rig_sweep_frame), reduces cost,
// gradient and the 3 x 3 Gram in a fixed order (no atomics: repeatable bit for bit), and thread 0 takes the LM decision with
// lm_decide (cc_common.hpp) on its own LmCtl. Nothing waits for another workgroup.
//
// Outer loop (TrustRegionMinimizer::DoInnerIterationsIfNeeded), three-kernel form only, between the candidate's sweep and the
// elimination of rig_enqueue_round: k_rig_inner_begin (run the pass? candidate cost, model term) -> the four group launches on
// the candidate buffers -> k_rig_inner_records (records of the new candidate) -> the sweep again -> k_rig_inner_decide (the
// decision with the augmented model; the elimination then finds no pending candidate and eliminates at the decided point).

namespace cc {

enum { RIG_IN_ENABLED = 0, RIG_IN_TOL, RIG_IN_RUN, RIG_IN_CAND, RIG_IN_QMODEL, RIG_IN_PASSES, RIG_IN_USEFUL, RIG_IN_REMOVED, RIG_IN_WORDS = 16 };

// what the kernels read of a rig handle (cc_rig.hip: RigDev, the same buffers)
struct RigInnerDev {
  int64_t F, NG;
  int32_t C, fmode;
  const float* uv;          // [N] float2, (frame, camera)-sorted
  const float* oxyz;        // [3N] world point of every observation
  const int64_t* goff;      // [NG+1]
  const int32_t* gframe;    // [NG]
  const int32_t* gcam;      // [NG]
  const int64_t* fgoff;     // [F+1]
  const int32_t* cam_goff;  // [C+1]
  const int32_t* cam_glist; // [NG]
  const int32_t* pcol;      // [C] -1: camera held constant
  double* cam;              // [2][C][8]
  double* pose;             // [2][F][8]
  double* camrec;           // [C][32] R(9) t(3) unscaled step(6)
  double* frec;             // [F][32]
  const double* gstats;     // [NG or F][2] cost, model term of the last sweep
  LmCtl* ctl;
  LmCtl* ctl_next;
  const LmOpts* opts;
  cc_iteration* log;
  int32_t log_cap;
  double huber_a;
  double* st;        // [RIG_IN_WORDS] enabled, tolerance, run (this round), candidate cost, model term, passes, useful passes, cost removed
  int32_t* iters;    // [2C + 2F] iterations of each block's mini-solve in the last pass (t_cr | q_cr | t_rw | q_rw)
};

// the four groups of one pass, in Ceres' order (buf >= 0: on that buffer; buf < 0: on a solve round's candidate)
void rig_inner_enqueue_groups(const RigInnerDev& I, hipStream_t s, int buf);
// the outer-loop hook around the second sweep: begin + groups + records, then (after the caller's sweep) the decision
void rig_inner_enqueue_before_sweep(const RigInnerDev& I, hipStream_t s);
void rig_inner_enqueue_decide(const RigInnerDev& I, hipStream_t s);

}  // namespace cc
