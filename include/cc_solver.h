/*
 * cc_solver.h -- C ABI of the MI355X-native reprojection-error LM solver.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  It replaces, for
 * the hot path only, what the reference builds out of ceres::Problem / ceres::Solve:
 *   - cc_intrinsics_*  <->  Calibrator::Optimize            (/root/reference/src/calibrator.cpp:221-336)
 *   - cc_rig_*         <->  ExtrinsicsCalibrator::Optimize  (/root/reference/src/extrinsics_calibrator.cpp:86-257)
 *   - cc_distort / cc_undistort <-> Calibrator::Distort / Undistort (calibrator.cpp:118-166)
 * The C++ classes in camera_calibrator_amd/csrc/ (same names and signatures as the reference's
 * calibrator.hh / extrinsics_calibrator.hh) call these entry points; INTEGRATION.md shows the
 * binding a maintainer of the reference would add.
 *
 * All entry points return 0 on success or a negative cc_status; cc_last_error() gives text.
 * The library is HIP-only: there is no CPU fallback, every compute entry point fails with
 * CC_ERR_NO_DEVICE when no gfx950 device is usable.
 *
 * Conventions (identical to the reference): intrinsics order fx fy px py k1 k2 p1 p2 k3
 * (calibrator.cpp:168-179); quaternions w x y z (calibrator.cpp:277-278); observations and 3-D
 * points are float32 as the reference API stores them (types.hh:10-15); parameters are fp64.
 */
#ifndef CC_SOLVER_H
#define CC_SOLVER_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum cc_status {
  CC_OK = 0,
  CC_ERR_BAD_ARGUMENT = -1,
  CC_ERR_NO_DEVICE = -2,
  CC_ERR_HIP = -3,
  CC_ERR_COMM = -4,
  CC_ERR_STATE = -5
} cc_status;

/* Termination reasons (mirror Ceres' TerminationType + message for this path). */
enum {
  CC_NO_CONVERGENCE = 0,       /* max_iterations reached */
  CC_CONVERGENCE_GRADIENT = 1,
  CC_CONVERGENCE_PARAMETER = 2,
  CC_CONVERGENCE_FUNCTION = 3,
  CC_FAILURE_INVALID_STEPS = 4,
  CC_MIN_RADIUS = 5,
  CC_FAILURE_EXCHANGE = 6      /* multi-GPU mailbox exchange timed out (solve returns CC_ERR_COMM) */
};

/* Solver options.  cc_options_init() sets the Ceres 2.x defaults overlaid with what the
 * reference sets at calibrator.cpp:314-321 (non-monotonic steps, 100 iterations). Tolerances
 * < 0 disable the corresponding test. */
typedef struct cc_options {
  int32_t max_iterations;                     /* 100 (calibrator.cpp:319); rig default 1000 (extrinsics_calibrator.cpp:211) */
  int32_t use_nonmonotonic_steps;             /* 1 (calibrator.cpp:315) */
  int32_t max_consecutive_nonmonotonic_steps; /* 5 */
  int32_t jacobi_scaling;                     /* 1 */
  int32_t max_consecutive_invalid_steps;      /* 5 */
  int32_t check_interval;                     /* LM iterations enqueued per host poll of the device 'done' flag (4) */
  double function_tolerance;                  /* 1e-6 */
  double gradient_tolerance;                  /* 1e-10 */
  double parameter_tolerance;                 /* 1e-8 */
  double initial_radius;                      /* 1e4 */
  double max_radius;                          /* 1e16 */
  double min_radius;                          /* 1e-32 */
  double min_relative_decrease;               /* 1e-3 */
  double min_lm_diagonal;                     /* 1e-6 */
  double max_lm_diagonal;                     /* 1e32 */
  int32_t use_graph;                          /* 1: replay a captured hipGraph of check_interval iterations */
  int32_t profile_kernels;                    /* 1: bracket every kernel launch with hipEvents (implies no graph) */
} cc_options;

typedef struct cc_iteration {
  double cost;
  double cost_change;
  double model_cost_change;
  double relative_decrease;
  double gradient_max_norm;   /* Ceres': ||x - Plus(x, -g)||_inf (pose blocks with |g_rot| >= 1/4: tangent max-norm) */
  double step_norm;
  double radius;
  int32_t accepted;
  int32_t valid;
} cc_iteration;

enum { CC_K_SWEEP = 0, CC_K_DECIDE = 1, CC_K_ELIM = 2, CC_K_SOLVE = 3, CC_K_ALLREDUCE = 4, CC_K_UPDATE = 5, CC_K_REDUCE = 6, CC_K_COUNT = 8 };

typedef struct cc_summary {
  int32_t iterations;        /* LM iterations executed (accepted + rejected + invalid) */
  int32_t successful_steps;
  int32_t termination;
  int32_t log_len;
  double initial_cost;
  double final_cost;
  double seconds;            /* host wall time of the solve call, device work included */
  cc_iteration* log;         /* caller-provided buffer (may be NULL) */
  int32_t log_capacity;
  int32_t sweeps;            /* Jacobian sweeps launched (1 initial + 1 per valid LM iteration) */
  /* profile_kernels=1 only: per-kernel device time from hipEvents on the solver's stream */
  double kernel_ms[CC_K_COUNT];      /* total ms per kernel kind, over the launches that DID WORK (see kernel_idle_*) */
  int32_t kernel_launches[CC_K_COUNT];
  /* the launches of the last chunk that came after the terminating decision and returned at once (rounds are enqueued
   * check_interval at a time): kept apart so that kernel_ms / kernel_launches is the time of a launch that does work */
  double kernel_idle_ms[CC_K_COUNT];
  int32_t kernel_idle_launches[CC_K_COUNT];
} cc_summary;

void cc_options_init(cc_options* o);
const char* cc_last_error(void);
/* Pinned host memory, cached between calls, for a caller that packs its inputs itself (the C++ classes do: one memcpy per frame
 * of the reference's vector<Points2D> / vector<Points3D> arguments, calibrator.cpp:261-292). Optional: every entry point takes
 * any host pointer. Returns NULL when the allocation fails. */
void* cc_host_staging_acquire(size_t bytes);
void cc_host_staging_release(void* p);
/* Wall milliseconds of the phases of this thread's last cc_intrinsics_estimate / cc_intrinsics_optimize:
 * [0] handle + device arena, [1] upload, [2] Zhang initialisation (estimate only), [3] solve, [4] read-back + teardown. */
void cc_last_call_timing(double out_ms[5]);
const char* cc_version(void);
/* The library keeps a few things between calls so that a caller that re-estimates as images arrive (the reference's workflow
 * builds a fresh solver per call: cam_calibration.py:290-322) does not pay for allocation every time. What is retained, at most:
 * per device four arena pieces (the device memory of a solver handle, each <= 1.25 GB) and pooled device blocks up to 8 GB, one
 * 64 MB scratch block; per process four pinned host staging pieces (each <= 1.25 GB), a few 512-byte pinned blocks, streams, the
 * host worker threads (cc_parallel_for) and the regrouping arrays of the last rig call. This gives the idle ones back (safe at
 * any time from any thread; pieces in use by a running call stay; the next call allocates / starts them again). */
void cc_release_caches(void);
/* Solver form and reruns of this thread's LAST one-shot call (cc_intrinsics_estimate / _optimize / _views / _multi,
 * cc_rig_optimize / _frames / _multi): these calls destroy their handles before returning, so cc_*_solver_status cannot be asked.
 * form: 0 several kernels per iteration, 1 / 2 / 4 the persistent per-solve kernel; reruns > 0: a persistent solve gave up
 * (workgroups not co-resident: another tenant, a tool that serialises kernels, a host thread inside a device-wide runtime call)
 * and the solve was run again in the several-kernel form -- late by 10 ms (intrinsics) / 42 ms (rig) when the first round never
 * came together, 1.3 s in a later round; equal to rounding; note says what the kernel reported. form is what the solve RAN in.
 * A give-up is remembered per device and process, not per handle (these calls make a new handle every time): the next 8 solves
 * AND 2 s on that device do not try the persistent form at all (form 0, reruns 0), then ONE solve probes it; a probe that gives
 * up doubles the window (at most 1024 solves / 10 min), one that completes ends it. The C++ classes expose this as
 * LastSolverReruns() / LastSolverNote() / LastSolverForm(). */
int cc_last_call_solver_status(int32_t* form, int32_t* reruns, char* note, int32_t note_capacity);
/* The library's host worker pool, for a caller's own parallel phases (the C++ classes flatten / fill their arrays with it,
 * extrinsics_calibrator.cpp): fn(ctx, part) for part = 0 .. parts - 1, part 0 on the calling thread, returns when all are done.
 * The threads are created at first use (at most 15), kept for the life of the process, joined by cc_release_caches.
 * One job at a time (a second host thread waits its turn). Re-entry is allowed: a cc_parallel_for -- or any library call that
 * uses the pool (cc_rig_optimize*, cc_rig_get_state) -- made FROM a part runs its parts inline on that thread, one after the
 * other, and cc_release_caches called from a part leaves the pool's threads alone.
 * cc_parallel_parts: how many parts the library itself would use for n items of which a part should hold min_per_part. */
void cc_parallel_for(int32_t parts, void (*fn)(void* ctx, int32_t part), void* ctx);
int32_t cc_parallel_parts(int64_t n, int64_t min_per_part);
int32_t cc_host_pool_threads(void);
/* Number of usable HIP devices (0 if none); never touches the oracle or a CPU path. */
int cc_device_count(void);

/* ---------------------------------------------------------------------------------------------
 * Single-camera intrinsics problem: 9 shared intrinsics + one (q,t) pose per frame.
 * Frames are ragged: frame f owns observations [frame_offsets[f], frame_offsets[f+1]).
 * ------------------------------------------------------------------------------------------- */
typedef struct cc_intrinsics cc_intrinsics;

/* Uploads the observations to HBM (device `device`, a stream of its own). uv: 2N floats (pixels),
 * xyz: 3N floats. */
int cc_intrinsics_create(int32_t device, int64_t n_frames, const int64_t* frame_offsets,
                         const float* uv, const float* xyz, cc_intrinsics** out);
void cc_intrinsics_destroy(cc_intrinsics* h);

/* Sets the current parameters (and remembers them as the initial state for cc_intrinsics_reset).
 * const_mask bit i freezes intrinsic i (ForceDistortionToConstant(d) -> bit d+4, calibrator.cpp:338-340). */
int cc_intrinsics_set_state(cc_intrinsics* h, const double* intr9, uint32_t const_mask,
                            const double* q_wxyz, const double* t_xyz);
int cc_intrinsics_reset(cc_intrinsics* h); /* device-side copy back to the last set_state */
int cc_intrinsics_get_state(cc_intrinsics* h, double* intr9, double* q_wxyz, double* t_xyz);

/* One Jacobian sweep at the current state: per-frame 16x16 Gram blocks
 * G_f = sum_rows v v^T, v = [J_intr(9) J_pose(6) r] (row-major, blocks may be NULL) and the
 * total cost 1/2 sum r^2. */
int cc_intrinsics_eval(cc_intrinsics* h, double* blocks, double* cost);

/* Runs the LM loop on the device from the current state (replaces the ceres::Solve call, calibrator.cpp:323-324).
 * Two forms, same arithmetic, chosen when the handle is created (cc_intrinsics_solver_form):
 *   persistent -- ONE kernel launch per solve: every frame keeps a team of a resident workgroup for the whole solve
 *     (pose, Gram blocks and back-substitution matrix in LDS), a control workgroup takes the trust-region decisions;
 *     used whenever every frame fits a resident team (<= 4 frames per compute unit: 1020 frames on an MI355X) and the
 *     device is the solve's own; CC_INTR_PERSIST=0 disables it;
 *   two kernels per LM iteration (sweep, decide + eliminate + solve), replayed from a captured graph -- any size. */
int cc_intrinsics_solve(cc_intrinsics* h, const cc_options* opt, cc_summary* summary);
/* 0: two kernels per iteration; 1, 2, 4: the persistent kernel with that many frames per workgroup. With an exchange
 * attached the answer is what the ranks agreed on (cc_intrinsics_exchange_attach). */
int cc_intrinsics_solver_form(cc_intrinsics* h);
/* The same, with the history of the handle: *reruns = persistent solves that gave up (a wait inside the kernel timed out:
 * not every workgroup resident) and were run again in the two-kernel form, which the handle then keeps; note = what the
 * last one reported (NUL-terminated, truncated to note_capacity). Any output may be NULL. */
int cc_intrinsics_solver_status(cc_intrinsics* h, int32_t* form, int32_t* reruns, char* note, int32_t note_capacity);

/* Measurement aid: launches `n` steady-state Jacobian sweeps (candidate step + sweep, exactly the
 * kernel an LM iteration runs) back to back on the solver's stream between two hipEvents and
 * returns the average ms per launch. Needs a completed cc_intrinsics_solve with >= 1 iteration.
 * The accepted point is left untouched. */
int cc_intrinsics_profile_sweep(cc_intrinsics* h, int32_t n, double* avg_ms);
/* Measurement aid for the persistent form (one launch = one complete solve): runs `n` solves from the state of the
 * last set_state, each launch bracketed by two hipEvents on the solver's stream; returns the average ms per launch
 * and the evaluations (initial + one per LM iteration) a launch made. CC_ERR_STATE when the handle does not use the
 * persistent form or has an exchange attached. */
int cc_intrinsics_profile_solve(cc_intrinsics* h, const cc_options* opt, int32_t n, double* avg_launch_ms, int32_t* sweeps_per_launch);

/* One-shot convenience: create + set_state + solve + get_state + destroy. This is the call
 * Calibrator::Optimize makes in place of calibrator.cpp:236-324. */
int cc_intrinsics_optimize(const cc_options* opt, int32_t device, int64_t n_frames,
                           const int64_t* frame_offsets, const float* uv, const float* xyz,
                           double* intr9, uint32_t const_mask, double* q_wxyz, double* t_xyz,
                           cc_summary* summary);

/* Calibrator::Estimate in one call (calibrator.cpp:47-68: Zhang initialisation, then Optimize): the observations are
 * uploaded once, cc_zhang_init's kernels run on the handle's device copies, and the solve starts from their K and poses
 * rounded to float -- exactly what the two calls cc_zhang_init + cc_intrinsics_optimize exchange through the class
 * members, so the results are identical. distortion5 (k1 k2 p1 p2 k3) = the object's current distortion (may be NULL:
 * zeros); K_init9 (may be NULL) receives Zhang's K; intr9 / q_wxyz [4F] / t_xyz [3F] receive the optimised state.
 * Needs >= 3 frames with >= 4 points each. */
int cc_intrinsics_estimate(const cc_options* opt, int32_t device, int64_t n_frames, const int64_t* frame_offsets,
                           const float* uv, const float* xyz, const double* distortion5, uint32_t const_mask,
                           float* K_init9, double* intr9, double* q_wxyz, double* t_xyz, cc_summary* summary);
/* The same for views given as separate arrays, the shape of the reference's arguments (vector<Points2D> / vector<Points3D>,
 * calibrator.cpp:47-68): view i has counts[i] points, uv_views[i] = 2 floats per point, xyz_views[i] = 3. The library packs
 * the views into cached pinned memory in pieces and uploads each piece while it packs the next. */
int cc_intrinsics_estimate_views(const cc_options* opt, int32_t device, int64_t n_frames, const float* const* uv_views,
                                 const float* const* xyz_views, const int64_t* counts, const double* distortion5,
                                 uint32_t const_mask, float* K_init9, double* intr9, double* q_wxyz, double* t_xyz,
                                 cc_summary* summary);
/* cc_intrinsics_optimize for views given as separate arrays (Calibrator::Optimize's arguments, calibrator.cpp:70-74). */
int cc_intrinsics_optimize_views(const cc_options* opt, int32_t device, int64_t n_frames, const float* const* uv_views,
                                 const float* const* xyz_views, const int64_t* counts, double* intr9, uint32_t const_mask,
                                 double* q_wxyz, double* t_xyz, cc_summary* summary);

/* Multi-GPU inside ONE process, ONE host thread (SURVEY.md 8(b) thread model): the one-shot call over several
 * devices. Frames are sharded contiguously by observation count (cc_partition_frames), one handle + stream per
 * device, the per-iteration exchange (112 + 16 doubles) goes through mailboxes in peer HBM wired inside the process
 * (hipDeviceEnablePeerAccess, no hipIpc), every device's launches are enqueued before any device is waited for.
 * devices[i] may repeat (several shards on one GPU). n_devices 1..8; with 1 it is cc_intrinsics_optimize.
 * Calibrator::SetDevices selects it behind the class surface. */
int cc_intrinsics_optimize_multi(const cc_options* opt, int32_t n_devices, const int32_t* devices,
                                 int64_t n_frames, const int64_t* frame_offsets, const float* uv,
                                 const float* xyz, double* intr9, uint32_t const_mask, double* q_wxyz,
                                 double* t_xyz, cc_summary* summary);

/* Multi-GPU: one process per GPU, each owning a contiguous shard of frames. Rank 0 calls
 * cc_comm_get_unique_id and broadcasts the 128 bytes (e.g. over torch.distributed); every rank
 * then attaches its handle. Per LM iteration the handles all-reduce (RCCL, sum, fp64) only the
 * reduced shared-parameter blocks (64 doubles after elimination, 64 after the sweep). */
int cc_comm_get_unique_id(uint8_t id[128]);
int cc_intrinsics_comm_init(cc_intrinsics* h, const uint8_t id[128], int32_t rank, int32_t nranks);

/* Multi-GPU within one node, without a collective library in the loop (preferred for <= 8 ranks):
 * the two reductions of an iteration are <= 1 KB and purely latency-bound, so every rank STORES its
 * partial sums straight into a mailbox in each peer's HBM over xGMI and the consumer kernels wait
 * on flags in their own memory (cc_device.hpp). The iteration stays three/four kernels inside one
 * captured graph. Protocol: every rank calls _export (allocates the mailbox, returns its 64-byte
 * hipIpcMemHandle), the caller all-gathers the handles over its control plane (rank order), every
 * rank calls _attach with all nranks*64 bytes (COLLECTIVE for nranks > 1: the ranks agree, through the mailboxes,
 * on the form of the solver they all run; a peer that does not attach within 10 s -> CC_ERR_COMM). All ranks must then call cc_intrinsics_solve /
 * cc_intrinsics_reset the same number of times with the same options. A peer that does not show
 * up within 10 s makes the solve return CC_ERR_COMM (termination CC_FAILURE_EXCHANGE) instead of
 * hanging. Keep the handle alive until every rank has finished its last solve. */
int cc_intrinsics_exchange_export(cc_intrinsics* h, uint8_t handle[64]);
int cc_intrinsics_exchange_attach(cc_intrinsics* h, int32_t rank, int32_t nranks, const uint8_t* handles);

/* ---------------------------------------------------------------------------------------------
 * EXTENSION (the reference's Calibrator::Optimize sets no loss function, calibrator.cpp:236-324; the rig path has carried
 * Ceres' HuberLoss from the start): ceres::HuberLoss(a) with its Corrector for the single-camera solve, a in PIXELS, off by
 * default. Per observation s = ru^2 + rv^2; rho(s) = s for s <= a^2, else 2 a sqrt(s) - a^2; cost = 1/2 sum rho(s); the
 * observation's two Jacobian rows and its residual are multiplied by sqrt(rho'(s)) (1 up to a^2, sqrt(a / sqrt(s)) beyond;
 * rho'' <= 0, so the Corrector has no second-order term). One mis-detected corner then pulls K and the distortion with a
 * bounded force. a <= 0: off (every entry point returns the bits it returned before the loss existed); NaN:
 * CC_ERR_BAD_ARGUMENT; +inf: allowed, no observation is ever in the tail. A non-finite residual still makes the cost
 * non-finite and ends the solve as it does with the loss off.
 * Out of scope: the persistent per-solve kernel, every multi-GPU form, losses other than Huber.
 * ------------------------------------------------------------------------------------------- */
/* Applies to later cc_intrinsics_eval / _solve / _obs_cost calls. With a > 0 the handle solves in the two-kernel form by choice
 * (cc_intrinsics_solver_form reports 0; no give-up, no device back-off entry, reruns stays 0) and a captured graph is dropped;
 * a <= 0 gives the handle back the form it had. CC_ERR_STATE on a handle with an exchange or communicator attached;
 * cc_intrinsics_exchange_export / _attach, cc_intrinsics_comm_init and cc_intrinsics_profile_solve return CC_ERR_STATE on a
 * handle with the loss on. */
int cc_intrinsics_set_huber(cc_intrinsics* h, double a_pixels);
/* The sweep of the LAST round of a solve in the persistent form. A decision that ends a solve reads the candidate's cost and
 * nothing else of its sweep; where the control predicts such a decision (iteration limit: certain; function tolerance: from the
 * last two accepted cost changes) the workers evaluate residuals only, and sweep again in full should the solve go on.
 * mode 0: every sweep full; 1: as described (the default); 2: predicted at every accepting decision (tests). The results are
 * the same bits in every mode. Other values: CC_ERR_BAD_ARGUMENT. */
int cc_intrinsics_set_final_sweep(cc_intrinsics* h, int32_t mode);
/* Of the last persistent solve of the handle: rounds swept residual-only, and how many of those were swept again in full. Waits
 * for the handle's stream. Zeros before the first such solve; a solve in the two-kernel form leaves them alone. */
int cc_intrinsics_final_sweep_counts(cc_intrinsics* h, int32_t* residual_only, int32_t* redone);
/* obs_cost [N]: the cost of every observation at the current point, in the caller's order -- 1/2 rho(s) with the loss on,
 * 1/2 s with it off. */
int cc_intrinsics_obs_cost(cc_intrinsics* h, double* obs_cost);
/* cc_intrinsics_optimize_views / cc_intrinsics_estimate_views with a trailing huber_a (those two ARE these with 0). */
int cc_intrinsics_optimize_views_huber(const cc_options* opt, int32_t device, int64_t n_frames, const float* const* uv_views,
                                       const float* const* xyz_views, const int64_t* counts, double* intr9, uint32_t const_mask,
                                       double* q_wxyz, double* t_xyz, cc_summary* summary, double huber_a);
int cc_intrinsics_estimate_views_huber(const cc_options* opt, int32_t device, int64_t n_frames, const float* const* uv_views,
                                       const float* const* xyz_views, const int64_t* counts, const double* distortion5,
                                       uint32_t const_mask, float* K_init9, double* intr9, double* q_wxyz, double* t_xyz,
                                       cc_summary* summary, double huber_a);

/* ---------------------------------------------------------------------------------------------
 * EXTENSION (the reference calibrates one lens model, pinhole + radial-tangential distortion, calibrator.cpp:70-95): the
 * Kannala-Brandt / OpenCV `fisheye` model for the single-camera solve, for lenses past ~100 degrees of field of view where the
 * polynomial in r = tan(theta) diverges. For a point (xc, yc, zc) = R(q) X + t in the camera frame:
 *   rho = sqrt(xc^2 + yc^2), theta = atan2(rho, zc), theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8),
 *   u = fx theta_d xc / rho + px, v = fy theta_d yc / rho + py        (residuals in pixels; the limit value on the axis)
 * For zc > 0 this is cv::fisheye's atan(r); for zc <= 0 it stays finite and smooth. Slots of intr9: fx fy px py k1 k2 k3 k4 -;
 * slot 8 is unused: its bit of the constant mask is forced on and it reads back as 0.
 * The batch carries the model too (cc_intrinsics_batch_set_model below), and so does the rig solve with intrinsics
 * (cc_rigk_set_model). Out of scope: the persistent per-solve kernel, every
 * multi-GPU form, other models. cc_intrinsics_estimate_views_model starts from Zhang's pinhole K and poses with k = 0; a
 * start made for the lens is cc_intrinsics_estimate_start_fisheye below.
 * ------------------------------------------------------------------------------------------- */
enum { CC_MODEL_RADTAN = 0, CC_MODEL_FISHEYE = 1 };
/* The model of later cc_intrinsics_set_state / _eval / _solve / _reset / _get_state / _obs_cost calls; combines with
 * cc_intrinsics_set_huber. A fisheye handle solves in the two-kernel form by choice, like a handle with the loss on
 * (cc_intrinsics_solver_form reports 0; no give-up, no device back-off entry); cc_intrinsics_exchange_export / _attach,
 * cc_intrinsics_comm_init and cc_intrinsics_profile_solve return CC_ERR_STATE on it, and so does this call on a handle with an
 * exchange or communicator attached. A CHANGE of the model drops captured graphs and the state (the slots mean something
 * else): call cc_intrinsics_set_state next. Unknown model: CC_ERR_BAD_ARGUMENT. */
int cc_intrinsics_set_model(cc_intrinsics* h, int32_t model);
int32_t cc_intrinsics_get_model(cc_intrinsics* h);
/* The *_huber one-shot forms with a trailing model (those two ARE these with CC_MODEL_RADTAN). Fisheye: `distortion5` holds
 * four values, k1..k4. */
int cc_intrinsics_optimize_views_model(const cc_options* opt, int32_t device, int64_t n_frames, const float* const* uv_views,
                                       const float* const* xyz_views, const int64_t* counts, double* intr9, uint32_t const_mask,
                                       double* q_wxyz, double* t_xyz, cc_summary* summary, double huber_a, int32_t model);
int cc_intrinsics_estimate_views_model(const cc_options* opt, int32_t device, int64_t n_frames, const float* const* uv_views,
                                       const float* const* xyz_views, const int64_t* counts, const double* distortion5,
                                       uint32_t const_mask, float* K_init9, double* intr9, double* q_wxyz, double* t_xyz,
                                       cc_summary* summary, double huber_a, int32_t model);

/* ---------------------------------------------------------------------------------------------
 * EXTENSION (the reference starts every solve from Zhang's pinhole homographies, calibrator.cpp:47-66): a start of the FISHEYE
 * solve from the problem's own pixels, for lenses whose boards stand round the lens and beyond 90 degrees off its axis, where the
 * pinhole start puts the focal length and the centre far off and the solve takes several times the iterations or ends in a
 * wrong basin. A search over the focal length f of the equidistant lens r = f theta -- the fisheye model at
 * k = 0, fx = fy = f -- on the bearing form of the rig start (cc_rigk_estimate_start_bearing), on the device:
 *   1. centre c: `centre` when both coordinates are finite, else the midpoint of the bounding box of all finite pixels;
 *      r_max: the largest distance of a finite pixel from c.
 *   2. candidates j = 0 .. C-1: theta_j = theta_lo + j (theta_hi - theta_lo) / (C - 1) (C = 1: theta_lo), f_j = r_max / theta_j.
 *   3. searched views: all of them when search_views is 0 or >= F, else the S = search_views views floor(k F / S), k = 0 .. S-1.
 *   4. per (searched view, candidate), one wave: the float32 pixel into an fp64 bearing, d = uv - c, theta = |d| / f_j,
 *      b = (sin theta d / |d|, cos theta), the centre pixel (0, 0, 1); then the closed form from b x (P y~) = 0 and
 *      `refine_iterations` Levenberg-Marquardt steps on the chord p / |p| - b, the arithmetic of cc_rigk_estimate_start_bearing's
 *      views; cost = sum |p / |p| - b|^2 at the returned pose.
 *   5. S_j = f_j^2 sum_v cost_{j,v} over the searched views in index order (pixel units: without f_j^2 the chord favours long
 *      focal lengths). A candidate with a searched view it cannot place is disqualified, unless no candidate places that view.
 *      The smallest S_j among the qualified candidates wins, the lowest index on ties.
 *   6. every view's pose at the winner (the searched views come out again with the same bits).
 * The batch has the same start for all its problems at once (cc_intrinsics_batch_estimate_start_fisheye, below).
 * Out of scope: the radial-tangential model, estimating k or a non-square pixel
 * in the start, interpolation between candidates, multi-GPU handles, the persistent kernel; no entry point takes this start by
 * default, and the rig solve does not take its result by itself (cc_rigk_set_intrinsics is the caller's second call).
 * ------------------------------------------------------------------------------------------- */
typedef struct cc_intr_start_options {
  double centre[2];          /* NaN (either): the bounding box's midpoint */
  double theta_lo, theta_hi; /* the angle of the outermost pixel under the first and the last candidate: 0 < lo <= hi < pi */
  int32_t candidates;        /* 1 .. 64 */
  int32_t search_views;      /* 0: every view */
  int32_t refine_iterations; /* 0 .. 1000 */
} cc_intr_start_options;
/* NaN, NaN, 0.3, 3.0, 24, 32, 3 */
void cc_intr_start_options_init(cc_intr_start_options* o);
typedef struct cc_intr_start_report {
  double centre[2], r_max, focal;
  int32_t best_candidate, candidates_qualified;
  int64_t views, views_searched, views_invalid;
} cc_intr_start_report;
/* The start of a handle whose model is CC_MODEL_FISHEYE (any other handle, or one with an exchange or a communicator:
 * CC_ERR_STATE). opt NULL: the defaults; candidates, theta_lo / theta_hi, search_views or refine_iterations out of range:
 * CC_ERR_BAD_ARGUMENT. intr9 receives (f, f, c_x, c_y, 0, 0, 0, 0, 0), q_wxyz [4F] / t_xyz [3F] every view's pose; a view that
 * is invalid by its own data (fewer than 4 points, collinear points, a non-finite pixel or point) is counted in
 * report->views_invalid and gets q = (1, 0, 0, 0), t = 0. Every output may be NULL. No qualified candidate: CC_ERR_STATE, and
 * nothing is written. The handle's state is not touched -- cc_intrinsics_set_state comes next, as after cc_zhang_init. */
int cc_intrinsics_estimate_start_fisheye(cc_intrinsics* h, const cc_intr_start_options* opt, double* intr9, double* q_wxyz,
                                         double* t_xyz, cc_intr_start_report* report);
/* The last search of the handle: f [C], score [C] (S_j), qualified [C] (each may be NULL). CC_ERR_STATE before any start. */
int cc_intrinsics_start_scores(cc_intrinsics* h, double* f, double* score, int32_t* qualified);
/* cc_intrinsics_estimate_views_model with the start chosen. start NULL: that call, bit for bit (Zhang). Otherwise the model must
 * be CC_MODEL_FISHEYE (CC_ERR_BAD_ARGUMENT), the start above replaces Zhang's, the distortion starts from `distortion5`'s four
 * values (NULL: zeros), and K_init9 receives (f, 0, c_x; 0, f, c_y; 0, 0, 1). A view without a pose at the winner:
 * CC_ERR_BAD_ARGUMENT, the message names the first such view (views of fewer than 4 points included: the start, not the
 * packing, refuses them); no qualified candidate: CC_ERR_BAD_ARGUMENT too (there is no handle whose state it could be). */
int cc_intrinsics_estimate_views_start(const cc_options* opt, int32_t device, int64_t n_frames, const float* const* uv_views,
                                       const float* const* xyz_views, const int64_t* counts, const double* distortion5,
                                       uint32_t const_mask, float* K_init9, double* intr9, double* q_wxyz, double* t_xyz,
                                       cc_summary* summary, double huber_a, int32_t model, const cc_intr_start_options* start);

/* ---------------------------------------------------------------------------------------------
 * EXTENSION (nothing in the reference does it): a BATCH of independent single-camera problems solved together on one
 * device -- a rig's cameras before the rig solve (system_calibration.py runs optimize_intrinsics camera by camera,
 * cam_calibration.py:290-314), leave-one-view-out and bootstrap runs, subset fits. Problem p owns frames
 * [problem_offsets[p], problem_offsets[p+1]) of the concatenated frame list, frame f observations
 * [frame_offsets[f], frame_offsets[f+1]) of the concatenated uv / xyz. Per LM iteration the WHOLE batch costs two launches
 * (one sweep workgroup per frame of every problem, one step workgroup per problem); a problem that has finished is left
 * untouched while the others iterate, and a problem's result -- every bit of state, summary and log -- does not depend on
 * what else is in the batch or where it sits in it (it differs from cc_intrinsics_solve's in the order of a few sums:
 * rounding). One device, no exchange, no persistent form.
 * Bad arguments (n_problems <= 0, a problem without frames, offsets that do not start at 0 or decrease, NULL arrays) are
 * refused with CC_ERR_BAD_ARGUMENT before any device call.
 * ------------------------------------------------------------------------------------------- */
typedef struct cc_intrinsics_batch cc_intrinsics_batch;

int cc_intrinsics_batch_create(int32_t device, int64_t n_problems, const int64_t* problem_offsets /* [B+1] */,
                               const int64_t* frame_offsets /* [Ftot+1] */, const float* uv, const float* xyz,
                               cc_intrinsics_batch** out);
void cc_intrinsics_batch_destroy(cc_intrinsics_batch* h);
/* intr9 [B][9], const_mask [B] (NULL: nothing held), q_wxyz [Ftot][4], t_xyz [Ftot][3]: the current point of every problem. */
int cc_intrinsics_batch_set_state(cc_intrinsics_batch* h, const double* intr9, const uint32_t* const_mask,
                                  const double* q_wxyz, const double* t_xyz);
int cc_intrinsics_batch_get_state(cc_intrinsics_batch* h, double* intr9, double* q_wxyz, double* t_xyz);
/* Runs every problem's LM loop from its current point. ONE cc_options for the whole batch; summaries [B] (may be NULL), each
 * with its own caller-provided log; `seconds` is the wall time of the call in every one. Rounds are enqueued 1 + check_interval
 * (then check_interval) at a time with plain launches, the B control blocks are read in one transfer after each chunk, and the
 * call returns when every problem is done. use_graph is IGNORED (nothing is captured); profile_kernels is refused with
 * CC_ERR_BAD_ARGUMENT; max_iterations above 1023 is clamped to 1023. */
int cc_intrinsics_batch_solve(cc_intrinsics_batch* h, const cc_options* opt, cc_summary* summaries);
/* One-shot: create + set_state + solve + get_state + destroy. */
int cc_intrinsics_batch_optimize(const cc_options* opt, int32_t device, int64_t n_problems, const int64_t* problem_offsets,
                                 const int64_t* frame_offsets, const float* uv, const float* xyz, double* intr9,
                                 const uint32_t* const_mask, double* q_wxyz, double* t_xyz, cc_summary* summaries);
/* cc_intrinsics_estimate for every problem: Zhang's initialisation per problem on the same stream, then the batched solve.
 * distortion5 [B][5] (NULL: zeros) and const_mask [B] (NULL) are per problem; K_init9 [B][9] (may be NULL) receives Zhang's K.
 * Every problem needs >= 3 frames with >= 4 points each. */
int cc_intrinsics_batch_estimate(const cc_options* opt, int32_t device, int64_t n_problems, const int64_t* problem_offsets,
                                 const int64_t* frame_offsets, const float* uv, const float* xyz, const double* distortion5,
                                 const uint32_t* const_mask, float* K_init9, double* intr9, double* q_wxyz, double* t_xyz,
                                 cc_summary* summaries);
/* EXTENSION: the Huber loss of cc_intrinsics_set_huber per problem, a_pixels [B] (NULL: all off), for later solves. A problem
 * with a <= 0 keeps, bit for bit, what a batch without any loss returns for it; bad arguments (NULL handle, a NaN) are
 * refused before any device call. cc_intrinsics_batch_estimate_huber: cc_intrinsics_batch_estimate with huber_a [B] or NULL
 * (cc_intrinsics_batch_estimate IS it with NULL). */
int cc_intrinsics_batch_set_huber(cc_intrinsics_batch* h, const double* a_pixels);
int cc_intrinsics_batch_estimate_huber(const cc_options* opt, int32_t device, int64_t n_problems, const int64_t* problem_offsets,
                                       const int64_t* frame_offsets, const float* uv, const float* xyz, const double* distortion5,
                                       const uint32_t* const_mask, float* K_init9, double* intr9, double* q_wxyz, double* t_xyz,
                                       cc_summary* summaries, const double* huber_a);
/* EXTENSION: the camera model of the batch (CC_MODEL_RADTAN, the default, or CC_MODEL_FISHEYE). The model belongs to the
 * batch, not to a problem -- one handle, one model: a rig with both kinds of lens solves two batches. A fisheye handle
 * launches ONE sweep per round for every problem, with the Huber loss on or off per problem (cc_intrinsics_batch_set_huber; a
 * problem with the loss off, or with a threshold of +inf, keeps bit for bit what a batch without any loss returns for it);
 * a radial-tangential handle launches exactly what it launched before. On a fisheye handle cc_intrinsics_batch_set_state
 * takes the slots fx fy px py k1 k2 k3 k4 - per problem: bit 8 of every problem's constant mask is forced on, slot 8 is
 * stored as 0 and reads back as 0. A CHANGE of the model drops the state (the slots mean something else): call
 * cc_intrinsics_batch_set_state next, cc_intrinsics_batch_solve / _get_state return CC_ERR_STATE until then; setting the
 * model the handle has changes nothing; the Huber thresholds survive either way. An unknown model or a NULL handle:
 * CC_ERR_BAD_ARGUMENT, no device call. profile_kernels stays refused and use_graph ignored, as for every batch.
 * cc_intrinsics_batch_estimate_model: cc_intrinsics_batch_estimate_huber with a trailing model (that one IS this with
 * CC_MODEL_RADTAN). Fisheye: distortion5[p] holds k1..k4, its fifth entry is ignored; the start is Zhang's pinhole K and
 * poses with the given coefficients, as in cc_intrinsics_estimate_views_model. */
int cc_intrinsics_batch_set_model(cc_intrinsics_batch* h, int32_t model);
int cc_intrinsics_batch_get_model(const cc_intrinsics_batch* h, int32_t* model);
int cc_intrinsics_batch_estimate_model(const cc_options* opt, int32_t device, int64_t n_problems, const int64_t* problem_offsets,
                                       const int64_t* frame_offsets, const float* uv, const float* xyz, const double* distortion5,
                                       const uint32_t* const_mask, float* K_init9, double* intr9, double* q_wxyz, double* t_xyz,
                                       cc_summary* summaries, const double* huber_a, int32_t model);
/* EXTENSION: the fisheye focal-length start (cc_intrinsics_estimate_start_fisheye, above) for EVERY problem of a batch handle
 * whose model is CC_MODEL_FISHEYE (any other handle: CC_ERR_STATE), as one stream of seven launches whatever the number of
 * problems -- the boxes' zeroing, bounding boxes, r_max, centres and candidates, the search over (searched view of any
 * problem) x candidate, the pick, the pose pass over all views -- and one host wait. ONE cc_intr_start_options
 * for the whole batch (NULL: the defaults; out of range: CC_ERR_BAD_ARGUMENT before any device call); a finite `centre` applies
 * to every problem; search_views selects per problem: every view of a problem with no more views than that, else its views
 * floor(k F_p / S). Per problem the outputs are what the single call defines, and they do not depend on what else is in the
 * batch or where the problem sits in it: intr9 [B][9] = (f, f, c_x, c_y, 0, ...), q_wxyz [Ftot][4] / t_xyz [Ftot][3] with
 * q = (1, 0, 0, 0), t = 0 for a view that is invalid by its own data, counted in reports[p].views_invalid; reports [B]. Every
 * output may be NULL. The handle's state is not touched. A problem without a qualified candidate: CC_ERR_STATE, all B reports
 * are filled (best_candidate = -1 and views_invalid = 0 mark such a problem), the message names the first one, and nothing else
 * is written. */
int cc_intrinsics_batch_estimate_start_fisheye(cc_intrinsics_batch* h, const cc_intr_start_options* opt, double* intr9,
                                               double* q_wxyz, double* t_xyz, cc_intr_start_report* reports);
/* The last search of the handle: f, score (S_j), qualified, [B][C] each with C the candidates of that search (each may be
 * NULL). CC_ERR_STATE before any start. */
int cc_intrinsics_batch_start_scores(cc_intrinsics_batch* h, double* f, double* score, int32_t* qualified);
/* cc_intrinsics_batch_estimate_model with the start chosen. start NULL: that call, bit for bit (Zhang). Otherwise the model
 * must be CC_MODEL_FISHEYE (CC_ERR_BAD_ARGUMENT), the batched search replaces the per-problem Zhang launches, K_init9[p]
 * receives (f, 0, c_x; 0, f, c_y; 0, 0, 1) and the distortion starts from distortion5[p]'s four values (NULL: zeros). Every
 * problem needs >= 3 frames. A view without a pose at its problem's winner, or a problem without a winner:
 * CC_ERR_BAD_ARGUMENT, the message names the problem (and the view, by its index within the problem). The argument checks come
 * before the device is selected. */
int cc_intrinsics_batch_estimate_start(const cc_options* opt, int32_t device, int64_t n_problems, const int64_t* problem_offsets,
                                       const int64_t* frame_offsets, const float* uv, const float* xyz, const double* distortion5,
                                       const uint32_t* const_mask, float* K_init9, double* intr9, double* q_wxyz, double* t_xyz,
                                       cc_summary* summaries, const double* huber_a, int32_t model,
                                       const cc_intr_start_options* start);

/* Contiguous frame partition balanced by observation count (host logic, no GPU needed).
 * first_frame has nranks+1 entries; rank r owns frames [first_frame[r], first_frame[r+1]). */
int cc_partition_frames(int64_t n_frames, const int64_t* frame_offsets, int32_t nranks,
                        int64_t* first_frame);

/* ---------------------------------------------------------------------------------------------
 * Rig problem (ExtrinsicsCalibrator::Optimize, extrinsics_calibrator.cpp:86-257): one pose per
 * camera (camera_T_rig, shared) and one per observation frame (rig_T_world); world points are
 * constant; residuals in normalised image coordinates with ceres::HuberLoss(huber_a).
 * Observations are grouped by frame: frame f owns [obs_frame_offsets[f], obs_frame_offsets[f+1]).
 * obs_world indexes world_xyz (3 floats per point). cam_frozen[c] != 0 keeps camera c constant;
 * cameras / frames without observations are left untouched (they never enter the problem).
 * Any number of cameras: only cameras that are observed and not frozen own columns of the reduced system
 * (6 each, at most 255 in all, i.e. 42 optimised cameras; at most 64 observed cameras). Up to 127 coordinates the
 * tuned kernels run; beyond, plainer ones with a blocked factorisation of the reduced system (sixteen-column panels, trailing
 * updates on the matrix pipe); both take either exchange (since round 4 the large ones too: column sums posted / all-reduced,
 * one solving block).
 * ------------------------------------------------------------------------------------------- */
typedef struct cc_rig cc_rig;

int cc_rig_create(int32_t device, int64_t n_cams, int64_t n_frames, int64_t n_world,
                  const int64_t* obs_frame_offsets, const uint32_t* obs_cam,
                  const uint64_t* obs_world, const float* obs_uv, const float* world_xyz,
                  const uint8_t* cam_frozen, double huber_a, cc_rig** out);
void cc_rig_destroy(cc_rig* h);
int cc_rig_set_state(cc_rig* h, const double* cam_q, const double* cam_t, const double* frame_q,
                     const double* frame_t);
int cc_rig_reset(cc_rig* h);
int cc_rig_solve(cc_rig* h, const cc_options* opt, cc_summary* summary);
/* Which form cc_rig_solve runs (without profiling):
 *   2 -- the whole solve as ONE launch of the lean persistent kernel (+ its control workgroup's launch): poses only, at most 4
 *        observed cameras, 24 shared coordinates, ~1020 frames, the device to itself; the default where it fits. If its
 *        workgroups cannot all be resident the solve is run again in form 0 (same result, 1.3 s late, once per handle:
 *        the handle stays on form 0 -- cc_rig_solver_status says so and why);
 *   0 -- three kernels per LM iteration (sweep, decision + elimination, reduce + solve step + pose update): any size, any
 *        exchange; CC_RIG_PERSIST=0 forces it.
 * (Round 3's form 1, a glued persistent kernel behind CC_RIG_PERSIST=1, was slower than form 0 everywhere and is gone.) */
int cc_rig_solver_form(cc_rig* h);
/* The same, with the history of the handle: *reruns = lean persistent solves that gave up (not every workgroup resident)
 * and were run again in form 0; note (NUL-terminated, truncated to note_capacity) = the reason of the last one -- round
 * reached, workers started, whether and where the control workgroup ran. Any output may be NULL. */
int cc_rig_solver_status(cc_rig* h, int32_t* form, int32_t* reruns, char* note, int32_t note_capacity);
/* Ceres' inner iterations (Solver::Options::use_inner_iterations, CoordinateDescentMinimizer) for the poses-only rig
 * problem on one device; off by default. Semantics restated from Ceres 2.x, parity with Ceres unpinned:
 * after every candidate of a valid step with a finite cost, one inner pass visits the blocks group by group -- every camera's
 * t_cr, every camera's q_cr, every frame's t_rw, every frame's q_rw -- and minimises each with the others held (a trust-region
 * LM with Ceres' default Solver::Options, 50 iterations); the pass's cost reduction is added to the model cost change, the step
 * succeeds when the pass ends below the current cost or the relative decrease passes, and the passes stop for the rest of the
 * solve once one removes no more than `tolerance` (Ceres' inner_iteration_tolerance, 1e-3) of the candidate's cost.
 * cc_rig_set_inner_iterations applies to later cc_rig_solve calls; enabled, the handle solves in form 0 (three kernels per
 * iteration; cc_rig_solver_form reports 0). CC_ERR_STATE for a cc_rigk_* handle and for a handle with an exchange or an
 * all-reduce attached: those are out of scope (cc_rig_comm_init / cc_rig_exchange_attach refuse a handle with them on).
 * cc_rig_inner_pass: one pass from the current state, which it updates (a test and measurement aid); costs before and after;
 * mini_iterations[g] = the most iterations any block of group g (0 t_cr, 1 q_cr, 2 t_rw, 3 q_rw) ran. Outputs may be NULL.
 * cc_rig_inner_status: the last solve's passes, passes that ended below the current cost, whether the passes were still enabled
 * at its end, and the cost the passes removed in all. Any output may be NULL. */
int cc_rig_set_inner_iterations(cc_rig* h, int32_t enable, double tolerance);
int cc_rig_inner_pass(cc_rig* h, double* cost_before, double* cost_after, int32_t mini_iterations[4]);
int cc_rig_inner_status(cc_rig* h, int32_t* passes, int32_t* useful_passes, int32_t* enabled_at_end, double* cost_removed);
/* Any output may be NULL. obs_cost[k] = 1/2 rho(|r_k|^2) at the current point, in the caller's
 * observation order (extrinsics_calibrator.cpp:219-225). */
int cc_rig_get_state(cc_rig* h, double* cam_q, double* cam_t, double* frame_q, double* frame_t,
                     double* obs_cost);
/* Total robustified cost at the current point (one sweep; this rank's observations only). */
int cc_rig_eval(cc_rig* h, double* cost);
/* EXTENSION: start poses from the handle's own observations, on the device (the reference takes its start from OpenCV solvePnP
 * in a helper package; cc_rig_set_state needs poses). A VIEW is one camera's observations in one frame.
 *   V  every view in closed form: planar views (>= 4 points, the board anywhere in the world) by a homography in the board's
 *      own basis, general views (>= 6 points) by a 3 x 4 DLT, both on centred and scaled points; collinear or coincident
 *      points, too few points or a non-finite coordinate make the view INVALID: it is skipped and counted
 *   R  at most refine_iterations Levenberg-Marquardt steps on the view's six pose coordinates (residual x/z - u, y/z - v, no
 *      loss function); 0: the closed form as it is
 *   T  a spanning tree over the cameras by co-visible valid views, rooted at the observed frozen camera with the most valid
 *      views (none frozen: the observed camera with the most valid views, placed at the identity); frozen cameras keep the
 *      caller's pose; ties go to the lowest index
 *   C  camera_T_rig along the tree: per (child, parent) edge the mean relative pose over the co-visible frames, weighted by
 *      1 / (rms^2 of the child's view + rms^2 of the parent's)
 *   F  rig_T_world of every frame: mean over its valid views of placed cameras, weighted by 1 / rms^2
 * cam_q / cam_t / frame_q / frame_t are the caller's poses (NULL: the identity): used for frozen cameras, for cameras without a
 * path to the root and for frames without a valid view of a placed camera. The result becomes the handle's state as
 * cc_rig_set_state would have set it (cc_rig_reset returns to it); read it with cc_rig_get_state. opt and report may be NULL;
 * report->parent (may be NULL) receives n_cams entries: the parent of every estimated camera, -1 for the root, frozen and
 * unplaced cameras.
 * cc_rig_start_views reads back stages V and R of the last call, one entry per view in (frame, camera) order: n_views first
 * (the other outputs may be NULL; they hold n_views entries, q 4 and t 3 doubles each), kind 0 invalid / 1 planar / 2 general,
 * rms2 = mean squared residual per observation coordinate.
 * CC_ERR_STATE, the handle unchanged: a cc_rigk_* handle (pixel observations need the lens model first: cc_rigk_estimate_start
 * below), a handle with an
 * exchange or a communicator, a handle none of whose cameras is observed. */
typedef struct cc_rig_start_options {
  int32_t refine_iterations;   /* default 10 */
} cc_rig_start_options;
void cc_rig_start_options_init(cc_rig_start_options* o);
typedef struct cc_rig_start_report {
  int64_t views_valid, views_planar, views_general, views_invalid;
  int64_t frames_placed, frames_unplaced;
  int32_t cameras_placed, cameras_unplaced;
  int32_t root_camera;         /* -1: no camera has a valid view */
  int32_t root_at_identity;    /* the root is not frozen: it defines the rig frame */
  int32_t* parent;             /* caller array of n_cams entries, or NULL */
} cc_rig_start_report;
int cc_rig_estimate_start(cc_rig* h, const cc_rig_start_options* opt, const double* cam_q, const double* cam_t,
                          const double* frame_q, const double* frame_t, cc_rig_start_report* report);
int cc_rig_start_views(cc_rig* h, int64_t* n_views, int32_t* view_cam, int64_t* view_frame, int32_t* kind, double* q, double* t,
                       double* rms2);
/* Multi-GPU: each rank creates its handle with a contiguous shard of frames (cc_partition_frames on
 * obs_frame_offsets) and ALL cameras / world points; then attaches as for the intrinsics problem.
 * Per LM iteration: one all-reduce of the reduced (6C)x(6C) system (PC + 32 doubles) and one of
 * 4 + 6C statistics. */
int cc_rig_comm_init(cc_rig* h, const uint8_t id[128], int32_t rank, int32_t nranks);
/* Mailbox exchange for the rig path (same protocol as cc_intrinsics_exchange_*; <= 8 ranks of one node).
 * _attach is collective: every rank must call it (the per-rank "camera seen" flags are summed through
 * the mailboxes, like cc_rig_comm_init does with an all-reduce). */
int cc_rig_exchange_export(cc_rig* h, uint8_t handle[64]);
int cc_rig_exchange_attach(cc_rig* h, int32_t rank, int32_t nranks, const uint8_t* handles);

/* EXTENSION (BASELINE.json configs[3]-[4] name it, nothing in the reference does it):
 * the rig problem with 9 intrinsics (fx fy px py k1 k2 p1 p2 k3, calibrator.cpp:168-179) shared by all
 * cameras and co-optimised with the poses. Observations are PIXELS: the residual is the composition of
 * ReprojectionErrorExtrinsics (extrinsics_calibrator.cpp:51-84) and DistortNormalized/DistortPixels
 * (calibrator.cpp:70-95). huber_a is in pixels, <= 0 switches the loss off. 6 columns per optimised camera + 9
 * must stay <= 255. Multi-GPU through cc_rig_exchange_* / cc_rig_comm_init like the plain rig problem (intrinsics
 * replicated), at every supported size.
 * The handle is a cc_rig: set_state / reset / solve / get_state / eval / destroy are the cc_rig_* calls;
 * cc_rigk_set_intrinsics must be called once before the first solve (const_mask bit i freezes intrinsic i). */
int cc_rigk_create(int32_t device, int64_t n_cams, int64_t n_frames, int64_t n_world,
                   const int64_t* obs_frame_offsets, const uint32_t* obs_cam, const uint64_t* obs_world,
                   const float* obs_uv_pixels, const float* world_xyz, const uint8_t* cam_frozen,
                   double huber_a, cc_rig** out);
int cc_rigk_set_intrinsics(cc_rig* h, const double* intr9, uint32_t const_mask);
int cc_rigk_get_intrinsics(cc_rig* h, double* intr9);
/* Same extension with one set of 9 intrinsics PER CAMERA (BASELINE.json configs[4]: "full intrinsics+extrinsics
 * co-optimisation"): shared block = 6 per optimised camera + 9 per observed camera (<= 255: seventeen cameras; <= 127,
 * eight cameras, for the tuned kernels and for several GPUs).
 * cc_rigk_set_intrinsics sets every camera's set at once, cc_rigk_set_camera_intrinsics one camera's (with its own
 * constant mask, cf. Calibrator::ForceDistortionToConstant); cc_rigk_get_camera_intrinsics reads one set. */
int cc_rigk_create_per_camera(int32_t device, int64_t n_cams, int64_t n_frames, int64_t n_world,
                              const int64_t* obs_frame_offsets, const uint32_t* obs_cam, const uint64_t* obs_world,
                              const float* obs_uv_pixels, const float* world_xyz, const uint8_t* cam_frozen,
                              double huber_a, cc_rig** out);
int cc_rigk_set_camera_intrinsics(cc_rig* h, int64_t camera, const double* intr9, uint32_t const_mask);
int cc_rigk_get_camera_intrinsics(cc_rig* h, int64_t camera, double* intr9);
/* EXTENSION: the pixel model of a cc_rigk_* handle (CC_MODEL_RADTAN, the default, or CC_MODEL_FISHEYE, above). The model
 * belongs to the handle, for all of its cameras -- one shared set or one per camera; a rig that mixes both gives each camera
 * its own (cc_rigk_set_camera_model below).
 * Fisheye: the slots are fx fy px py k1 k2 k3 k4 -; cc_rigk_set_intrinsics / _set_camera_intrinsics force bit 8 of the
 * constant mask and store 0 in slot 8. A CHANGE of the model drops the captured graphs and the intrinsics (the next solve
 * needs cc_rigk_set_intrinsics again) and puts the handle on the tile form of the sweep (k_rig_sweep_lens: there is
 * no compact-record form, whatever the group size and CC_RIG_K_COMPACT). Setting the model the handle has is a no-op; a
 * handle that never leaves CC_MODEL_RADTAN launches the kernels it always did. Large rigs (<= 255 shared coordinates),
 * cc_rig_eval / _reset / _solver_status and profiled rounds work as on any cc_rigk_* handle.
 * CC_ERR_STATE: a poses-only handle (cc_rig_create); CC_MODEL_FISHEYE on a handle with an exchange or a communicator
 * (and cc_rig_comm_init / cc_rig_exchange_export / _attach on a fisheye handle: one device only).
 * CC_ERR_BAD_ARGUMENT: an unknown model. */
int cc_rigk_set_model(cc_rig* h, int32_t model);
int cc_rigk_get_model(cc_rig* h, int32_t* model);
/* EXTENSION: a pixel model PER CAMERA, for a handle with a set of intrinsics per camera (cc_rigk_create_per_camera): a fisheye
 * lens next to radial-tangential ones, refined jointly over the frame poses they share. cc_rigk_get_model reports
 * CC_MODEL_MIXED when the cameras differ, otherwise their common model; CC_MODEL_MIXED is never accepted as an argument.
 * Setting the model a camera has is a no-op. A CHANGE drops the captured graphs and THAT camera's intrinsics only -- the other
 * sets and all poses stay; a solve, eval or start before that camera's next cc_rigk_set_camera_intrinsics (or
 * cc_rigk_set_intrinsics) fails with CC_ERR_STATE. A fisheye camera's set has the slots fx fy px py k1 k2 k3 k4 -:
 * cc_rigk_set_camera_intrinsics forces bit 8 of THAT set's constant mask and stores 0 in its slot 8, a radial-tangential
 * camera's set is taken as given; cc_rigk_set_intrinsics applies the rule set by set. cc_rigk_set_model keeps its meaning on
 * such a handle: every camera gets the model (a no-op when every camera has it, otherwise all intrinsics are dropped).
 * A handle all of whose cameras have one model IS the homogeneous handle of that model, however it got there: it launches the
 * kernels such a handle launches and returns the same bits. A handle whose cameras differ sweeps into tiles (no compact-record
 * form, whatever the group size and CC_RIG_K_COMPACT) with ONE LAUNCH PER MODEL that has an observed camera
 * (k_rig_sweep_lens): under profile_kernels a sweep then counts two launches of CC_K_SWEEP in kernel_launches while
 * `sweeps` stays one per round. Large rigs, cc_rig_eval / _reset / _solver_status / _get_state, profiled rounds and
 * cc_rigk_estimate_start (every pixel through the inverse of ITS camera's model) work. A camera without observations keeps
 * its recorded model.
 * CC_ERR_STATE, the handle unchanged: a poses-only handle (cc_rig_create); a handle with one shared set (cc_rigk_create: one
 * set of nine numbers cannot follow two models, use cc_rigk_set_model); CC_MODEL_FISHEYE on a handle with an exchange or a
 * communicator (and cc_rig_comm_init / cc_rig_exchange_export / _attach on a handle ANY camera of which is fisheye).
 * CC_ERR_BAD_ARGUMENT, the handle unchanged: a camera out of range, an unknown model, CC_MODEL_MIXED, a NULL output. */
enum { CC_MODEL_MIXED = 2 };   /* reported only, never accepted as an argument */
int cc_rigk_set_camera_model(cc_rig* h, int64_t camera, int32_t model);
int cc_rigk_get_camera_model(cc_rig* h, int64_t camera, int32_t* model);
/* EXTENSION: cc_rig_estimate_start for a cc_rigk_* handle, whose observations are pixels. Every pixel first goes through the
 * inverse of the handle's pixel model at the handle's START intrinsics -- what cc_rigk_set_intrinsics / _set_camera_intrinsics
 * last wrote, not what a solve has made of them -- on the device, in double precision, into a float normalised image point;
 * stages V, R, T, C and F above then run on those points unchanged. Arguments, options, report and the meaning of the caller's
 * poses are those of cc_rig_estimate_start; the result becomes the handle's state (cc_rig_reset returns to it), the intrinsics,
 * their masks and the model are not written, and cc_rig_start_views reads the views back as after cc_rig_estimate_start.
 *   radial-tangential: the root of the distortion map by damped Newton steps from the distorted point (the method of
 *     cc_undistort, at most 100 steps); a search that does not end on a root of the map gives no point
 *   fisheye: theta in [0, pi/2) with theta_d(theta) = |distorted point| by the rule of cc_undistort_fisheye, the point scaled
 *     by tan(theta) / theta_d; a polynomial that turns back before it reaches the pixel gives no point; the axis maps to itself
 * A pixel without a point (no root, a non-finite pixel, a zero or non-finite fx / fy) becomes NaN, NaN and makes its view
 * INVALID, as a non-finite coordinate does in cc_rig_estimate_start: single observations are not dropped. Intrinsics under which
 * no view is valid are not an error: CC_OK, every pose keeps the caller's value, the report counts the views as invalid.
 * The pinhole form x / z of the normalised point limits THIS start to points well inside 90 degrees off the axis; wider rigs
 * start from cc_rigk_estimate_start_bearing below.
 * cc_rigk_start_points: the normalised points of the last cc_rigk_estimate_start in the CALLER's observation order (2 floats
 * per observation) and how many of them are NaN; either output may be NULL.
 * CC_ERR_STATE, the handle unchanged: a poses-only handle (cc_rig_create: use cc_rig_estimate_start), no intrinsics set (never,
 * or not since cc_rigk_set_model changed the model), a handle with an exchange or a communicator, a handle none of whose
 * cameras is observed; cc_rigk_start_points before a start has run. cc_rig_estimate_start keeps refusing cc_rigk_* handles. */
int cc_rigk_estimate_start(cc_rig* h, const cc_rig_start_options* opt, const double* cam_q, const double* cam_t,
                           const double* frame_q, const double* frame_t, cc_rig_start_report* report);
int cc_rigk_start_points(cc_rig* h, float* uv_normalised, int64_t* n_without_root);
/* EXTENSION: cc_rigk_estimate_start on UNIT BEARINGS instead of x / z, for rigs whose points reach or pass 90 degrees off the
 * optical axis (surround-view fisheye lenses of 185 - 200 degrees), where a normalised image point does not exist. Arguments,
 * options, report, the meaning of the caller's poses and the CC_ERR_STATE cases are those of cc_rigk_estimate_start; the handle
 * may have one shared set, a set per camera or a model per camera. The result becomes the handle's state (cc_rig_reset returns
 * to it), intrinsics, masks and models are not written, cc_rig_start_views reads the views back. cc_rigk_estimate_start keeps
 * its arithmetic and its bits; this is a second entry point, not its replacement.
 *   bearing of a pixel (device, double precision on the float pixel, rounded to three floats):
 *     radial-tangential: the root (x, y) exactly as in cc_rigk_estimate_start, b = (x, y, 1) / |(x, y, 1)|
 *     fisheye: theta in [0, pi) -- not [0, pi/2) -- with theta_d(theta) = |distorted point| by the same rule (Newton steps that
 *       fall back to bisection inside the bracket 0 .. the double below pi; plain Newton up the first rising branch when the far
 *       end does not bracket), b = (sin theta (xd, yd) / theta_d, cos theta); the axis gives exactly (0, 0, 1)
 *     no root, a non-finite pixel, a zero or non-finite fx / fy: NaN x 3, the view INVALID (single observations are not dropped)
 *   stage V: the same classification, centring, scaling and board basis; P (3 x 3 on a board's coordinates, 3 x 4 otherwise) is
 *     the null vector of the Gram sum_i (I - b_i b_i^T) (x) y~_i y~_i^T, which is b x (P y~) = 0. General views keep
 *     P / cbrt(det P_3x3); planar views scale by 1 / |first column| and take the sign with sum_i b_i . (P y~_i) > 0, the points
 *     along their bearings (t_z > 0 would be wrong for a board that the camera's plane cuts)
 *   stage R: Levenberg-Marquardt on the chord r = p / |p| - b, p = R X + t, the same updates and damping, a step accepted when
 *     the cost drops and is finite (no depth test: nothing is singular short of p = 0); rms^2 = cost / (2 n), a squared angle
 *     for small errors -- the unit of the x / z form near the axis, so the weights of stages C and F keep their meaning
 * (a bearing is normalised again in double precision where it is used: the rounding to float leaves its length 6e-8 off 1).
 * cc_rigk_start_bearings: the bearings of the last cc_rigk_estimate_start_bearing in the CALLER's observation order (3 floats per
 * observation) and how many are NaN; either output may be NULL. CC_ERR_STATE before a bearing start has run and after a
 * cc_rigk_estimate_start since; cc_rigk_start_points likewise returns CC_ERR_STATE after a bearing start: each reads its own
 * start's buffer only. */
int cc_rigk_estimate_start_bearing(cc_rig* h, const cc_rig_start_options* opt, const double* cam_q, const double* cam_t,
                                   const double* frame_q, const double* frame_t, cc_rig_start_report* report);
int cc_rigk_start_bearings(cc_rig* h, float* bearing_xyz, int64_t* n_without_root);

/* One-shot: the call ExtrinsicsCalibrator::Optimize makes in place of
 * extrinsics_calibrator.cpp:92-225. opt == NULL -> cc_options_init with max_iterations = 1000. */
int cc_rig_optimize(const cc_options* opt, int32_t device, int64_t n_cams, int64_t n_frames,
                    int64_t n_world, const int64_t* obs_frame_offsets, const uint32_t* obs_cam,
                    const uint64_t* obs_world, const float* obs_uv, const float* world_xyz,
                    double* cam_q, double* cam_t, const uint8_t* cam_frozen, double* frame_q,
                    double* frame_t, double huber_a, double* obs_cost, cc_summary* summary);
/* EXTENSION: start, then solve, behind one upload -- cc_rig_create, cc_rig_estimate_start (default options) with the poses
 * passed in as the caller's, cc_rig_solve, cc_rig_get_state. Same argument list as cc_rig_optimize. */
int cc_rig_estimate(const cc_options* opt, int32_t device, int64_t n_cams, int64_t n_frames,
                    int64_t n_world, const int64_t* obs_frame_offsets, const uint32_t* obs_cam,
                    const uint64_t* obs_world, const float* obs_uv, const float* world_xyz,
                    double* cam_q, double* cam_t, const uint8_t* cam_frozen, double* frame_q,
                    double* frame_t, double huber_a, double* obs_cost, cc_summary* summary);

/* The same for observations the caller keeps FRAME BY FRAME as arrays of records (ExtrinsicsCalibrator's per-frame lists of
 * sightings -- camera id, point id, normalised image point, cost -- extrinsics_calibrator.cpp:33-49 fills them): frame f has
 * counts[f] records starting at frame_records[f], `stride` bytes apart; in a record the camera id and the global world point
 * id are 64-bit unsigned integers at camera_offset / world_offset, the normalised image point two floats at uv_offset, and
 * the robustified cost 0.5 rho(||r||^2) is WRITTEN as a double at cost_offset (negative: not written). The library reads the
 * records in place (no flat copies on the caller's side) and writes the costs back into them. */
typedef struct cc_obs_layout {
  int64_t stride, camera_offset, world_offset, uv_offset, cost_offset;
} cc_obs_layout;
int cc_rig_optimize_frames(const cc_options* opt, int32_t device, int64_t n_cams, int64_t n_frames, int64_t n_world,
                           void* const* frame_records, const int64_t* counts, const cc_obs_layout* layout,
                           const float* world_xyz, double* cam_q, double* cam_t, const uint8_t* cam_frozen,
                           double* frame_q, double* frame_t, double huber_a, cc_summary* summary);

/* The same for observations kept frame by frame as COLUMNS (round 5: what ExtrinsicsCalibrator holds now -- per frame one
 * array of camera ids, one of global world point ids, one of normalised image points, one of costs): column[f] is the first
 * entry of frame f, entries `*_stride` bytes apart (arrays: the stride is the entry's size; records: the stride of the record
 * and column pointers into it -- cc_rig_optimize_frames is exactly that). Ids are unsigned, 4 or 8 bytes wide (`*_width`);
 * the image point two floats; the cost a double, WRITTEN (cost == NULL: not written). A frame without observations may have
 * NULL entries. Why columns: at 8 M observations the solve streams 20 bytes per observation instead of a 40-byte record and
 * the costs come back as sequential stores instead of one partial store per record. */
typedef struct cc_obs_columns {
  const void* const* camera; int64_t camera_stride; int32_t camera_width;
  const void* const* world;  int64_t world_stride;  int32_t world_width;
  const void* const* uv;     int64_t uv_stride;
  void* const* cost;         int64_t cost_stride;
} cc_obs_columns;
int cc_rig_optimize_columns(const cc_options* opt, int32_t device, int64_t n_cams, int64_t n_frames, int64_t n_world,
                            const cc_obs_columns* columns, const int64_t* counts,
                            const float* world_xyz, double* cam_q, double* cam_t, const uint8_t* cam_frozen,
                            double* frame_q, double* frame_t, double huber_a, cc_summary* summary);

/* The same over several devices from one host thread (cf. cc_intrinsics_optimize_multi): frames sharded, cameras and
 * world points replicated; ExtrinsicsCalibrator::SetDevices selects it behind the class surface. */
int cc_rig_optimize_multi(const cc_options* opt, int32_t n_devices, const int32_t* devices, int64_t n_cams,
                          int64_t n_frames, int64_t n_world, const int64_t* obs_frame_offsets,
                          const uint32_t* obs_cam, const uint64_t* obs_world, const float* obs_uv,
                          const float* world_xyz, double* cam_q, double* cam_t, const uint8_t* cam_frozen,
                          double* frame_q, double* frame_t, double huber_a, double* obs_cost,
                          cc_summary* summary);

/* ---------------------------------------------------------------------------------------------
 * Zhang's closed-form initialisation on the device: what Calibrator::Estimate does before calling
 * Optimize (calibrator.cpp:47-66): per-frame DLT homography from (world x,y) -> image
 * (geometry.cpp:70-105), K from the homographies (geometry.cpp:123-177), per-frame pose
 * (geometry.cpp:179-203) as a float quaternion w x y z and translation. Needs >= 3 frames with
 * >= 4 points each. Outputs K9 (row-major 3x3); q_wxyz [4F], t_xyz [3F], homographies [9F] may be
 * NULL. The DLT null vector's sign is fixed so that the board lies in front of the camera.
 * ------------------------------------------------------------------------------------------- */
int cc_zhang_init(int32_t device, int64_t n_frames, const int64_t* frame_offsets, const float* uv,
                  const float* xyz, float* K9, float* q_wxyz, float* t_xyz, float* homographies);

/* ---------------------------------------------------------------------------------------------
 * Point kernels of the Calibrator surface.
 * ------------------------------------------------------------------------------------------- */
/* Calibrator::Distort (calibrator.cpp:157-166): normalised -> pixel coordinates, float arithmetic
 * with the reference's promotions. K: row-major 3x3, dist: k1 k2 p1 p2 k3. */
int cc_distort(int32_t device, const float* K9, const float* dist5, int64_t n,
               const float* xy_normalized, float* uv_out);
/* Calibrator::Undistort (calibrator.cpp:118-155): pixel -> undistorted normalised coordinates. */
int cc_undistort(int32_t device, const float* K9, const float* dist5, int64_t n, const float* uv,
                 float* xy_out);
/* EXTENSION: the same pair for the fisheye model (CC_MODEL_FISHEYE above), dist4: k1 k2 k3 k4; float in and out, double
 * arithmetic; K's fx fy px py are used. Distort: with r = |xy| and theta = atan(r), uv = K (theta_d / r) xy (the limit value at
 * r = 0). Undistort: (x', y') = K^-1 uv, theta_d = |(x', y')|, the root theta in [0, pi/2) of theta_d(theta) by a bracketed
 * Newton iteration, xy = tan(theta) / theta_d (x', y'). A pixel without a root in that interval (theta_d beyond the polynomial's
 * range there, a non-monotone polynomial that never reaches it) gives NaN in both coordinates. */
int cc_distort_fisheye(int32_t device, const float* K9, const float* dist4, int64_t n,
                       const float* xy_normalized, float* uv_out);
int cc_undistort_fisheye(int32_t device, const float* K9, const float* dist4, int64_t n, const float* uv,
                         float* xy_out);

#ifdef __cplusplus
}
#endif
#endif
