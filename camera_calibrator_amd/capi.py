"""ctypes binding of the C ABI declared in include/cc_solver.h (libcc_hip.so).

This is the boundary the parity tests and bench.py call through. There is no CPU fallback: if the
shared library is missing, or no gfx950 device is usable, the calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CC_LIB_PATH", os.path.join(_HERE, "libcc_hip.so"))

K_NAMES = ["sweep", "decide", "elim", "solve", "allreduce", "update", "reduce"]
TERMINATION = {0: "NO_CONVERGENCE", 1: "GRADIENT", 2: "PARAMETER", 3: "FUNCTION",
               4: "FAILURE_INVALID_STEPS", 5: "MIN_RADIUS", 6: "FAILURE_EXCHANGE"}


class CcError(RuntimeError):
    pass


class Options(C.Structure):
    _fields_ = [
        ("max_iterations", C.c_int32),
        ("use_nonmonotonic_steps", C.c_int32),
        ("max_consecutive_nonmonotonic_steps", C.c_int32),
        ("jacobi_scaling", C.c_int32),
        ("max_consecutive_invalid_steps", C.c_int32),
        ("check_interval", C.c_int32),
        ("function_tolerance", C.c_double),
        ("gradient_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double),
        ("initial_radius", C.c_double),
        ("max_radius", C.c_double),
        ("min_radius", C.c_double),
        ("min_relative_decrease", C.c_double),
        ("min_lm_diagonal", C.c_double),
        ("max_lm_diagonal", C.c_double),
        ("use_graph", C.c_int32),
        ("profile_kernels", C.c_int32),
    ]


class Iteration(C.Structure):
    _fields_ = [
        ("cost", C.c_double),
        ("cost_change", C.c_double),
        ("model_cost_change", C.c_double),
        ("relative_decrease", C.c_double),
        ("gradient_max_norm", C.c_double),
        ("step_norm", C.c_double),
        ("radius", C.c_double),
        ("accepted", C.c_int32),
        ("valid", C.c_int32),
    ]


class IntrStartOptions(C.Structure):
    """cc_intr_start_options: the fisheye focal-length start (cc_intrinsics_estimate_start_fisheye)."""
    _fields_ = [
        ("centre", C.c_double * 2),
        ("theta_lo", C.c_double),
        ("theta_hi", C.c_double),
        ("candidates", C.c_int32),
        ("search_views", C.c_int32),
        ("refine_iterations", C.c_int32),
    ]


class IntrStartReport(C.Structure):
    _fields_ = [
        ("centre", C.c_double * 2),
        ("r_max", C.c_double),
        ("focal", C.c_double),
        ("best_candidate", C.c_int32),
        ("candidates_qualified", C.c_int32),
        ("views", C.c_int64),
        ("views_searched", C.c_int64),
        ("views_invalid", C.c_int64),
    ]


class Summary(C.Structure):
    _fields_ = [
        ("iterations", C.c_int32),
        ("successful_steps", C.c_int32),
        ("termination", C.c_int32),
        ("log_len", C.c_int32),
        ("initial_cost", C.c_double),
        ("final_cost", C.c_double),
        ("seconds", C.c_double),
        ("log", C.POINTER(Iteration)),
        ("log_capacity", C.c_int32),
        ("sweeps", C.c_int32),
        ("kernel_ms", C.c_double * 8),
        ("kernel_launches", C.c_int32 * 8),
        ("kernel_idle_ms", C.c_double * 8),
        ("kernel_idle_launches", C.c_int32 * 8),
    ]


# every symbol include/cc_solver.h declares
EXPORTED_SYMBOLS = [
    "cc_options_init", "cc_last_error", "cc_version", "cc_device_count", "cc_release_caches", "cc_parallel_for", "cc_parallel_parts", "cc_host_pool_threads", "cc_last_call_solver_status",
    "cc_intrinsics_create", "cc_intrinsics_destroy", "cc_intrinsics_set_state",
    "cc_intrinsics_reset", "cc_intrinsics_get_state", "cc_intrinsics_eval",
    "cc_intrinsics_solve", "cc_intrinsics_solver_form", "cc_intrinsics_solver_status", "cc_intrinsics_profile_sweep", "cc_intrinsics_profile_solve", "cc_intrinsics_optimize", "cc_intrinsics_estimate", "cc_intrinsics_estimate_views", "cc_intrinsics_optimize_views", "cc_host_staging_acquire", "cc_host_staging_release", "cc_last_call_timing", "cc_comm_get_unique_id",
    "cc_intrinsics_comm_init", "cc_intrinsics_exchange_export", "cc_intrinsics_exchange_attach", "cc_partition_frames", "cc_distort", "cc_undistort",
    "cc_rig_create", "cc_rig_destroy", "cc_rig_set_state", "cc_rig_reset", "cc_rig_solve",
    "cc_rig_get_state", "cc_rig_solver_form", "cc_rig_solver_status", "cc_rig_eval", "cc_rig_optimize", "cc_rig_comm_init", "cc_rig_exchange_export", "cc_rig_exchange_attach", "cc_rigk_create",
    "cc_rigk_set_intrinsics", "cc_rigk_get_intrinsics", "cc_rigk_create_per_camera", "cc_rigk_set_camera_intrinsics",
    "cc_rigk_get_camera_intrinsics", "cc_rigk_set_model", "cc_rigk_get_model", "cc_rigk_set_camera_model", "cc_rigk_get_camera_model", "cc_rigk_estimate_start", "cc_rigk_start_points", "cc_rigk_estimate_start_bearing", "cc_rigk_start_bearings", "cc_zhang_init", "cc_intrinsics_optimize_multi", "cc_rig_optimize_multi", "cc_rig_optimize_frames", "cc_rig_optimize_columns",
    "cc_rig_set_inner_iterations", "cc_rig_inner_pass", "cc_rig_inner_status",
    "cc_rig_start_options_init", "cc_rig_estimate_start", "cc_rig_start_views", "cc_rig_estimate",
    "cc_intrinsics_batch_create", "cc_intrinsics_batch_destroy", "cc_intrinsics_batch_set_state", "cc_intrinsics_batch_get_state",
    "cc_intrinsics_batch_solve", "cc_intrinsics_batch_optimize", "cc_intrinsics_batch_estimate",
    "cc_intrinsics_set_huber", "cc_intrinsics_obs_cost", "cc_intrinsics_optimize_views_huber", "cc_intrinsics_estimate_views_huber",
    "cc_intrinsics_batch_set_huber", "cc_intrinsics_batch_estimate_huber",
    "cc_intrinsics_set_final_sweep", "cc_intrinsics_final_sweep_counts",
    "cc_intrinsics_set_model", "cc_intrinsics_get_model", "cc_intrinsics_optimize_views_model", "cc_intrinsics_estimate_views_model",
    "cc_distort_fisheye", "cc_undistort_fisheye",
    "cc_intrinsics_batch_set_model", "cc_intrinsics_batch_get_model", "cc_intrinsics_batch_estimate_model",
    "cc_intr_start_options_init", "cc_intrinsics_estimate_start_fisheye", "cc_intrinsics_start_scores", "cc_intrinsics_estimate_views_start",
    "cc_intrinsics_batch_estimate_start_fisheye", "cc_intrinsics_batch_start_scores", "cc_intrinsics_batch_estimate_start",
]
# EXTENSION: camera models of the single-camera solve (cc_solver.h)
MODEL_RADTAN, MODEL_FISHEYE = 0, 1
MODEL_MIXED = 2   # what RigProblem.get_model reports when the cameras differ (set_camera_model); never an argument
# every symbol include/cc_harness.h declares (synthetic-input harness, host code)
HARNESS_SYMBOLS = [
    "cc_generator_create", "cc_generator_destroy", "cc_generator_set_k", "cc_generator_set_distortion",
    "cc_generator_set_noise", "cc_generator_planar", "cc_generator_points", "cc_rig_scenario", "cc_affine_to_qt",
]

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CcError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        _lib = C.CDLL(LIB_PATH)
        _lib.cc_last_error.restype = C.c_char_p
        _lib.cc_version.restype = C.c_char_p
        _lib.cc_generator_create.restype = C.c_void_p
        _lib.cc_generator_planar.restype = C.c_int64
        _lib.cc_generator_points.restype = C.c_int64
    return _lib


def _check(rc):
    if rc != 0:
        raise CcError(f"cc error {rc}: {lib().cc_last_error().decode()}")


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def default_options(**kw):
    o = Options()
    lib().cc_options_init(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def intr_start_options(**kw):
    """cc_intr_start_options with the library's defaults (centre NaN NaN: the pixels' bounding box, theta_lo 0.3, theta_hi 3.0,
    candidates 24, search_views 32, refine_iterations 3) and the given fields; centre takes a pair."""
    o = IntrStartOptions()
    lib().cc_intr_start_options_init(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        if k == "centre":
            o.centre[0], o.centre[1] = float(v[0]), float(v[1])
        else:
            setattr(o, k, v)
    return o


def device_count():
    return int(lib().cc_device_count())


def partition_frames(frame_offsets, nranks):
    off = np.ascontiguousarray(frame_offsets, dtype=np.int64)
    first = np.zeros(nranks + 1, dtype=np.int64)
    _check(lib().cc_partition_frames(C.c_int64(len(off) - 1), _p(off, C.c_int64), C.c_int32(nranks),
                                     _p(first, C.c_int64)))
    return first


def _start_report_dict(r):
    """cc_intr_start_report as a dict (centre: a pair)."""
    report = {k: getattr(r, k) for k, _ in IntrStartReport._fields_ if k != "centre"}
    report["centre"] = (r.centre[0], r.centre[1])
    return report


def _summary(log_capacity):
    """(Summary with a log of log_capacity rows, the log): what a solve call fills and _summary_dict reads."""
    log = (Iteration * max(1, log_capacity))()
    s = Summary()
    s.log, s.log_capacity = C.cast(log, C.POINTER(Iteration)), log_capacity
    return s, log


def _summary_dict(s, log):
    names = [f[0] for f in Iteration._fields_]
    return {
        "iterations": s.iterations, "successful_steps": s.successful_steps,
        "termination": TERMINATION.get(s.termination, str(s.termination)),
        "initial_cost": s.initial_cost, "final_cost": s.final_cost, "seconds": s.seconds,
        "sweeps": s.sweeps,
        "kernel_ms": {K_NAMES[i]: s.kernel_ms[i] for i in range(len(K_NAMES))},
        "kernel_launches": {K_NAMES[i]: s.kernel_launches[i] for i in range(len(K_NAMES))},
        "kernel_idle_ms": {K_NAMES[i]: s.kernel_idle_ms[i] for i in range(len(K_NAMES))},
        "kernel_idle_launches": {K_NAMES[i]: s.kernel_idle_launches[i] for i in range(len(K_NAMES))},
        "log": [{k: getattr(log[i], k) for k in names} for i in range(s.log_len)],
    }


class IntrinsicsProblem:
    """Handle on a single-camera intrinsics problem resident in HBM (cc_intrinsics_*)."""

    def __init__(self, frame_offsets, uv, xyz, device=0):
        self._h = C.c_void_p()
        off = np.ascontiguousarray(frame_offsets, dtype=np.int64)
        self.n_frames = len(off) - 1
        self.n_obs = int(off[-1])
        uv, xyz = _f32(uv), _f32(xyz)
        assert uv.size == 2 * self.n_obs and xyz.size == 3 * self.n_obs
        _check(lib().cc_intrinsics_create(C.c_int32(device), C.c_int64(self.n_frames),
                                          _p(off, C.c_int64), _p(uv, C.c_float), _p(xyz, C.c_float),
                                          C.byref(self._h)))

    def close(self):
        if self._h:
            lib().cc_intrinsics_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_state(self, intr, q, t, const_mask=0):
        intr, q, t = _f64(intr), _f64(q), _f64(t)
        assert intr.size == 9 and q.size == 4 * self.n_frames and t.size == 3 * self.n_frames
        _check(lib().cc_intrinsics_set_state(self._h, _p(intr, C.c_double), C.c_uint32(const_mask),
                                             _p(q, C.c_double), _p(t, C.c_double)))

    def reset(self):
        _check(lib().cc_intrinsics_reset(self._h))

    def get_state(self):
        intr = np.zeros(9)
        q = np.zeros((self.n_frames, 4))
        t = np.zeros((self.n_frames, 3))
        _check(lib().cc_intrinsics_get_state(self._h, _p(intr, C.c_double), _p(q, C.c_double),
                                             _p(t, C.c_double)))
        return intr, q, t

    def eval(self, want_blocks=True):
        blocks = np.zeros((self.n_frames, 16, 16)) if want_blocks else None
        cost = C.c_double()
        _check(lib().cc_intrinsics_eval(self._h, _p(blocks, C.c_double) if want_blocks else None,
                                        C.byref(cost)))
        return cost.value, blocks

    def solve(self, options=None, log_capacity=1024):
        opt = options if options is not None else default_options()
        s, log = _summary(log_capacity)
        _check(lib().cc_intrinsics_solve(self._h, C.byref(opt), C.byref(s)))
        return _summary_dict(s, log)

    def solve_lean(self, options):
        """cc_intrinsics_solve without a log and without building the Python summary (timing loops: the dictionary
        costs more host time per solve than the C call's own overhead). Returns the iteration count."""
        s = getattr(self, "_lean_summary", None)
        if s is None:
            s = self._lean_summary = Summary()
            s.log = None
            s.log_capacity = 0
        _check(lib().cc_intrinsics_solve(self._h, C.byref(options), C.byref(s)))
        return s.iterations

    def set_huber(self, a):
        """EXTENSION: ceres::HuberLoss(a), a in pixels, for later eval / solve / obs_cost calls (cc_intrinsics_set_huber);
        a <= 0 switches it off. With it on the handle solves in the two-kernel form."""
        _check(lib().cc_intrinsics_set_huber(self._h, C.c_double(a)))

    def set_final_sweep(self, mode):
        """The sweep of a persistent solve's last round (cc_intrinsics_set_final_sweep): 0 always full, 1 residual-only where the
        control predicts that the round's decision ends the solve (the default), 2 predicted at every accepting decision (tests)."""
        _check(lib().cc_intrinsics_set_final_sweep(self._h, C.c_int32(mode)))

    def final_sweep_counts(self):
        """(residual_only, redone) of the last persistent solve (cc_intrinsics_final_sweep_counts)."""
        a, b = C.c_int32(0), C.c_int32(0)
        _check(lib().cc_intrinsics_final_sweep_counts(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def set_model(self, model):
        """EXTENSION: the camera model of later set_state / eval / solve / obs_cost calls (cc_intrinsics_set_model):
        MODEL_RADTAN (the default) or MODEL_FISHEYE (slots fx fy px py k1 k2 k3 k4 -, slot 8 held at 0; two-kernel form).
        A change drops the state: call set_state next."""
        _check(lib().cc_intrinsics_set_model(self._h, C.c_int32(model)))

    def get_model(self):
        return int(lib().cc_intrinsics_get_model(self._h))

    def obs_cost(self):
        """The cost of every observation at the current point, in the caller's order (cc_intrinsics_obs_cost): 1/2 rho(s) with
        the Huber loss on, 1/2 |r|^2 with it off."""
        out = np.zeros(self.n_obs)
        _check(lib().cc_intrinsics_obs_cost(self._h, _p(out, C.c_double)))
        return out

    def estimate_start_fisheye(self, **options):
        """EXTENSION: a start of the fisheye solve from the handle's own pixels (cc_intrinsics_estimate_start_fisheye): a search
        over the focal length of the equidistant lens on bearing vectors, then every view's pose at the picked one. `options`:
        the fields of cc_intr_start_options (intr_start_options). Returns (intr [9] = f f cx cy 0 .., q [F, 4], t [F, 3], report);
        the handle's state is not touched: call set_state next."""
        o = intr_start_options(**options)
        intr, q, t = np.zeros(9), np.zeros((self.n_frames, 4)), np.zeros((self.n_frames, 3))
        r = IntrStartReport()
        _check(lib().cc_intrinsics_estimate_start_fisheye(self._h, C.byref(o), _p(intr, C.c_double), _p(q, C.c_double),
                                                          _p(t, C.c_double), C.byref(r)))
        return intr, q, t, _start_report_dict(r)

    def start_scores(self):
        """(f [C], score [C], qualified [C]) of the last estimate_start_fisheye's search (cc_intrinsics_start_scores): the
        candidate focal lengths, S_j = f_j^2 sum of the searched views' chord costs, and whether candidate j placed every view
        some candidate places."""
        f, score, qualified = np.zeros(64), np.zeros(64), np.full(64, -1, dtype=np.int32)
        _check(lib().cc_intrinsics_start_scores(self._h, _p(f, C.c_double), _p(score, C.c_double), _p(qualified, C.c_int32)))
        n = int((qualified >= 0).sum())   # (the library writes 0 or 1 for every candidate of the search, and only those)
        return f[:n].copy(), score[:n].copy(), qualified[:n].copy()

    def profile_sweep(self, n=50):
        ms = C.c_double()
        _check(lib().cc_intrinsics_profile_sweep(self._h, C.c_int32(n), C.byref(ms)))
        return ms.value

    def solver_form(self):
        """0: two kernels per LM iteration; 1, 2, 4: the persistent per-solve kernel with that many frames per workgroup."""
        return int(lib().cc_intrinsics_solver_form(self._h))

    def solver_status(self):
        """(form, reruns, note): cc_intrinsics_solver_status -- persistent solves that gave up and were run again, and why."""
        form, reruns = C.c_int32(), C.c_int32()
        note = C.create_string_buffer(2048)
        _check(lib().cc_intrinsics_solver_status(self._h, C.byref(form), C.byref(reruns), note, 2048))
        return form.value, reruns.value, note.value.decode()

    def profile_solve(self, options=None, n=20):
        """Persistent form: (average ms per launch = per complete solve, evaluations per launch), hipEvents on the solver's stream."""
        options = options if options is not None else default_options()
        ms, sw = C.c_double(), C.c_int32()
        _check(lib().cc_intrinsics_profile_solve(self._h, C.byref(options), C.c_int32(n), C.byref(ms), C.byref(sw)))
        return ms.value, sw.value

    def comm_init(self, unique_id, rank, nranks):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        _check(lib().cc_intrinsics_comm_init(self._h, buf, C.c_int32(rank), C.c_int32(nranks)))

    def exchange_export(self):
        """Allocate this rank's mailbox; returns the 64-byte IPC handle to all-gather."""
        buf = (C.c_uint8 * 64)()
        _check(lib().cc_intrinsics_exchange_export(self._h, buf))
        return bytes(buf)

    def exchange_attach(self, rank, handles):
        """handles: every rank's 64-byte handle, in rank order."""
        blob = b"".join(bytes(x) for x in handles)
        assert len(blob) == 64 * len(handles)
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        _check(lib().cc_intrinsics_exchange_attach(self._h, C.c_int32(rank), C.c_int32(len(handles)), buf))


def comm_get_unique_id():
    buf = (C.c_uint8 * 128)()
    _check(lib().cc_comm_get_unique_id(buf))
    return bytes(buf)


def _views(off, uv, xyz):
    """(uv_views, xyz_views, counts, keep-alive) for the *_views entry points: one pointer per view, each view its own
    array (as a vector<Points2D> holds them), not slices of one block."""
    F = len(off) - 1
    parts_uv = [np.array(uv.reshape(-1, 2)[off[f]:off[f + 1]], dtype=np.float32, order="C") for f in range(F)]
    parts_xyz = [np.array(xyz.reshape(-1, 3)[off[f]:off[f + 1]], dtype=np.float32, order="C") for f in range(F)]
    fp = C.POINTER(C.c_float)
    uv_views = (fp * F)(*[a.ctypes.data_as(fp) for a in parts_uv])
    xyz_views = (fp * F)(*[a.ctypes.data_as(fp) for a in parts_xyz])
    counts = np.ascontiguousarray(np.diff(off), dtype=np.int64)
    return uv_views, xyz_views, counts, (parts_uv, parts_xyz)


def intrinsics_optimize(frame_offsets, uv, xyz, intr, q, t, const_mask=0, options=None, device=0,
                        log_capacity=1024, devices=None, views=False, huber_a=0.0, model=0):
    """One-shot cc_intrinsics_optimize (devices=[...]: cc_intrinsics_optimize_multi, one host thread driving several
    devices; views=True: cc_intrinsics_optimize_views, every view handed over as its own array; huber_a > 0: the extension
    cc_intrinsics_optimize_views_huber, one device, views handed over as their own arrays; model != 0: the extension
    cc_intrinsics_optimize_views_model, likewise, with huber_a passed on). Returns (intr, q, t, summary)."""
    off = np.ascontiguousarray(frame_offsets, dtype=np.int64)
    F = len(off) - 1
    uv, xyz = _f32(uv), _f32(xyz)
    intr, q, t = _f64(intr).copy(), _f64(q).copy(), _f64(t).copy()
    opt = options if options is not None else default_options()
    s, log = _summary(log_capacity)
    # The symbol and what it takes behind the shared arguments. model 0 and huber_a <= 0 are off: the symbols without them; an
    # unknown model or a NaN threshold goes on to the C side, which refuses it.
    where, loss = (C.c_int32(device),), not huber_a <= 0
    if (model != 0 or loss) and devices is not None:
        raise ValueError(("model" if model != 0 else "huber_a") + " is for one device only")
    if model != 0:
        name, tail = "cc_intrinsics_optimize_views_model", (C.c_double(huber_a), C.c_int32(model))
    elif loss:
        name, tail = "cc_intrinsics_optimize_views_huber", (C.c_double(huber_a),)
    elif devices is not None:
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        name, tail, where = "cc_intrinsics_optimize_multi", (), (C.c_int32(len(devs)), _p(devs, C.c_int32))
    else:
        name, tail = "cc_intrinsics_optimize_views" if views else "cc_intrinsics_optimize", ()
    if "_views" in name:
        uv_views, xyz_views, counts, _keep = _views(off, uv, xyz)
        obs = (uv_views, xyz_views, _p(counts, C.c_int64))
    else:
        obs = (_p(off, C.c_int64), _p(uv, C.c_float), _p(xyz, C.c_float))
    _check(getattr(lib(), name)(C.byref(opt), *where, C.c_int64(F), *obs, _p(intr, C.c_double), C.c_uint32(const_mask),
                                _p(q, C.c_double), _p(t, C.c_double), C.byref(s), *tail))
    return intr, q, t, _summary_dict(s, log)


def intrinsics_estimate(frame_offsets, uv, xyz, distortion5=None, const_mask=0, options=None, device=0, log_capacity=1024,
                        views=False, huber_a=0.0, model=0, start="zhang", start_options=None):
    """cc_intrinsics_estimate (= Calibrator::Estimate: Zhang initialisation + solve, one upload; views=True:
    cc_intrinsics_estimate_views, every view handed over as its own array and packed by the library under its upload;
    huber_a > 0: the extension cc_intrinsics_estimate_views_huber, views handed over as their own arrays; model != 0: the
    extension cc_intrinsics_estimate_views_model, likewise, `distortion5` then holding the model's coefficients).
    start="fisheye": the extension cc_intrinsics_estimate_views_start, the focal-length search of estimate_start_fisheye in
    place of Zhang's initialisation (model must be MODEL_FISHEYE; start_options: a dict of cc_intr_start_options fields or an
    IntrStartOptions); start="zhang", the default, is the call as it was.
    Returns (K_init float32 3x3, intr, q, t, summary)."""
    if start not in ("zhang", "fisheye"):
        raise ValueError(f"start must be 'zhang' or 'fisheye', not {start!r}")
    if start == "zhang" and start_options is not None:
        raise ValueError("start_options belong to start='fisheye'")
    off = np.ascontiguousarray(frame_offsets, dtype=np.int64)
    F = len(off) - 1
    uv, xyz = _f32(uv), _f32(xyz)
    opt = options if options is not None else default_options()
    s, log = _summary(log_capacity)
    K = np.zeros(9, dtype=np.float32)
    intr, q, t = np.zeros(9), np.zeros((F, 4)), np.zeros((F, 3))
    d5 = _f64(distortion5) if distortion5 is not None else None
    # The symbol and what it takes behind the shared arguments. model 0 and huber_a <= 0 are off: the symbols without them; a
    # NaN threshold goes on to the C side, which refuses it.
    if start == "fisheye":
        so = start_options if isinstance(start_options, IntrStartOptions) else intr_start_options(**(start_options or {}))
        name, tail = "cc_intrinsics_estimate_views_start", (C.c_double(huber_a), C.c_int32(model), C.byref(so))
    elif model != 0:
        name, tail = "cc_intrinsics_estimate_views_model", (C.c_double(huber_a), C.c_int32(model))
    elif not huber_a <= 0:
        name, tail = "cc_intrinsics_estimate_views_huber", (C.c_double(huber_a),)
    else:
        name, tail = "cc_intrinsics_estimate_views" if views else "cc_intrinsics_estimate", ()
    if "_views" in name:
        uv_views, xyz_views, counts, _keep = _views(off, uv, xyz)
        obs = (uv_views, xyz_views, _p(counts, C.c_int64))
    else:
        obs = (_p(off, C.c_int64), _p(uv, C.c_float), _p(xyz, C.c_float))
    _check(getattr(lib(), name)(C.byref(opt), C.c_int32(device), C.c_int64(F), *obs, _p(d5, C.c_double) if d5 is not None else None,
                                C.c_uint32(const_mask), _p(K, C.c_float), _p(intr, C.c_double), _p(q, C.c_double),
                                _p(t, C.c_double), C.byref(s), *tail))
    return K.reshape(3, 3), intr, q, t, _summary_dict(s, log)


def _batch_layout(problems):
    """problems: one (frame_offsets, uv, xyz) per problem -> (problem_offsets [B+1], frame_offsets [Ftot+1], uv, xyz) of
    the concatenated batch, as cc_intrinsics_batch_* take it."""
    poff, foff, uvs, xyzs = [0], [0], [], []
    for off, uv, xyz in problems:
        off = np.ascontiguousarray(off, dtype=np.int64)
        uv, xyz = _f32(uv).reshape(-1, 2), _f32(xyz).reshape(-1, 3)
        assert off[0] == 0 and len(uv) == off[-1] and len(xyz) == off[-1]
        foff.extend((off[1:] + foff[-1]).tolist())
        poff.append(poff[-1] + len(off) - 1)
        uvs.append(uv)
        xyzs.append(xyz)
    uv = np.ascontiguousarray(np.concatenate(uvs), dtype=np.float32) if uvs else np.zeros((0, 2), np.float32)
    xyz = np.ascontiguousarray(np.concatenate(xyzs), dtype=np.float32) if xyzs else np.zeros((0, 3), np.float32)
    return np.array(poff, dtype=np.int64), np.array(foff, dtype=np.int64), uv, xyz


def _batch_summaries(B, log_capacity):
    logs = [(Iteration * max(1, log_capacity))() for _ in range(B)]
    ss = (Summary * B)()
    for p in range(B):
        ss[p].log = C.cast(logs[p], C.POINTER(Iteration))
        ss[p].log_capacity = log_capacity
    return ss, logs


class IntrinsicsBatch:
    """Handle on a batch of independent single-camera problems resident in HBM (cc_intrinsics_batch_*, an extension:
    the reference calibrates its cameras one after another). problems: one (frame_offsets, uv, xyz) per problem."""

    def __init__(self, problems, device=0):
        self._h = C.c_void_p()
        self.problem_offsets, self.frame_offsets, uv, xyz = _batch_layout(problems)
        self.n_problems = len(self.problem_offsets) - 1
        self.n_frames = int(self.problem_offsets[-1])
        _check(lib().cc_intrinsics_batch_create(C.c_int32(device), C.c_int64(self.n_problems), _p(self.problem_offsets, C.c_int64),
                                                _p(self.frame_offsets, C.c_int64), _p(uv, C.c_float), _p(xyz, C.c_float),
                                                C.byref(self._h)))

    def close(self):
        if self._h:
            lib().cc_intrinsics_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _split(self, a, width):
        a = a.reshape(-1, width)
        return [a[self.problem_offsets[p]:self.problem_offsets[p + 1]].copy() for p in range(self.n_problems)]

    def set_state(self, intr, q, t, const_mask=None):
        """intr: [B][9]; q, t: one array per problem ([F_p][4], [F_p][3]) or the concatenation; const_mask: one per problem."""
        intr = _f64(np.asarray(intr, dtype=np.float64).reshape(-1))
        q = _f64(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1, 4) for x in q]) if isinstance(q, (list, tuple)) else q)
        t = _f64(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in t]) if isinstance(t, (list, tuple)) else t)
        assert intr.size == 9 * self.n_problems and q.size == 4 * self.n_frames and t.size == 3 * self.n_frames
        mask = np.zeros(self.n_problems, dtype=np.uint32) if const_mask is None else np.ascontiguousarray(const_mask, dtype=np.uint32)
        assert mask.size == self.n_problems
        _check(lib().cc_intrinsics_batch_set_state(self._h, _p(intr, C.c_double), _p(mask, C.c_uint32), _p(q, C.c_double),
                                                   _p(t, C.c_double)))

    def set_huber(self, a_list):
        """EXTENSION: ceres::HuberLoss(a_list[p]), pixels, for problem p in later solves (cc_intrinsics_batch_set_huber);
        <= 0 leaves a problem without the loss, None switches it off for all."""
        if a_list is None:
            _check(lib().cc_intrinsics_batch_set_huber(self._h, None))
            return
        a = _f64(np.asarray(a_list, dtype=np.float64).reshape(-1))
        assert a.size == self.n_problems
        _check(lib().cc_intrinsics_batch_set_huber(self._h, _p(a, C.c_double)))

    def set_model(self, model):
        """EXTENSION: the camera model of the WHOLE batch in later set_state / solve / get_state calls
        (cc_intrinsics_batch_set_model): MODEL_RADTAN (the default) or MODEL_FISHEYE (slots fx fy px py k1 k2 k3 k4 -, slot 8
        held at 0 for every problem; one sweep per round for all problems, loss on or off). A change drops the state:
        set_state comes next. The Huber thresholds stay."""
        _check(lib().cc_intrinsics_batch_set_model(self._h, C.c_int32(model)))

    def get_model(self):
        model = C.c_int32(-1)
        _check(lib().cc_intrinsics_batch_get_model(self._h, C.byref(model)))
        return int(model.value)

    def get_state(self):
        """(intr [B][9], [q_p], [t_p]): the current point of every problem."""
        intr = np.zeros((self.n_problems, 9))
        q = np.zeros((self.n_frames, 4))
        t = np.zeros((self.n_frames, 3))
        _check(lib().cc_intrinsics_batch_get_state(self._h, _p(intr, C.c_double), _p(q, C.c_double), _p(t, C.c_double)))
        return intr, self._split(q, 4), self._split(t, 3)

    def solve(self, options=None, log_capacity=1024):
        """One summary dictionary per problem (as IntrinsicsProblem.solve returns)."""
        opt = options if options is not None else default_options()
        ss, logs = _batch_summaries(self.n_problems, log_capacity)
        _check(lib().cc_intrinsics_batch_solve(self._h, C.byref(opt), ss))
        return [_summary_dict(ss[p], logs[p]) for p in range(self.n_problems)]

    def solve_lean(self, options):
        """cc_intrinsics_batch_solve without logs or Python summaries (timing loops). Returns the iteration counts."""
        ss = getattr(self, "_lean", None)
        if ss is None:
            ss = self._lean = (Summary * self.n_problems)()
        _check(lib().cc_intrinsics_batch_solve(self._h, C.byref(options), ss))
        return [ss[p].iterations for p in range(self.n_problems)]

    def estimate_start_fisheye(self, **options):
        """EXTENSION: IntrinsicsProblem.estimate_start_fisheye for every problem of the batch at once
        (cc_intrinsics_batch_estimate_start_fisheye; the handle's model must be MODEL_FISHEYE): seven launches whatever the
        number of problems. `options`: the fields of cc_intr_start_options, one set for the whole batch. Returns
        (intr [B, 9], q [Ftot, 4], t [Ftot, 3], [report_p]); the handle's state is not touched. A problem without a qualified
        candidate raises; `last_start_reports` then holds every problem's report (best_candidate -1 marks such a problem)."""
        o = intr_start_options(**options)
        intr, q, t = np.zeros((self.n_problems, 9)), np.zeros((self.n_frames, 4)), np.zeros((self.n_frames, 3))
        r = (IntrStartReport * self.n_problems)()
        rc = lib().cc_intrinsics_batch_estimate_start_fisheye(self._h, C.byref(o), _p(intr, C.c_double), _p(q, C.c_double),
                                                              _p(t, C.c_double), r)
        self.last_start_reports = [_start_report_dict(r[p]) for p in range(self.n_problems)] if rc in (0, -5) else None
        _check(rc)
        return intr, q, t, self.last_start_reports

    def start_scores(self):
        """(f [B, C], score [B, C], qualified [B, C]) of the last estimate_start_fisheye's search
        (cc_intrinsics_batch_start_scores), per problem as IntrinsicsProblem.start_scores returns them."""
        n = 64 * self.n_problems
        f, score, qualified = np.zeros(n), np.zeros(n), np.full(n, -1, dtype=np.int32)
        _check(lib().cc_intrinsics_batch_start_scores(self._h, _p(f, C.c_double), _p(score, C.c_double), _p(qualified, C.c_int32)))
        c = int((qualified >= 0).sum()) // self.n_problems   # (the library writes 0 or 1 for every candidate of the search, and only those)
        shape = (self.n_problems, c)
        return f[:c * self.n_problems].reshape(shape).copy(), score[:c * self.n_problems].reshape(shape).copy(), qualified[:c * self.n_problems].reshape(shape).copy()


def intrinsics_batch_optimize(problems, intr, q, t, const_mask=None, options=None, device=0, log_capacity=1024, model=0):
    """One-shot cc_intrinsics_batch_optimize. problems: one (frame_offsets, uv, xyz) per problem; intr [B][9]; q, t: one array
    per problem. model != 0 (the extension, MODEL_FISHEYE for the whole batch): the same steps through a handle with
    cc_intrinsics_batch_set_model in front of set_state. Returns (intr [B][9], [q_p], [t_p], [summary_p])."""
    if model != 0:   # (0 is off: the one-shot symbol, below; an unknown value goes on to the C side, which refuses it)
        h = IntrinsicsBatch(problems, device=device)
        try:
            h.set_model(model)
            h.set_state(intr, q, t, const_mask)
            ss = h.solve(options, log_capacity)
            io, qs, ts = h.get_state()
        finally:
            h.close()
        return io, qs, ts, ss
    poff, foff, uv, xyz = _batch_layout(problems)
    B = len(poff) - 1
    intr = _f64(np.asarray(intr, dtype=np.float64).reshape(-1)).copy()
    q = _f64(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1, 4) for x in q])).copy()
    t = _f64(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in t])).copy()
    mask = np.zeros(B, dtype=np.uint32) if const_mask is None else np.ascontiguousarray(const_mask, dtype=np.uint32)
    opt = options if options is not None else default_options()
    ss, logs = _batch_summaries(B, log_capacity)
    _check(lib().cc_intrinsics_batch_optimize(C.byref(opt), C.c_int32(device), C.c_int64(B), _p(poff, C.c_int64), _p(foff, C.c_int64),
                                              _p(uv, C.c_float), _p(xyz, C.c_float), _p(intr, C.c_double), _p(mask, C.c_uint32),
                                              _p(q, C.c_double), _p(t, C.c_double), ss))
    qs = [q[poff[p]:poff[p + 1]].copy() for p in range(B)]
    ts = [t[poff[p]:poff[p + 1]].copy() for p in range(B)]
    return intr.reshape(B, 9), qs, ts, [_summary_dict(ss[p], logs[p]) for p in range(B)]


def intrinsics_batch_estimate(problems, distortion5=None, const_mask=None, options=None, device=0, log_capacity=1024, huber_a=None,
                              model=0, start="zhang", start_options=None):
    """cc_intrinsics_batch_estimate (Zhang initialisation per problem + the batched solve). distortion5: [B][5] or None;
    const_mask: one per problem or None; huber_a: one Huber threshold in pixels per problem (the extension
    cc_intrinsics_batch_estimate_huber) or None; model != 0: the extension cc_intrinsics_batch_estimate_model, one model for
    the whole batch, huber_a passed on, `distortion5` then [B][4] (k1..k4) or [B][5] with the fifth entry ignored.
    start="fisheye": the extension cc_intrinsics_batch_estimate_start, the batched focal-length search of
    IntrinsicsBatch.estimate_start_fisheye in place of the per-problem Zhang launches (model must be MODEL_FISHEYE;
    start_options: a dict of cc_intr_start_options fields or an IntrStartOptions, one for the whole batch); start="zhang" (or
    None), the default, is the call as it was.
    Returns (K_init float32 [B][3][3], intr [B][9], [q_p], [t_p], [summary_p])."""
    if start is None:
        start = "zhang"
    if start not in ("zhang", "fisheye"):
        raise ValueError(f"start must be 'zhang' or 'fisheye', not {start!r}")
    if start == "zhang" and start_options is not None:
        raise ValueError("start_options belong to start='fisheye'")
    poff, foff, uv, xyz = _batch_layout(problems)
    B, F = len(poff) - 1, int(poff[-1])
    K = np.zeros((B, 9), dtype=np.float32)
    intr, q, t = np.zeros((B, 9)), np.zeros((F, 4)), np.zeros((F, 3))
    if distortion5 is not None and model != 0:
        d = np.asarray(distortion5, dtype=np.float64).reshape(B, -1)
        distortion5 = np.concatenate([d[:, :4], np.zeros((B, 1))], axis=1)
    d5 = _f64(np.asarray(distortion5, dtype=np.float64).reshape(B, 5)) if distortion5 is not None else None
    mask = np.zeros(B, dtype=np.uint32) if const_mask is None else np.ascontiguousarray(const_mask, dtype=np.uint32)
    opt = options if options is not None else default_options()
    ss, logs = _batch_summaries(B, log_capacity)
    if start == "fisheye":
        so = start_options if isinstance(start_options, IntrStartOptions) else intr_start_options(**(start_options or {}))
    ha = None
    if huber_a is not None:
        ha = _f64(np.asarray(huber_a, dtype=np.float64).reshape(-1))
        assert ha.size == B
    ha_p = _p(ha, C.c_double) if ha is not None else None
    # The symbol and what it takes behind the shared arguments. model 0 is off: the symbols without a model argument; an unknown
    # value goes on to the C side, which refuses it.
    if start == "fisheye":
        name, tail = "cc_intrinsics_batch_estimate_start", (ha_p, C.c_int32(model), C.byref(so))
    elif model != 0:
        name, tail = "cc_intrinsics_batch_estimate_model", (ha_p, C.c_int32(model))
    elif ha is not None:
        name, tail = "cc_intrinsics_batch_estimate_huber", (ha_p,)
    else:
        name, tail = "cc_intrinsics_batch_estimate", ()
    _check(getattr(lib(), name)(C.byref(opt), C.c_int32(device), C.c_int64(B), _p(poff, C.c_int64), _p(foff, C.c_int64),
                                _p(uv, C.c_float), _p(xyz, C.c_float), _p(d5, C.c_double) if d5 is not None else None,
                                _p(mask, C.c_uint32), _p(K, C.c_float), _p(intr, C.c_double), _p(q, C.c_double),
                                _p(t, C.c_double), ss, *tail))
    qs = [q[poff[p]:poff[p + 1]].copy() for p in range(B)]
    ts = [t[poff[p]:poff[p + 1]].copy() for p in range(B)]
    return K.reshape(B, 3, 3), intr, qs, ts, [_summary_dict(ss[p], logs[p]) for p in range(B)]


HUBER_A = float(np.float32(3.0) / np.float32(500.0))  # extrinsics_calibrator.cpp:176


def release_caches():
    """cc_release_caches: hand the library's cached device / pinned memory back (idle pieces only)."""
    lib().cc_release_caches.restype = None
    lib().cc_release_caches()


class ObsLayout(C.Structure):
    _fields_ = [("stride", C.c_int64), ("camera_offset", C.c_int64), ("world_offset", C.c_int64), ("uv_offset", C.c_int64),
                ("cost_offset", C.c_int64)]


# one sighting as ExtrinsicsCalibrator keeps it (camera, point in frame, global point, normalised image point, cost)
SIGHTING = np.dtype([("camera", "<u8"), ("point_in_frame", "<u8"), ("world", "<u8"), ("uv", "<f4", (2,)), ("cost", "<f8")])


def rig_optimize_frames(n_cams, frame_offsets, obs_cam, obs_world, obs_uv, world_xyz, cam_q, cam_t, cam_frozen,
                        frame_q, frame_t, huber_a=HUBER_A, options=None, device=0, log_capacity=2048):
    """cc_rig_optimize_frames: the observations handed over frame by frame as arrays of SIGHTING records (one numpy array per
    frame, as the C++ class holds one vector per frame); the costs come back inside the records.
    Returns (cam_q, cam_t, frame_q, frame_t, obs_cost, summary) like rig_optimize."""
    off = np.ascontiguousarray(frame_offsets, dtype=np.int64)
    F = len(off) - 1
    obs_cam, obs_world = np.asarray(obs_cam), np.asarray(obs_world)
    uv = _f32(obs_uv).reshape(-1, 2)
    world_xyz = _f32(world_xyz)
    frames = []
    for f in range(F):
        a = np.zeros(int(off[f + 1] - off[f]), dtype=SIGHTING)
        a["camera"] = obs_cam[off[f]:off[f + 1]]
        a["world"] = obs_world[off[f]:off[f + 1]]
        a["uv"] = uv[off[f]:off[f + 1]]
        a["cost"] = -1.0
        frames.append(a)
    ptrs = (C.c_void_p * F)(*[a.ctypes.data if len(a) else None for a in frames])
    counts = np.ascontiguousarray(np.diff(off), dtype=np.int64)
    lay = ObsLayout(SIGHTING.itemsize, SIGHTING.fields["camera"][1], SIGHTING.fields["world"][1], SIGHTING.fields["uv"][1],
                    SIGHTING.fields["cost"][1])
    frozen = np.ascontiguousarray(cam_frozen, dtype=np.uint8)
    cam_q, cam_t = _f64(cam_q).copy(), _f64(cam_t).copy()
    frame_q, frame_t = _f64(frame_q).copy(), _f64(frame_t).copy()
    opt = options if options is not None else default_options(max_iterations=1000)
    s, log = _summary(log_capacity)
    _check(lib().cc_rig_optimize_frames(C.byref(opt), C.c_int32(device), C.c_int64(n_cams), C.c_int64(F),
                                        C.c_int64(world_xyz.size // 3), ptrs, _p(counts, C.c_int64), C.byref(lay),
                                        _p(world_xyz, C.c_float), _p(cam_q, C.c_double), _p(cam_t, C.c_double),
                                        _p(frozen, C.c_uint8), _p(frame_q, C.c_double), _p(frame_t, C.c_double),
                                        C.c_double(huber_a), C.byref(s)))
    cost = np.concatenate([a["cost"] for a in frames]) if F else np.zeros(0)
    return cam_q, cam_t, frame_q, frame_t, cost, _summary_dict(s, log)


class ObsColumns(C.Structure):
    _fields_ = [("camera", C.POINTER(C.c_void_p)), ("camera_stride", C.c_int64), ("camera_width", C.c_int32),
                ("world", C.POINTER(C.c_void_p)), ("world_stride", C.c_int64), ("world_width", C.c_int32),
                ("uv", C.POINTER(C.c_void_p)), ("uv_stride", C.c_int64),
                ("cost", C.POINTER(C.c_void_p)), ("cost_stride", C.c_int64)]


def rig_optimize_columns(n_cams, frame_offsets, obs_cam, obs_world, obs_uv, world_xyz, cam_q, cam_t, cam_frozen,
                         frame_q, frame_t, huber_a=HUBER_A, options=None, device=0, log_capacity=2048,
                         camera_dtype=np.uint32, world_dtype=np.uint64, want_cost=True):
    """cc_rig_optimize_columns: the observations handed over frame by frame as four arrays per frame (camera ids, world point ids,
    image points, costs -- what the C++ class holds since round 5); ids 4 or 8 bytes wide.
    Returns (cam_q, cam_t, frame_q, frame_t, obs_cost, summary) like rig_optimize (obs_cost None with want_cost=False)."""
    off = np.ascontiguousarray(frame_offsets, dtype=np.int64)
    F = len(off) - 1
    obs_cam, obs_world = np.asarray(obs_cam), np.asarray(obs_world)
    uv = _f32(obs_uv).reshape(-1, 2)
    world_xyz = _f32(world_xyz)
    cols = {"camera": [], "world": [], "uv": [], "cost": []}
    for f in range(F):
        a, b = int(off[f]), int(off[f + 1])
        cols["camera"].append(np.ascontiguousarray(obs_cam[a:b], dtype=camera_dtype))
        cols["world"].append(np.ascontiguousarray(obs_world[a:b], dtype=world_dtype))
        cols["uv"].append(np.ascontiguousarray(uv[a:b]))
        cols["cost"].append(np.full(b - a, -1.0))
    ptr = {k: (C.c_void_p * F)(*[x.ctypes.data if len(x) else None for x in v]) for k, v in cols.items()}
    oc = ObsColumns(ptr["camera"], np.dtype(camera_dtype).itemsize, np.dtype(camera_dtype).itemsize,
                    ptr["world"], np.dtype(world_dtype).itemsize, np.dtype(world_dtype).itemsize,
                    ptr["uv"], 8, ptr["cost"] if want_cost else None, 8)
    counts = np.ascontiguousarray(np.diff(off), dtype=np.int64)
    frozen = np.ascontiguousarray(cam_frozen, dtype=np.uint8)
    cam_q, cam_t = _f64(cam_q).copy(), _f64(cam_t).copy()
    frame_q, frame_t = _f64(frame_q).copy(), _f64(frame_t).copy()
    opt = options if options is not None else default_options(max_iterations=1000)
    s, log = _summary(log_capacity)
    _check(lib().cc_rig_optimize_columns(C.byref(opt), C.c_int32(device), C.c_int64(n_cams), C.c_int64(F),
                                         C.c_int64(world_xyz.size // 3), C.byref(oc), _p(counts, C.c_int64),
                                         _p(world_xyz, C.c_float), _p(cam_q, C.c_double), _p(cam_t, C.c_double),
                                         _p(frozen, C.c_uint8), _p(frame_q, C.c_double), _p(frame_t, C.c_double),
                                         C.c_double(huber_a), C.byref(s)))
    cost = (np.concatenate(cols["cost"]) if F else np.zeros(0)) if want_cost else None
    return cam_q, cam_t, frame_q, frame_t, cost, _summary_dict(s, log)


class RigStartOptions(C.Structure):
    _fields_ = [("refine_iterations", C.c_int32)]


class RigStartReport(C.Structure):
    _fields_ = [("views_valid", C.c_int64), ("views_planar", C.c_int64), ("views_general", C.c_int64), ("views_invalid", C.c_int64),
                ("frames_placed", C.c_int64), ("frames_unplaced", C.c_int64), ("cameras_placed", C.c_int32),
                ("cameras_unplaced", C.c_int32), ("root_camera", C.c_int32), ("root_at_identity", C.c_int32),
                ("parent", C.POINTER(C.c_int32))]


class RigProblem:
    """Handle on a rig pose problem resident in HBM (cc_rig_*)."""

    def __init__(self, n_cams, frame_offsets, obs_cam, obs_world, obs_uv, world_xyz, cam_frozen,
                 huber_a=HUBER_A, device=0, with_intrinsics=False):
        """with_intrinsics=True: the extension cc_rigk_create (pixel observations, 9 shared intrinsics);
        with_intrinsics="per_camera": cc_rigk_create_per_camera (one set of 9 per camera)."""
        self._h = C.c_void_p()
        self.with_intrinsics = bool(with_intrinsics)
        self.per_camera = with_intrinsics == "per_camera"
        off = np.ascontiguousarray(frame_offsets, dtype=np.int64)
        self.n_cams, self.n_frames, self.n_obs = int(n_cams), len(off) - 1, int(off[-1])
        obs_cam = np.ascontiguousarray(obs_cam, dtype=np.uint32)
        obs_world = np.ascontiguousarray(obs_world, dtype=np.uint64)
        obs_uv, world_xyz = _f32(obs_uv), _f32(world_xyz)
        frozen = np.ascontiguousarray(cam_frozen, dtype=np.uint8)
        create = (lib().cc_rigk_create_per_camera if self.per_camera else lib().cc_rigk_create) if with_intrinsics else lib().cc_rig_create
        _check(create(C.c_int32(device), C.c_int64(n_cams), C.c_int64(self.n_frames),
                                   C.c_int64(world_xyz.size // 3), _p(off, C.c_int64),
                                   _p(obs_cam, C.c_uint32), _p(obs_world, C.c_uint64),
                                   _p(obs_uv, C.c_float), _p(world_xyz, C.c_float),
                                   _p(frozen, C.c_uint8), C.c_double(huber_a), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().cc_rig_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_state(self, cam_q, cam_t, frame_q, frame_t):
        cam_q, cam_t, frame_q, frame_t = _f64(cam_q), _f64(cam_t), _f64(frame_q), _f64(frame_t)
        assert cam_q.size == 4 * self.n_cams and frame_q.size == 4 * self.n_frames
        _check(lib().cc_rig_set_state(self._h, _p(cam_q, C.c_double), _p(cam_t, C.c_double),
                                      _p(frame_q, C.c_double), _p(frame_t, C.c_double)))

    def set_intrinsics(self, intr9, const_mask=0):
        intr9 = _f64(intr9)
        assert intr9.size == 9
        _check(lib().cc_rigk_set_intrinsics(self._h, _p(intr9, C.c_double), C.c_uint32(const_mask)))

    def get_intrinsics(self):
        out = np.zeros(9)
        _check(lib().cc_rigk_get_intrinsics(self._h, _p(out, C.c_double)))
        return out

    def set_camera_intrinsics(self, camera, intr9, const_mask=0):
        intr9 = _f64(intr9)
        assert intr9.size == 9
        _check(lib().cc_rigk_set_camera_intrinsics(self._h, C.c_int64(camera), _p(intr9, C.c_double), C.c_uint32(const_mask)))

    def set_model(self, model):
        """The pixel model of every camera of a with_intrinsics handle (cc_rigk_set_model): MODEL_RADTAN (the default) or
        MODEL_FISHEYE (slots fx fy px py k1 k2 k3 k4 -, slot 8 held at 0; tile form of the sweep, one device). A change drops
        the intrinsics: set_intrinsics again before the next solve."""
        _check(lib().cc_rigk_set_model(self._h, C.c_int32(model)))

    def get_model(self):
        out = C.c_int32(0)
        _check(lib().cc_rigk_get_model(self._h, C.byref(out)))
        return int(out.value)

    def set_camera_model(self, camera, model):
        """The pixel model of ONE camera of a with_intrinsics="per_camera" handle (cc_rigk_set_camera_model). A change drops
        that camera's intrinsics only: set_camera_intrinsics(camera, ...) again before the next solve. get_model then reports
        MODEL_MIXED when the cameras differ."""
        _check(lib().cc_rigk_set_camera_model(self._h, C.c_int64(camera), C.c_int32(model)))

    def get_camera_model(self, camera=None):
        """One camera's model, or (camera=None) the list of all of them (cc_rigk_get_camera_model)."""
        if camera is None:
            return [self.get_camera_model(c) for c in range(self.n_cams)]
        out = C.c_int32(0)
        _check(lib().cc_rigk_get_camera_model(self._h, C.c_int64(camera), C.byref(out)))
        return int(out.value)

    def get_camera_intrinsics(self, camera=None):
        """One camera's set, or (camera=None) an [n_cams, 9] array of all of them."""
        if camera is None:
            return np.stack([self.get_camera_intrinsics(c) for c in range(self.n_cams)])
        out = np.zeros(9)
        _check(lib().cc_rigk_get_camera_intrinsics(self._h, C.c_int64(camera), _p(out, C.c_double)))
        return out

    def reset(self):
        _check(lib().cc_rig_reset(self._h))

    def solve(self, options=None, log_capacity=2048):
        opt = options if options is not None else default_options(max_iterations=1000)
        s, log = _summary(log_capacity)
        _check(lib().cc_rig_solve(self._h, C.byref(opt), C.byref(s)))
        return _summary_dict(s, log)

    def get_state(self, want_cost=True):
        cq, ct = np.zeros((self.n_cams, 4)), np.zeros((self.n_cams, 3))
        fq, ft = np.zeros((self.n_frames, 4)), np.zeros((self.n_frames, 3))
        cost = np.zeros(self.n_obs) if want_cost else None
        _check(lib().cc_rig_get_state(self._h, _p(cq, C.c_double), _p(ct, C.c_double), _p(fq, C.c_double),
                                      _p(ft, C.c_double), _p(cost, C.c_double) if want_cost else None))
        return cq, ct, fq, ft, cost

    def solver_form(self):
        """2: the whole solve as one launch of the lean persistent kernel; 0: three kernels per LM iteration."""
        return int(lib().cc_rig_solver_form(self._h))

    def solver_status(self):
        """(form, reruns, note): cc_rig_solver_status -- lean persistent solves that gave up and were run again, and why."""
        form, reruns = C.c_int32(), C.c_int32()
        note = C.create_string_buffer(1024)
        _check(lib().cc_rig_solver_status(self._h, C.byref(form), C.byref(reruns), note, 1024))
        return form.value, reruns.value, note.value.decode()

    def eval(self):
        c = C.c_double()
        _check(lib().cc_rig_eval(self._h, C.byref(c)))
        return c.value

    def set_inner_iterations(self, enable=True, tolerance=1e-3):
        """Ceres' inner iterations for later solves (cc_rig_set_inner_iterations; poses only, one device, off by default)."""
        _check(lib().cc_rig_set_inner_iterations(self._h, C.c_int32(1 if enable else 0), C.c_double(tolerance)))

    def inner_pass(self):
        """One inner pass from the current state (cc_rig_inner_pass): (cost_before, cost_after, mini_iterations[4])."""
        c0, c1 = C.c_double(), C.c_double()
        it = (C.c_int32 * 4)()
        _check(lib().cc_rig_inner_pass(self._h, C.byref(c0), C.byref(c1), it))
        return c0.value, c1.value, [int(v) for v in it]

    def inner_status(self):
        """The last solve's inner iterations (cc_rig_inner_status): dict of passes, useful_passes, enabled_at_end, cost_removed."""
        p, u, e = C.c_int32(), C.c_int32(), C.c_int32()
        r = C.c_double()
        _check(lib().cc_rig_inner_status(self._h, C.byref(p), C.byref(u), C.byref(e), C.byref(r)))
        return dict(passes=p.value, useful_passes=u.value, enabled_at_end=e.value, cost_removed=r.value)

    def estimate_start(self, cam_q=None, cam_t=None, frame_q=None, frame_t=None, refine_iterations=10):
        """Start poses from the handle's own observations (cc_rig_estimate_start): they become the handle's state as set_state
        would have set it. The four arrays are the caller's poses (None: the identity), kept for frozen cameras, cameras without
        a path to the root and frames without a valid view. Returns the report as a dict (parent: one entry per camera)."""
        return self._estimate_start(lib().cc_rig_estimate_start, cam_q, cam_t, frame_q, frame_t, refine_iterations)

    def estimate_start_pixels(self, cam_q=None, cam_t=None, frame_q=None, frame_t=None, refine_iterations=10):
        """estimate_start for a with_intrinsics handle (cc_rigk_estimate_start): the pixels go through the inverse of the handle's
        pixel model at its START intrinsics (set_intrinsics / set_camera_intrinsics) first; a pixel without a root makes its view
        invalid. Same arguments and report; the intrinsics are not written."""
        return self._estimate_start(lib().cc_rigk_estimate_start, cam_q, cam_t, frame_q, frame_t, refine_iterations)

    def estimate_start_bearings(self, cam_q=None, cam_t=None, frame_q=None, frame_t=None, refine_iterations=10):
        """estimate_start_pixels on unit bearings instead of x / z (cc_rigk_estimate_start_bearing): for rigs whose points reach
        or pass 90 degrees off the optical axis. Same arguments and report; the intrinsics are not written."""
        return self._estimate_start(lib().cc_rigk_estimate_start_bearing, cam_q, cam_t, frame_q, frame_t, refine_iterations)

    def _estimate_start(self, call, cam_q, cam_t, frame_q, frame_t, refine_iterations):
        opt = RigStartOptions(refine_iterations=int(refine_iterations))
        rep = RigStartReport()
        parent = np.full(self.n_cams, -1, dtype=np.int32)
        rep.parent = _p(parent, C.c_int32)
        arrs = []
        for a, n in ((cam_q, 4 * self.n_cams), (cam_t, 3 * self.n_cams), (frame_q, 4 * self.n_frames), (frame_t, 3 * self.n_frames)):
            if a is not None:
                a = _f64(a)
                assert a.size == n
            arrs.append(a)
        _check(call(self._h, C.byref(opt), *[_p(a, C.c_double) if a is not None else None for a in arrs], C.byref(rep)))
        out = {k: int(getattr(rep, k)) for k, _ in RigStartReport._fields_ if k != "parent"}
        out["parent"] = parent
        return out

    def start_views(self):
        """What the last estimate_start computed per view (cc_rig_start_views), in (frame, camera) order: dict of camera, frame,
        kind (0 invalid, 1 planar, 2 general), q [n, 4], t [n, 3], rms2 [n]."""
        n = C.c_int64(0)
        _check(lib().cc_rig_start_views(self._h, C.byref(n), None, None, None, None, None, None))
        n = int(n.value)
        cam, frame, kind = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
        q, t, rms2 = np.zeros((n, 4)), np.zeros((n, 3)), np.zeros(n)
        nn = C.c_int64(0)
        _check(lib().cc_rig_start_views(self._h, C.byref(nn), _p(cam, C.c_int32), _p(frame, C.c_int64), _p(kind, C.c_int32),
                                        _p(q, C.c_double), _p(t, C.c_double), _p(rms2, C.c_double)))
        return dict(camera=cam, frame=frame, kind=kind, q=q, t=t, rms2=rms2)

    def start_points(self):
        """(uv [n_obs, 2] float32, n_without_root): the normalised image points the last estimate_start_pixels used, in the
        caller's observation order (NaN, NaN: no root), and how many of them are NaN (cc_rigk_start_points)."""
        uv = np.zeros((self.n_obs, 2), dtype=np.float32)
        bad = C.c_int64(0)
        _check(lib().cc_rigk_start_points(self._h, _p(uv, C.c_float), C.byref(bad)))
        return uv, int(bad.value)

    def start_bearings(self):
        """(b [n_obs, 3] float32, n_without_root): the unit bearings the last estimate_start_bearings used, in the caller's
        observation order (NaN x 3: no root), and how many of them are NaN (cc_rigk_start_bearings)."""
        b = np.zeros((self.n_obs, 3), dtype=np.float32)
        bad = C.c_int64(0)
        _check(lib().cc_rigk_start_bearings(self._h, _p(b, C.c_float), C.byref(bad)))
        return b, int(bad.value)

    def comm_init(self, unique_id, rank, nranks):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        _check(lib().cc_rig_comm_init(self._h, buf, C.c_int32(rank), C.c_int32(nranks)))

    def exchange_export(self):
        buf = (C.c_uint8 * 64)()
        _check(lib().cc_rig_exchange_export(self._h, buf))
        return bytes(buf)

    def exchange_attach(self, rank, handles):
        """Collective: every rank calls it with all handles in rank order."""
        blob = b"".join(bytes(x) for x in handles)
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        _check(lib().cc_rig_exchange_attach(self._h, C.c_int32(rank), C.c_int32(len(handles)), buf))


def rig_optimize(n_cams, frame_offsets, obs_cam, obs_world, obs_uv, world_xyz, cam_q, cam_t, cam_frozen,
                 frame_q, frame_t, huber_a=HUBER_A, options=None, device=0, log_capacity=2048, devices=None):
    """One-shot cc_rig_optimize (devices=[...]: cc_rig_optimize_multi). Returns (cam_q, cam_t, frame_q, frame_t, obs_cost, summary)."""
    off = np.ascontiguousarray(frame_offsets, dtype=np.int64)
    F = len(off) - 1
    obs_cam = np.ascontiguousarray(obs_cam, dtype=np.uint32)
    obs_world = np.ascontiguousarray(obs_world, dtype=np.uint64)
    obs_uv, world_xyz = _f32(obs_uv), _f32(world_xyz)
    frozen = np.ascontiguousarray(cam_frozen, dtype=np.uint8)
    cam_q, cam_t = _f64(cam_q).copy(), _f64(cam_t).copy()
    frame_q, frame_t = _f64(frame_q).copy(), _f64(frame_t).copy()
    cost = np.zeros(len(obs_cam))
    opt = options if options is not None else default_options(max_iterations=1000)
    s, log = _summary(log_capacity)
    if devices is not None:
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        _check(lib().cc_rig_optimize_multi(C.byref(opt), C.c_int32(len(devs)), _p(devs, C.c_int32), C.c_int64(n_cams), C.c_int64(F),
                                           C.c_int64(world_xyz.size // 3), _p(off, C.c_int64), _p(obs_cam, C.c_uint32),
                                           _p(obs_world, C.c_uint64), _p(obs_uv, C.c_float), _p(world_xyz, C.c_float),
                                           _p(cam_q, C.c_double), _p(cam_t, C.c_double), _p(frozen, C.c_uint8),
                                           _p(frame_q, C.c_double), _p(frame_t, C.c_double), C.c_double(huber_a),
                                           _p(cost, C.c_double), C.byref(s)))
        return cam_q, cam_t, frame_q, frame_t, cost, _summary_dict(s, log)
    _check(lib().cc_rig_optimize(C.byref(opt), C.c_int32(device), C.c_int64(n_cams), C.c_int64(F),
                                 C.c_int64(world_xyz.size // 3), _p(off, C.c_int64), _p(obs_cam, C.c_uint32),
                                 _p(obs_world, C.c_uint64), _p(obs_uv, C.c_float), _p(world_xyz, C.c_float),
                                 _p(cam_q, C.c_double), _p(cam_t, C.c_double), _p(frozen, C.c_uint8),
                                 _p(frame_q, C.c_double), _p(frame_t, C.c_double), C.c_double(huber_a),
                                 _p(cost, C.c_double), C.byref(s)))
    return cam_q, cam_t, frame_q, frame_t, cost, _summary_dict(s, log)


def rig_estimate(n_cams, frame_offsets, obs_cam, obs_world, obs_uv, world_xyz, cam_frozen, cam_q=None, cam_t=None, frame_q=None,
                 frame_t=None, huber_a=HUBER_A, options=None, device=0, log_capacity=2048):
    """One-shot cc_rig_estimate: start poses from the observations, then the solve. The pose arrays are the caller's poses
    (None: the identity). Returns (cam_q, cam_t, frame_q, frame_t, obs_cost, summary)."""
    off = np.ascontiguousarray(frame_offsets, dtype=np.int64)
    F = len(off) - 1
    obs_cam = np.ascontiguousarray(obs_cam, dtype=np.uint32)
    obs_world = np.ascontiguousarray(obs_world, dtype=np.uint64)
    obs_uv, world_xyz = _f32(obs_uv), _f32(world_xyz)
    frozen = np.ascontiguousarray(cam_frozen, dtype=np.uint8)
    ident = np.array([1.0, 0.0, 0.0, 0.0])
    cam_q = np.tile(ident, (n_cams, 1)) if cam_q is None else _f64(cam_q).copy()
    cam_t = np.zeros((n_cams, 3)) if cam_t is None else _f64(cam_t).copy()
    frame_q = np.tile(ident, (F, 1)) if frame_q is None else _f64(frame_q).copy()
    frame_t = np.zeros((F, 3)) if frame_t is None else _f64(frame_t).copy()
    cost = np.zeros(len(obs_cam))
    opt = options if options is not None else default_options(max_iterations=1000)
    s, log = _summary(log_capacity)
    _check(lib().cc_rig_estimate(C.byref(opt), C.c_int32(device), C.c_int64(n_cams), C.c_int64(F),
                                 C.c_int64(world_xyz.size // 3), _p(off, C.c_int64), _p(obs_cam, C.c_uint32),
                                 _p(obs_world, C.c_uint64), _p(obs_uv, C.c_float), _p(world_xyz, C.c_float),
                                 _p(cam_q, C.c_double), _p(cam_t, C.c_double), _p(frozen, C.c_uint8),
                                 _p(frame_q, C.c_double), _p(frame_t, C.c_double), C.c_double(huber_a),
                                 _p(cost, C.c_double), C.byref(s)))
    return cam_q, cam_t, frame_q, frame_t, cost, _summary_dict(s, log)


def rigk_estimate(n_cams, frame_offsets, obs_cam, obs_world, obs_uv_pixels, world_xyz, cam_frozen, intr, const_mask=0, model=MODEL_RADTAN,
                  per_camera=False, cam_q=None, cam_t=None, frame_q=None, frame_t=None, huber_a=0.0, options=None, device=0,
                  log_capacity=2048, start="pinhole"):
    """Start, then solve, for the rig problem with intrinsics: a with_intrinsics handle (per_camera: one set per camera), its
    model (one, or with per_camera a sequence of n_cams: set_camera_model, applied before the intrinsics), intr ([9], or
    [n_cams, 9] per camera) and const_mask (one, or one per camera) as the start intrinsics,
    estimate_start_pixels (start="pinhole") or estimate_start_bearings (start="bearing": points at or beyond 90 degrees off the
    axis) with the pose arrays as the caller's poses (None: the identity), solve. Returns
    (intr, cam_q, cam_t, frame_q, frame_t, obs_cost, summary, report); intr is [9], or [n_cams, 9] per camera."""
    if start not in ("pinhole", "bearing"):
        raise ValueError("rigk_estimate: start must be 'pinhole' or 'bearing', not %r" % (start,))
    models = None
    if not np.isscalar(model):
        models = [int(m) for m in model]
        if not per_camera:
            raise ValueError("rigk_estimate: a model per camera needs per_camera=True (one shared set cannot follow two models)")
        if len(models) != n_cams:
            raise ValueError("rigk_estimate: %d models for %d cameras" % (len(models), n_cams))
    p = RigProblem(n_cams, frame_offsets, obs_cam, obs_world, obs_uv_pixels, world_xyz, cam_frozen, huber_a=huber_a, device=device,
                   with_intrinsics="per_camera" if per_camera else True)
    try:
        if models is None:
            p.set_model(model)
        else:
            for c, m in enumerate(models):
                p.set_camera_model(c, m)
        intr = _f64(intr)
        if per_camera and intr.ndim == 2:
            masks = np.broadcast_to(np.asarray(const_mask, dtype=np.int64), (n_cams,))
            for c in range(n_cams):
                p.set_camera_intrinsics(c, intr[c], int(masks[c]))
        else:
            p.set_intrinsics(intr, int(const_mask))
        report = (p.estimate_start_bearings if start == "bearing" else p.estimate_start_pixels)(cam_q, cam_t, frame_q, frame_t)
        summary = p.solve(options, log_capacity=log_capacity)
        out = p.get_camera_intrinsics() if per_camera else p.get_intrinsics()
        return (out,) + p.get_state() + (summary, report)
    finally:
        p.close()


def zhang_init(frame_offsets, uv, xyz, device=0, want_homographies=False):
    """cc_zhang_init: returns (K 3x3 float32, q [F,4] float32, t [F,3] float32[, H [F,3,3]])."""
    off = np.ascontiguousarray(frame_offsets, dtype=np.int64)
    F = len(off) - 1
    uv, xyz = _f32(uv), _f32(xyz)
    K = np.zeros(9, dtype=np.float32)
    q = np.zeros((F, 4), dtype=np.float32)
    t = np.zeros((F, 3), dtype=np.float32)
    H = np.zeros((F, 3, 3), dtype=np.float32)
    _check(lib().cc_zhang_init(C.c_int32(device), C.c_int64(F), _p(off, C.c_int64), _p(uv, C.c_float),
                               _p(xyz, C.c_float), _p(K, C.c_float), _p(q, C.c_float), _p(t, C.c_float),
                               _p(H, C.c_float) if want_homographies else None))
    return (K.reshape(3, 3), q, t, H) if want_homographies else (K.reshape(3, 3), q, t)


def distort(K, dist, xy, device=0, model=0):
    """cc_distort; model=MODEL_FISHEYE: the extension cc_distort_fisheye, dist = k1 k2 k3 k4."""
    xy = _f32(xy)
    out = np.zeros_like(xy)
    if model != 0:
        if model != MODEL_FISHEYE:
            raise ValueError(f"unknown model {model}")
        _check(lib().cc_distort_fisheye(C.c_int32(device), _p(_f32(K), C.c_float), _p(_f32(np.asarray(dist).reshape(-1)[:4]), C.c_float),
                                        C.c_int64(xy.size // 2), _p(xy, C.c_float), _p(out, C.c_float)))
        return out
    _check(lib().cc_distort(C.c_int32(device), _p(_f32(K), C.c_float), _p(_f32(dist), C.c_float),
                            C.c_int64(xy.size // 2), _p(xy, C.c_float), _p(out, C.c_float)))
    return out


def undistort(K, dist, uv, device=0, model=0):
    """cc_undistort; model=MODEL_FISHEYE: the extension cc_undistort_fisheye, dist = k1 k2 k3 k4."""
    uv = _f32(uv)
    out = np.zeros_like(uv)
    if model != 0:
        if model != MODEL_FISHEYE:
            raise ValueError(f"unknown model {model}")
        _check(lib().cc_undistort_fisheye(C.c_int32(device), _p(_f32(K), C.c_float), _p(_f32(np.asarray(dist).reshape(-1)[:4]), C.c_float),
                                          C.c_int64(uv.size // 2), _p(uv, C.c_float), _p(out, C.c_float)))
        return out
    _check(lib().cc_undistort(C.c_int32(device), _p(_f32(K), C.c_float), _p(_f32(dist), C.c_float),
                              C.c_int64(uv.size // 2), _p(uv, C.c_float), _p(out, C.c_float)))
    return out


# ---- synthetic-input harness (include/cc_harness.h): the reference's DataGenerator without OpenCV ----
# fixture constants of src/test_calibrator.cpp:11-21
FIXTURE_W, FIXTURE_H = 1600, 1000
FIXTURE_K = np.array([[1000, 0, 800], [0, 1000, 500], [0, 0, 1]], dtype=np.float32)
FIXTURE_DIST = np.array([-4.0e-2, 5e-4, 1.0e-3, 2.0e-5, -3e-4], dtype=np.float32)
FIXTURE_NOISE = 0.5


class Generator:
    def __init__(self, width=FIXTURE_W, height=FIXTURE_H, K=FIXTURE_K, dist=FIXTURE_DIST, noise=FIXTURE_NOISE):
        self._g = C.c_void_p(lib().cc_generator_create(C.c_int32(width), C.c_int32(height)))
        lib().cc_generator_set_k(self._g, _p(_f32(K), C.c_float))
        lib().cc_generator_set_distortion(self._g, _p(_f32(dist), C.c_float))
        lib().cc_generator_set_noise(self._g, C.c_float(noise))

    def __del__(self):
        if getattr(self, "_g", None):
            lib().cc_generator_destroy(self._g)
            self._g = None

    def planar(self, num_p=100):
        uv = np.zeros((num_p, 2), dtype=np.float32)
        xyz = np.zeros((num_p, 3), dtype=np.float32)
        n = lib().cc_generator_planar(self._g, C.c_int32(num_p), _p(uv, C.c_float), _p(xyz, C.c_float))
        assert n == num_p
        return uv, xyz

    def points(self, num_p=100):
        uv = np.zeros((num_p, 2), dtype=np.float32)
        xyz = np.zeros((num_p, 3), dtype=np.float32)
        n = lib().cc_generator_points(self._g, C.c_int32(num_p), _p(uv, C.c_float), _p(xyz, C.c_float))
        assert n == num_p
        return uv, xyz


def make_intrinsics_problem(n_frames, pts_per_frame, **gen_kw):
    """One GetDistortedPointsPlanar call per frame (src/test_calibrator.cpp:52-60); pts_per_frame may be ragged."""
    g = Generator(**gen_kw)
    counts = [pts_per_frame] * n_frames if np.isscalar(pts_per_frame) else list(pts_per_frame)
    uvs, xyzs = [], []
    for m in counts:
        uv, xyz = g.planar(int(m))
        uvs.append(uv)
        xyzs.append(xyz)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return offsets, np.concatenate(uvs), np.concatenate(xyzs)


def rig_scenario(n_cams, n_frames, pts_per_frame, seed=0):
    """cc_rig_scenario: the reference's rig test scenario (test_extrinsics_calibrator.cpp:48-134) at any size."""
    C_, F, M = int(n_cams), int(n_frames), int(pts_per_frame)
    cam_T = np.zeros((C_, 16), dtype=np.float32)
    cam_T_true = np.zeros((C_, 16), dtype=np.float32)
    frame_T = np.zeros((F, 16), dtype=np.float32)
    world = np.zeros((F * M, 3), dtype=np.float32)
    n = F * M * C_
    obs_cam = np.zeros(n, dtype=np.uint32)
    obs_world = np.zeros(n, dtype=np.uint64)
    obs_uv = np.zeros((n, 2), dtype=np.float32)
    lib().cc_rig_scenario(C.c_int32(C_), C.c_int32(F), C.c_int32(M), C.c_uint32(seed), _p(cam_T, C.c_float),
                          _p(cam_T_true, C.c_float), _p(frame_T, C.c_float), _p(world, C.c_float),
                          _p(obs_cam, C.c_uint32), _p(obs_world, C.c_uint64), _p(obs_uv, C.c_float))
    return dict(cam_T=cam_T, cam_T_true=cam_T_true, frame_T=frame_T, world_xyz=world, obs_cam=obs_cam,
                obs_world=obs_world, obs_uv=obs_uv, frame_offsets=(np.arange(F + 1) * M * C_).astype(np.int64),
                cam_frozen=np.array([1] + [0] * (C_ - 1), dtype=np.uint8))


def affine_to_qt(T16):
    """cc_affine_to_qt on every row: (q [n,4] w x y z, t [n,3]) in fp64."""
    T16 = _f32(T16).reshape(-1, 16)
    q = np.zeros((T16.shape[0], 4))
    t = np.zeros((T16.shape[0], 3))
    for i in range(T16.shape[0]):
        lib().cc_affine_to_qt(_p(T16[i], C.c_float), _p(q[i], C.c_double), _p(t[i], C.c_double))
    return q, t
