"""The refusal cases of the one-shot intrinsics calls (cc_intrinsics_optimize / _estimate and their _views, _huber, _model, _start
forms; cc_intrinsics_batch_optimize / _estimate and its forms) that tests/test_oneshot_contract_cpu.py replays and
scripts/record_oneshot_refusals.py records into tests/golden/oneshot_refusals.json: every case is one call on zeros, on device
-1 (no device on any machine), whose answer is decided by the argument checks -- or, when it passes them all, by the device.

A case is (name, kind, symbol, keywords); run(lib, case) makes the call on the library given (a ctypes.CDLL) and returns
(return code, cc_last_error() text). No GPU is needed."""
import ctypes as C

import numpy as np

from camera_calibrator_amd import capi

SINGLE = ("cc_intrinsics_optimize", "cc_intrinsics_optimize_views", "cc_intrinsics_optimize_views_huber", "cc_intrinsics_optimize_views_model",
          "cc_intrinsics_estimate", "cc_intrinsics_estimate_views", "cc_intrinsics_estimate_views_huber", "cc_intrinsics_estimate_views_model",
          "cc_intrinsics_estimate_views_start")
BATCH = ("cc_intrinsics_batch_optimize", "cc_intrinsics_batch_estimate", "cc_intrinsics_batch_estimate_huber", "cc_intrinsics_batch_estimate_model",
         "cc_intrinsics_batch_estimate_start")
NAN = float("nan")
FISH = capi.MODEL_FISHEYE


def _p(a, ty):
    return a.ctypes.data_as(C.POINTER(ty)) if a is not None else None


def _tail(lib, sym, huber, model, start, keep):
    """The arguments behind the summary: the loss, the model, the start -- as far as the symbol has them."""
    tail = ()
    if sym.endswith(("_huber", "_model", "_start")):
        tail += (huber,)
    if sym.endswith(("_model", "_start")):
        tail += (C.c_int32(model),)
    if sym.endswith("_start"):
        so = None
        if start is not None:   # a dict of cc_intr_start_options fields over the library's defaults
            so = capi.IntrStartOptions()
            lib.cc_intr_start_options_init(C.byref(so))
            for k, v in start.items():
                setattr(so, k, v)
            keep.append(so)
        tail += (C.byref(so) if so is not None else None,)
    return tail


def _single(lib, sym, frames=3, outputs=True, huber=0.0, model=0, start=None, short=None, null_view=None, null_xyz_view=None, off=None):
    """frames views of 4 points (short: (view, points) for one of them; null_view / null_xyz_view: the view whose uv / xyz pointer is
    NULL); off: the packed offsets in place of the honest ones."""
    counts = np.full(max(frames, 1), 4, dtype=np.int64)
    if short is not None:
        counts[short[0]] = short[1]
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64) if off is None else np.array(off, dtype=np.int64)
    n = int(counts.sum())
    uv, xyz = np.zeros((n, 2), np.float32), np.zeros((n, 3), np.float32)
    intr, q, t, K = np.zeros(9), np.zeros((len(counts), 4)), np.zeros((len(counts), 3)), np.zeros(9, np.float32)
    keep = []
    if "_views" in sym:
        fp = C.POINTER(C.c_float)
        parts = [(np.zeros((c, 2), np.float32), np.zeros((c, 3), np.float32)) for c in counts]
        uvv = (fp * len(counts))(*[None if i == null_view else a.ctypes.data_as(fp) for i, (a, _) in enumerate(parts)])
        xyzv = (fp * len(counts))(*[None if i == null_xyz_view else b.ctypes.data_as(fp) for i, (_, b) in enumerate(parts)])
        keep.append(parts)
        obs = (uvv, xyzv, _p(counts, C.c_int64))
    else:
        obs = (_p(offs, C.c_int64), _p(uv, C.c_float), _p(xyz, C.c_float))
    opt = capi.Options()
    lib.cc_options_init(C.byref(opt))
    state = (_p(intr if outputs else None, C.c_double), _p(q, C.c_double), _p(t, C.c_double))
    if "estimate" in sym:
        mid = (None, C.c_uint32(0), _p(K, C.c_float)) + state + (None,)
    else:
        mid = (state[0], C.c_uint32(0)) + state[1:] + (None,)
    rc = getattr(lib, sym)(C.byref(opt), C.c_int32(-1), C.c_int64(frames), *obs, *mid, *_tail(lib, sym, C.c_double(huber), model, start, keep))
    return rc, lib.cc_last_error().decode()


def _batch(lib, sym, problems=(3, 4), outputs=True, huber=None, model=0, start=None, short=None, poff=None, foff=None, n_problems=None):
    """One problem per entry of `problems` (its frames, 4 points each; short: (frame, points) for one frame of the batch)."""
    counts = np.full(int(sum(problems)), 4, dtype=np.int64)
    if short is not None:
        counts[short[0]] = short[1]
    po = np.concatenate([[0], np.cumsum(problems)]).astype(np.int64) if poff is None else np.array(poff, dtype=np.int64)
    fo = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64) if foff is None else np.array(foff, dtype=np.int64)
    n, F, B = int(counts.sum()), len(counts), len(problems)
    uv, xyz = np.zeros((n, 2), np.float32), np.zeros((n, 3), np.float32)
    intr, q, t, K = np.zeros((B, 9)), np.zeros((F, 4)), np.zeros((F, 3)), np.zeros((B, 9), np.float32)
    ha = np.array(huber, dtype=np.float64) if huber is not None else None
    opt = capi.Options()
    lib.cc_options_init(C.byref(opt))
    keep = []
    head = (C.byref(opt), C.c_int32(-1), C.c_int64(B if n_problems is None else n_problems), _p(po, C.c_int64), _p(fo, C.c_int64),
            _p(uv, C.c_float), _p(xyz, C.c_float))
    state = (_p(intr if outputs else None, C.c_double), _p(q, C.c_double), _p(t, C.c_double))
    if "estimate" in sym:
        mid = (None, None, _p(K, C.c_float)) + state + (None,)
    else:
        mid = (state[0], None) + state[1:] + (None,)
    rc = getattr(lib, sym)(*head, *mid, *_tail(lib, sym, _p(ha, C.c_double), model, start, keep))
    return rc, lib.cc_last_error().decode()


def run(lib, case):
    _name, kind, sym, kw = case
    lib.cc_last_error.restype = C.c_char_p
    return (_single if kind == "single" else _batch)(lib, sym, **kw)


def cases():
    out = []

    def add(kind, sym, fault, **kw):
        if sym.endswith("_start") and kw.get("start", {}) is not None:
            kw.setdefault("start", {})   # the search at its defaults, on the fisheye model, unless the case says otherwise
            kw.setdefault("model", FISH)
        out.append(("%s:%s" % (sym, fault), kind, sym, kw))

    for sym in SINGLE:
        views, huber, model, est = "_views" in sym, sym.endswith(("_huber", "_model", "_start")), sym.endswith(("_model", "_start")), "estimate" in sym
        add("single", sym, "well_formed")
        add("single", sym, "null_outputs", outputs=False)
        add("single", sym, "too_few_frames", frames=2 if est else 0)
        add("single", sym, "short_view", short=(1, 3))
        add("single", sym, "null_outputs+short_view", outputs=False, short=(1, 3))
        if views:
            add("single", sym, "null_view", null_view=1)
            add("single", sym, "null_xyz_view", null_xyz_view=2)
            add("single", sym, "short_view+null_view", short=(0, 3), null_view=1)
            add("single", sym, "empty_view", short=(2, 0))
        else:
            add("single", sym, "offsets_start_at_1", off=[1, 5, 9, 13])
            add("single", sym, "offsets_decrease", off=[0, 8, 4, 12])
            add("single", sym, "offsets_decrease+too_few_frames", frames=2 if est else 0, off=[0, 8, 4, 12])
        if huber:
            add("single", sym, "nan_huber", huber=NAN)
            add("single", sym, "null_outputs+nan_huber", outputs=False, huber=NAN)
            add("single", sym, "nan_huber+short_view", huber=NAN, short=(1, 3))
        if model:
            add("single", sym, "unknown_model", model=7)
            add("single", sym, "nan_huber+unknown_model", huber=NAN, model=7)
            add("single", sym, "unknown_model+short_view", model=7, short=(1, 3))
            add("single", sym, "fisheye", model=FISH)
            add("single", sym, "fisheye+short_view", model=FISH, short=(1, 3))   # (the device is asked ahead of the views)
            add("single", sym, "fisheye+null_view", model=FISH, null_view=0)
    sym = "cc_intrinsics_estimate_views_start"
    add("single", sym, "null_start+unknown_model", start=None, model=7)
    add("single", sym, "null_start+short_view", start=None, model=0, short=(1, 3))
    add("single", sym, "start_on_radtan", model=0)
    add("single", sym, "candidates_0", start=dict(candidates=0))
    add("single", sym, "start_on_radtan+candidates_0", model=0, start=dict(candidates=0))
    add("single", sym, "nan_huber+candidates_0", huber=NAN, start=dict(candidates=0))
    add("single", sym, "candidates_0+short_view", start=dict(candidates=0), short=(1, 3))
    add("single", sym, "theta_hi_pi", start=dict(theta_hi=float(np.pi)))

    for sym in BATCH:
        huber, model, est = sym.endswith(("_huber", "_model", "_start")), sym.endswith(("_model", "_start")), "estimate" in sym
        add("batch", sym, "well_formed")
        add("batch", sym, "null_outputs", outputs=False)
        add("batch", sym, "too_few_frames", problems=(3, 2))
        add("batch", sym, "short_frame", short=(4, 3))
        add("batch", sym, "too_few_frames+short_frame", problems=(3, 2), short=(1, 3))   # (problem 0's frames come before problem 1's count)
        add("batch", sym, "short_frame+too_few_frames", problems=(2, 3), short=(3, 3))
        add("batch", sym, "no_problems", n_problems=0)
        add("batch", sym, "problem_offsets_start_at_1", poff=[1, 3, 7])
        add("batch", sym, "problem_offsets_decrease", poff=[0, 4, 3])
        add("batch", sym, "empty_problem", poff=[0, 7, 7])
        add("batch", sym, "frame_offsets_start_at_1", foff=[1, 4, 8, 12, 16, 20, 24, 28])
        add("batch", sym, "frame_offsets_decrease", foff=[0, 4, 8, 6, 16, 20, 24, 28])
        add("batch", sym, "null_outputs+problem_offsets_decrease", outputs=False, poff=[0, 4, 3])
        add("batch", sym, "frame_offsets_decrease+too_few_frames", problems=(3, 2), foff=[0, 4, 8, 6, 16, 20])
        if huber:
            add("batch", sym, "nan_huber", huber=[1.0, NAN])
            add("batch", sym, "null_outputs+nan_huber", outputs=False, huber=[NAN, 1.0])
            add("batch", sym, "nan_huber+problem_offsets_decrease", huber=[1.0, NAN], poff=[0, 4, 3])
            add("batch", sym, "nan_huber+too_few_frames", huber=[1.0, NAN], problems=(3, 2))
        if model:
            add("batch", sym, "unknown_model", model=7)
            add("batch", sym, "nan_huber+unknown_model", huber=[NAN, NAN], model=7)   # (the two calls answer this differently)
            add("batch", sym, "unknown_model+too_few_frames", model=7, problems=(3, 2))
            add("batch", sym, "fisheye", model=FISH)
            add("batch", sym, "fisheye+short_frame", model=FISH, short=(4, 3))
    sym = "cc_intrinsics_batch_estimate_start"
    add("batch", sym, "null_start+unknown_model", start=None, model=7)
    add("batch", sym, "null_start+nan_huber+unknown_model", start=None, model=7, huber=[NAN, 1.0])
    add("batch", sym, "null_start+short_frame", start=None, model=0, short=(4, 3))
    add("batch", sym, "start_on_radtan", model=0)
    add("batch", sym, "candidates_0", start=dict(candidates=0))
    add("batch", sym, "start_on_radtan+candidates_0", model=0, start=dict(candidates=0))
    add("batch", sym, "nan_huber+candidates_0", huber=[1.0, NAN], start=dict(candidates=0))
    add("batch", sym, "candidates_0+too_few_frames", start=dict(candidates=0), problems=(3, 2))
    add("batch", sym, "candidates_0+problem_offsets_decrease", start=dict(candidates=0), poff=[0, 4, 3])
    assert len({c[0] for c in out}) == len(out)
    return out
