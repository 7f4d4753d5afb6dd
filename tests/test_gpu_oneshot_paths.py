"""GPU: every one-shot intrinsics call returns, byte for byte, what the handle-level sequence it stands for returns -- create, the
start at handle level (the caller's state, cc_zhang_init rounded to float, or cc_intrinsics_estimate_start_fisheye), set_state,
solve with use_graph = 0, get_state: intrinsics, poses, costs, iteration counts and the whole iteration log. Packed and views
input; plain, Huber, fisheye, fisheye with the focal search; the batch at B = 2 with problems of different frame counts. Scenes:
4 (and 5) views of 12 points, a 3 x 4 board; three views of 20 000 points, whose upload goes in more than one piece; a view of 0
points. The five cc_last_call_timing slots are checked after every single-handle call."""
import ctypes as C
import functools

import numpy as np
import pytest

from camera_calibrator_amd import capi
from oracle import pyoracle as po
from tests import fisheye_ref as fr

pytestmark = pytest.mark.gpu
FISH, RADTAN = capi.MODEL_FISHEYE, capi.MODEL_RADTAN
HUBER_A = 1.5
D5 = np.array([1e-3, -1e-4, 1e-5, -1e-5, 1e-6])   # where an estimate's distortion starts (fisheye: the first four)


def _options():
    return capi.default_options(use_graph=0, max_iterations=12)


@functools.lru_cache(maxsize=None)
def _scene(views=4, seed=11):
    """`views` views of a 3 x 4 board through the fisheye lens of tests/fisheye_ref.py, with its Zhang start."""
    return fr.make_case([12] * views, 0.30, 0.45, 0.35, 0.3, seed=seed)


@functools.lru_cache(maxsize=None)
def _big_scene():
    off, uv, xyz = po.make_intrinsics_problem(3, 20000)
    assert int(off[-1]) == 60000   # more than one 32768-observation piece
    return dict(off=off, uv=uv, xyz=xyz)


def _timing():
    tm = (C.c_double * 5)()
    capi.lib().cc_last_call_timing(tm)
    return list(tm)


def _answer(intr, q, t, s):
    """What must agree: the state's bytes, the costs' bytes, the counts and the log."""
    return (np.ascontiguousarray(intr, dtype=np.float64).tobytes(), np.ascontiguousarray(q, dtype=np.float64).tobytes(),
            np.ascontiguousarray(t, dtype=np.float64).tobytes(), np.array([s["initial_cost"], s["final_cost"]]).tobytes(),
            s["iterations"], s["successful_steps"], s["termination"], s["sweeps"], str(s["log"]))


def _k_of(k):
    """The focal search's pick f f cx cy as a (float64) K."""
    return np.array([[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1]])


def _start_intr(K, model, d5):
    intr = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2], 0, 0, 0, 0, 0], dtype=np.float64)
    if d5 is not None:
        n = 4 if model == FISH else 5
        intr[4:4 + n] = d5[:n]
    return intr


def _by_handle(c, start, huber_a=0.0, model=RADTAN, d5=None, state=None):
    """start: "caller" (state = (intr, q, t)), "zhang" or "fisheye". Returns (K of the start or None, answer)."""
    p = capi.IntrinsicsProblem(c["off"], c["uv"], c["xyz"])
    try:
        if huber_a > 0:
            p.set_huber(huber_a)
        if model != RADTAN:
            p.set_model(model)
        K = None
        if start == "caller":
            intr0, q0, t0 = state
        elif start == "zhang":
            K, qf, tf = capi.zhang_init(c["off"], c["uv"], c["xyz"])
            intr0, q0, t0 = _start_intr(K, model, d5), qf.astype(np.float64), tf.astype(np.float64)
        else:
            k, q0, t0, _ = p.estimate_start_fisheye()
            K = _k_of(k)
            intr0 = _start_intr(K, model, d5)
        p.set_state(intr0, q0, t0)
        s = p.solve(_options())
        return K, _answer(*p.get_state(), s)
    finally:
        p.close()


def _check_timing(estimate):
    tm = _timing()
    assert all(tm[i] > 0 for i in (0, 1, 3, 4)), tm
    assert (tm[2] > 0) if estimate else (tm[2] == 0), tm


# ---- the single handle ----------------------------------------------------------------------------------------------------------
OPTIMIZE = [("packed", dict()), ("views", dict(views=True)), ("views_huber", dict(huber_a=HUBER_A)), ("views_fisheye", dict(model=FISH)),
            ("views_fisheye_huber", dict(model=FISH, huber_a=HUBER_A))]


@pytest.mark.parametrize("name,kw", OPTIMIZE, ids=[n for n, _ in OPTIMIZE])
def test_optimize_is_the_handle_sequence(name, kw):
    c = _scene()
    state = (c["intr0"], c["q0"], c["t0"])
    intr, q, t, s = capi.intrinsics_optimize(c["off"], c["uv"], c["xyz"], *state, options=_options(), **kw)
    _check_timing(estimate=False)
    _, want = _by_handle(c, "caller", huber_a=kw.get("huber_a", 0.0), model=kw.get("model", RADTAN), state=state)
    assert _answer(intr, q, t, s) == want


ESTIMATE = [("packed", dict()), ("views", dict(views=True)), ("views_huber", dict(huber_a=HUBER_A)), ("views_fisheye", dict(model=FISH)),
            ("views_fisheye_huber", dict(model=FISH, huber_a=HUBER_A)), ("views_fisheye_search", dict(model=FISH, start="fisheye")),
            ("views_fisheye_search_huber", dict(model=FISH, start="fisheye", huber_a=HUBER_A))]


@pytest.mark.parametrize("name,kw", ESTIMATE, ids=[n for n, _ in ESTIMATE])
def test_estimate_is_the_handle_sequence(name, kw):
    c = _scene()
    K, intr, q, t, s = capi.intrinsics_estimate(c["off"], c["uv"], c["xyz"], distortion5=D5, options=_options(), **kw)
    _check_timing(estimate=True)
    K_want, want = _by_handle(c, kw.get("start", "zhang"), huber_a=kw.get("huber_a", 0.0), model=kw.get("model", RADTAN), d5=D5)
    assert K.tobytes() == np.ascontiguousarray(K_want, dtype=np.float32).tobytes()
    assert _answer(intr, q, t, s) == want


def test_views_uploaded_in_more_than_one_piece():
    """Three views of 20 000 points: the pieces are [views 0, 1] and [view 2]."""
    c = _big_scene()
    K, intr, q, t, s = capi.intrinsics_estimate(c["off"], c["uv"], c["xyz"], views=True, options=_options())
    _check_timing(estimate=True)
    K_want, want = _by_handle(c, "zhang")
    assert K.tobytes() == K_want.tobytes() and _answer(intr, q, t, s) == want
    state = (intr, q, t)   # (and from there on: the caller's state over the same upload)
    got = capi.intrinsics_optimize(c["off"], c["uv"], c["xyz"], *state, views=True, options=_options())
    _check_timing(estimate=False)
    assert _answer(*got) == _by_handle(c, "caller", state=state)[1]


def test_optimize_views_with_a_view_of_no_points():
    c = _scene()
    off = np.concatenate([c["off"][:2], c["off"][1:]])   # view 1 is empty
    q0 = np.insert(c["q0"], 1, [1.0, 0.0, 0.0, 0.0], axis=0)
    t0 = np.insert(c["t0"], 1, [0.0, 0.0, 1.0], axis=0)
    e = dict(off=off, uv=c["uv"], xyz=c["xyz"])
    state = (c["intr0"], q0, t0)
    got = capi.intrinsics_optimize(off, c["uv"], c["xyz"], *state, views=True, options=_options())
    _check_timing(estimate=False)
    assert _answer(*got) == _by_handle(e, "caller", state=state)[1]


# ---- the batch ------------------------------------------------------------------------------------------------------------------
def _batch_scenes():
    return [_scene(4, 11), _scene(5, 12)]   # B = 2, four and five views


def _problems(cs):
    return [(c["off"], c["uv"], c["xyz"]) for c in cs]


def _batch_answer(intr, qs, ts, ss):
    return [_answer(intr[p], qs[p], ts[p], ss[p]) for p in range(len(ss))]


def _batch_by_handle(cs, start, huber=None, model=RADTAN, d5=None, state=None):
    """_by_handle for a batch: d5 one row per problem, huber one threshold per problem. Returns ([K_p] or None, [answer_p])."""
    h = capi.IntrinsicsBatch(_problems(cs))
    try:
        if model != RADTAN:
            h.set_model(model)
        Ks = None
        if start == "caller":
            intr0, q0, t0 = state
        else:
            if start == "zhang":
                z = [capi.zhang_init(*p) for p in _problems(cs)]
                Ks = [K for K, _, _ in z]
                q0, t0 = [qf.astype(np.float64) for _, qf, _ in z], [tf.astype(np.float64) for _, _, tf in z]
            else:
                ks, q0, t0, _ = h.estimate_start_fisheye()
                Ks = [_k_of(k) for k in ks]
            intr0 = np.stack([_start_intr(K, model, d5[p]) for p, K in enumerate(Ks)])
        h.set_state(intr0, q0, t0)
        if huber is not None:
            h.set_huber(huber)
        ss = h.solve(_options())
        return Ks, _batch_answer(*h.get_state(), ss)
    finally:
        h.close()


def test_batch_optimize_is_the_handle_sequence():
    cs = _batch_scenes()
    state = (np.stack([c["intr0"] for c in cs]), [c["q0"] for c in cs], [c["t0"] for c in cs])
    got = capi.intrinsics_batch_optimize(_problems(cs), *state, options=_options())
    assert _batch_answer(*got) == _batch_by_handle(cs, "caller", state=state)[1]


BATCH_ESTIMATE = [("plain", dict()), ("huber", dict(huber_a=[HUBER_A, 0.0])), ("fisheye", dict(model=FISH)),
                  ("fisheye_huber", dict(model=FISH, huber_a=[0.0, HUBER_A])), ("fisheye_search", dict(model=FISH, start="fisheye")),
                  ("fisheye_search_huber", dict(model=FISH, start="fisheye", huber_a=[HUBER_A, HUBER_A]))]


@pytest.mark.parametrize("name,kw", BATCH_ESTIMATE, ids=[n for n, _ in BATCH_ESTIMATE])
def test_batch_estimate_is_the_handle_sequence(name, kw):
    cs = _batch_scenes()
    d5 = np.stack([D5, 2 * D5])
    K, intr, qs, ts, ss = capi.intrinsics_batch_estimate(_problems(cs), distortion5=d5, options=_options(), **kw)
    Ks, want = _batch_by_handle(cs, kw.get("start", "zhang"), huber=kw.get("huber_a"), model=kw.get("model", RADTAN), d5=d5)
    assert K.tobytes() == np.stack(Ks).astype(np.float32).tobytes()
    assert _batch_answer(intr, qs, ts, ss) == want
