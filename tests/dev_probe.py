"""ctypes face of the primitive probe (tests/cpp/dev_probe.hip -> tests/cpp/libcc_dev_probe.so, built by
__graft_entry__.build()): one function per probed device helper, numpy in, numpy out. Test infrastructure only."""
import ctypes
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
_up = ctypes.POINTER(ctypes.c_uint)
_qp = ctypes.POINTER(ctypes.c_ulonglong)
_i = ctypes.c_int
_ll = ctypes.c_longlong
_lp = ctypes.POINTER(ctypes.c_longlong)
_fp = ctypes.POINTER(ctypes.c_float)


def lib():
    global _LIB
    if _LIB is None:
        # (CC_DEV_PROBE_LIB: a probe built from a scratch copy of the sources, as CC_LIB_PATH is for the product library)
        path = os.environ.get("CC_DEV_PROBE_LIB", os.path.join(HERE, "cpp", "libcc_dev_probe.so"))
        assert os.path.exists(path), "run __graft_entry__.build() first"
        L = ctypes.CDLL(path)
        for name, args in {
            "probe_lane_reduce": [_i, _dp, _dp],
            "probe_reduce_scatter": [_i, _dp, _dp],
            "probe_block_sum256": [_dp, _dp],
            "probe_gram": [_i, _i, _dp, _dp],
            "probe_scalar": [_i, _i, _dp, _dp],
            "probe_quat_plus": [_i, _i, _dp, _dp, _dp],
            "probe_quat_to_R": [_i, _dp, _dp],
            "probe_pose_grad": [_i, _i, _dp, _dp, _dp],
            "probe_granule": [_i, _up, _qp, _qp, _qp],
            "probe_untri": [_i, _ip],
            "probe_plus_coef": [_dp],
            "probe_spec_radius": [_i, _dp, _dp, _dp],
            "probe_chol_rows": [_i, _i, _dp, _dp, _dp, _ip],
            "probe_chol_block4": [_i, _i, _dp, _dp, _ip],
            "probe_zhang_gram": [_ll, _lp, _fp, _fp, _dp],
            "probe_smallest_eigvec": [_i, _ll, _dp, _dp],
            "probe_zhang_eig9": [_ll, _dp, _fp],
            "probe_zhang_k": [_ll, _fp, _fp],
            "probe_zhang_poses": [_ll, _fp, _fp, _fp, _fp],
            "probe_jacobi_eigen3": [_ll, _dp, _dp, _dp],
        }.items():
            f = getattr(L, name)
            f.argtypes = args
            f.restype = ctypes.c_int
        _LIB = L
    return _LIB


def _d(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        assert a.shape == shape, (a.shape, shape)
    return a


def _p(a, t=_dp):
    return a.ctypes.data_as(t)


def _ok(rc, what):
    if rc > 0:   # a HIP error: the device may be in no state to go on, so nothing more of this session runs on it
        pytest.exit(f"{what}: the probe's HIP calls failed with hipError_t {rc}", returncode=3)
    assert rc == 0, f"{what}: the probe refused its arguments"


LANE_REDUCTIONS = {"wave_sum_mod0": 0, "wave_sum_mod1": 1, "wave_sum_mod2": 2, "wave_sum_mod3": 3, "row16_sum": 4,
                   "row16_max": 5, "row_pair_sum": 6, "half_pair_sum": 7}


def lane_reduce(name, v):
    v, out = _d(v, (64,)), np.empty(64)
    _ok(lib().probe_lane_reduce(LANE_REDUCTIONS[name], _p(v), _p(out)), name)
    return out


def reduce_scatter(v):
    """v[lane][e], e < 32 or 64 -> p[0] of every lane after reduce_scatter32 / reduce_scatter64."""
    v = _d(v)
    assert v.shape in ((64, 32), (64, 64))
    out = np.empty(64)
    _ok(lib().probe_reduce_scatter(v.shape[1], _p(v), _p(out)), "reduce_scatter")
    return out


def block_sum256(v):
    v, out = _d(v, (256,)), np.empty(256)
    _ok(lib().probe_block_sum256(_p(v), _p(out)), "block_sum256")
    return out


GRAM_FORMS = {"gram_rows": 0, "gram_operands+gram_products": 1, "gram_rows_ahead": 2}


def gram_parts(form, rows):
    """rows[64 * passes][16] -> (block, acc0, acc1): the 16 x 16 block R^T R accumulated over the passes and the two
    accumulators it is the sum of, each in the block's layout."""
    rows = _d(rows)
    assert rows.ndim == 2 and rows.shape[1] == 16 and rows.shape[0] % 64 == 0
    out = np.empty((3, 16, 16))
    _ok(lib().probe_gram(GRAM_FORMS[form], rows.shape[0] // 64, _p(rows), _p(out)), form)
    return out[0], out[1], out[2]


def gram(form, rows):
    return gram_parts(form, rows)[0]


def plus_coef():
    out = np.empty(16)
    _ok(lib().probe_plus_coef(_p(out)), "kPlusCoef")
    return out


def _scalar(which, v):
    v = _d(v).ravel()
    out = np.empty_like(v)
    _ok(lib().probe_scalar(which, v.size, _p(v), _p(out)), "scalar map")
    return out


def rsqrt_pos(v):
    return _scalar(0, v)


def recip_depth(v):
    return _scalar(1, v)


def quat_plus(x, d, tab=False):
    x, d = _d(x), _d(d)
    n = x.shape[0]
    assert x.shape == (n, 4) and d.shape == (n, 3)
    out = np.empty((n, 4))
    _ok(lib().probe_quat_plus(int(tab), n, _p(x), _p(d), _p(out)), "quat_plus")
    return out


def quat_to_R(q):
    q = _d(q)
    n = q.shape[0]
    assert q.shape == (n, 4)
    out = np.empty((n, 3, 3))
    _ok(lib().probe_quat_to_R(n, _p(q), _p(out)), "quat_to_R")
    return out


def pose_grad_proj_max(q, g, tab=False):
    q, g = _d(q), _d(g)
    n = q.shape[0]
    assert q.shape == (n, 4) and g.shape == (n, 6)
    out = np.empty(n)
    _ok(lib().probe_pose_grad(int(tab), n, _p(q), _p(g), _p(out)), "pose_grad_proj_max")
    return out


def granule_round_trip(tags, bits):
    """-> (words[n][2]: the low / high granule of each value, back[n]: the bits ungranule returns)."""
    tags = np.ascontiguousarray(tags, dtype=np.uint32)
    bits = np.ascontiguousarray(bits, dtype=np.uint64)
    n = bits.size
    assert tags.shape == (n,) and bits.shape == (n,)
    words, back = np.empty((n, 2), dtype=np.uint64), np.empty(n, dtype=np.uint64)
    _ok(lib().probe_granule(n, _p(tags, _up), _p(bits, _qp), _p(words, _qp), _p(back, _qp)), "granule")
    return words, back


def untri(n):
    ij = np.empty((n, 2), dtype=np.int32)
    _ok(lib().probe_untri(n, _p(ij, _ip)), "untri")
    return ij


def spec_radius(radius, max_radius):
    """-> out[n][2]: persist_spec_radius, and the radius lm_apply leaves after an accepted step of quality 1."""
    radius, max_radius = _d(radius), _d(max_radius)
    n = radius.size
    assert radius.shape == (n,) and max_radius.shape == (n,)
    out = np.empty((n, 2))
    _ok(lib().probe_spec_radius(n, _p(radius), _p(max_radius), _p(out)), "persist_spec_radius")
    return out


def chol_solve_rows(a, b):
    """a[nsys][64][S] (what every lane holds, all of it), b[nsys][64] -> x[nsys][64][S], ok[nsys][64]."""
    a, b = _d(a), _d(b)
    nsys, S = a.shape[0], a.shape[2]
    assert a.shape == (nsys, 64, S) and b.shape == (nsys, 64)
    x, ok = np.empty((nsys, 64, S)), np.empty((nsys, 64), dtype=np.int32)
    _ok(lib().probe_chol_rows(S, nsys, _p(a), _p(b), _p(x), _p(ok, _ip)), "chol_solve_rows")
    return x, ok


def chol_block4(M):
    """M[nsys][S + 1][S + 1]: the LDS image, row S the right-hand side -> x[nsys][S], ok[nsys][256]."""
    M = _d(M)
    nsys, S = M.shape[0], M.shape[1] - 1
    assert M.shape == (nsys, S + 1, S + 1)
    x, ok = np.empty((nsys, 64)), np.empty((nsys, 256), dtype=np.int32)
    _ok(lib().probe_chol_block4(S, nsys, _p(M), _p(x), _p(ok, _ip)), "chol_block4")
    return x[:, :S].copy(), ok


# ---- Zhang initialisation (cc_zhang_dev.hpp)
def _f(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None:
        assert a.shape == shape, (a.shape, shape)
    return a


def zhang_gram(off, uv, xyz):
    """k_zhang_gram: off[F + 1], uv[N][2], xyz[N][3] (float32) -> gram[F][16][16]."""
    off = np.ascontiguousarray(off, dtype=np.int64)
    F, N = len(off) - 1, int(off[-1])
    uv, xyz = _f(uv, (N, 2)), _f(xyz, (N, 3))
    out = np.empty((F, 16, 16))
    _ok(lib().probe_zhang_gram(F, _p(off, _lp), _p(uv, _fp), _p(xyz, _fp), _p(out)), "k_zhang_gram")
    return out


def smallest_eigvec(A):
    """smallest_eigvec<N>, N = 6 or 9: A[count][N][N] -> x[count][N] (doubles, before any rounding to float)."""
    A = _d(A)
    count, N = A.shape[0], A.shape[1]
    assert A.shape == (count, N, N)
    out = np.empty((count, N))
    _ok(lib().probe_smallest_eigvec(N, count, _p(A), _p(out)), "smallest_eigvec")
    return out


def zhang_eig9(gram):
    """k_zhang_eig9: gram[F][16][16] -> H[F][3][3] float32."""
    gram = _d(gram)
    F = gram.shape[0]
    assert gram.shape == (F, 16, 16)
    out = np.empty((F, 3, 3), dtype=np.float32)
    _ok(lib().probe_zhang_eig9(F, _p(gram), _p(out, _fp)), "k_zhang_eig9")
    return out


def zhang_k(Hs):
    """k_zhang_k: Hs[F][3][3] float32 -> K[3][3] float32."""
    Hs = _f(Hs)
    F = Hs.shape[0]
    assert Hs.shape == (F, 3, 3)
    out = np.empty((3, 3), dtype=np.float32)
    _ok(lib().probe_zhang_k(F, _p(Hs, _fp), _p(out, _fp)), "k_zhang_k")
    return out


def zhang_poses(Hs, K):
    """k_zhang_poses: Hs[F][3][3], K[3][3] float32 -> q[F][4] (w x y z), t[F][3] float32."""
    Hs, K = _f(Hs), _f(K, (3, 3))
    F = Hs.shape[0]
    assert Hs.shape == (F, 3, 3)
    q, t = np.empty((F, 4), dtype=np.float32), np.empty((F, 3), dtype=np.float32)
    _ok(lib().probe_zhang_poses(F, _p(Hs, _fp), _p(K, _fp), _p(q, _fp), _p(t, _fp)), "k_zhang_poses")
    return q, t


def jacobi_eigen3(S):
    """jacobi_eigen<3>(S, V, 10): S[count][3][3] -> (eigenvalues[count][3], V[count][3][3], eigenvectors in columns)."""
    S = _d(S)
    count = S.shape[0]
    assert S.shape == (count, 3, 3)
    lam, V = np.empty((count, 3)), np.empty((count, 3, 3))
    _ok(lib().probe_jacobi_eigen3(count, _p(S), _p(lam), _p(V)), "jacobi_eigen<3>")
    return lam, V
