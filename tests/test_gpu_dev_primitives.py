"""The shared device primitives (cc_common.hpp, cc_device.hpp, cc_persist_dev.hpp, cc_rig_dev.hpp), each on its own through
the probe library (tests/cpp/dev_probe.hip, tests/dev_probe.py), against references that are neither the oracle nor the
code under test: mpmath at 50 digits, or Python integers where the result is exact. u = 2^-53 throughout.

Every bound below is stated before anything was run and comes from the arithmetic, not from the results; each test prints
its largest measured error as a fraction of the bound (`pytest -s`).

Measured on an MI355X (largest error / bound):

    0.036   63 u Σ|v|                                  lane sums of doubles (wave_sum_mod<0..3>, row16_sum, row_pair_sum, half_pair_sum, reduce_scatter32/64)
    0.001   255 u Σ|v|                                 block_sum256
    0.053   64 u Σ|a||b| per entry                     Gram entry, one pass of 64 rows (pairs cancelling to 1e-9 included)
    0.025   192 u Σ|a||b| per entry                    Gram entry, three passes
    0.375   4 u relative                               rsqrt_pos, all finite d > 0 (worst at 1 − ulp)
    0.250   4 u relative                               recip_depth, 2^-500 ≤ |z| ≤ 2^500 (worst at 1 − ulp)
    0.328   8 u Σ|a_i||x_i|                            quat_plus, series branch
    0.235   8 u Σ|a_i||x_i|                            quat_plus, libm branch (|d| ≥ 1/4 along one axis)
    0.500   16 u                                       quat_to_R entries
    0.466   32 u                                       quat_to_R orthogonality
    0.261   8 u Σ|terms| of the winning component      pose_grad_proj_max, |g_rot| < 1/4
    0.132   (3 S + 9) u |L||Lᵀ||x̂|                    chol_solve_rows<S>, S = 6, 9, 12, 18, 24 (worst: S = 6)
    0.135   (3 S + 9) u |L||Lᵀ||x̂|                    chol_block4 + chol_backward<false>, S = 1 … 63 (worst: S = 9)

The libm branch of quat_plus (OCML's 2 ulp for sin / cos) stays a factor 4 below its bound, quat_to_R a factor 2.
"""
import math
import struct

import numpy as np
import pytest
from mpmath import mp, mpf

from tests import dev_probe as dp

pytestmark = pytest.mark.gpu

mp.dps = 50
U = 2.0 ** -53
DBL_MAX = float(np.finfo(np.float64).max)
DBL_MIN = float(np.finfo(np.float64).tiny)
SUB_MIN = 5e-324


def _report(what, ratio):
    print(f"[dev-primitives] {what}: max measured / bound = {float(ratio):.3f}")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _mixed(rng, shape):
    """Doubles of mixed sign, magnitude 1e-8 .. 1e8."""
    return rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-8, 8, size=shape)


# ---------------------------------------------------------------------------------------------------------------------
# lane reductions
# ---------------------------------------------------------------------------------------------------------------------
def _lanes_of(name, l):
    """The lanes whose values the contract says lane l's result is made of."""
    if name.startswith("wave_sum_mod"):
        mask = (1 << int(name[-1])) - 1
        return [m for m in range(64) if (m & mask) == (l & mask)]
    if name.startswith("row16"):
        return [m for m in range(64) if m >> 4 == l >> 4]
    return sorted({l, l ^ (16 if name == "row_pair_sum" else 32)})


LANE_SUMS = ["wave_sum_mod0", "wave_sum_mod1", "wave_sum_mod2", "wave_sum_mod3", "row16_sum", "row_pair_sum", "half_pair_sum"]


@pytest.mark.parametrize("name", LANE_SUMS + ["row16_max"])
def test_lane_reductions_exact_on_integers_in_every_lane(name):
    rng = np.random.default_rng(11)
    for _ in range(4):
        v = rng.integers(0, 2 ** 20, size=64)
        got = dp.lane_reduce(name, v.astype(np.float64))
        red = max if name == "row16_max" else sum
        want = [red(int(v[m]) for m in _lanes_of(name, l)) for l in range(64)]
        assert [int(g) for g in got] == want and np.all(got == np.floor(got))


@pytest.mark.parametrize("width", [32, 64])
def test_reduce_scatter_exact_on_integers_value_e_where_the_contract_puts_it(width):
    """reduce_scatter32: value e in lanes 2e and 2e + 1; reduce_scatter64: value e in lane e."""
    rng = np.random.default_rng(12)
    for _ in range(3):
        v = rng.integers(0, 2 ** 20, size=(64, width))
        got = dp.reduce_scatter(v.astype(np.float64))
        col = [sum(int(x) for x in v[:, e]) for e in range(width)]
        want = [col[l // 2] if width == 32 else col[l] for l in range(64)]
        assert [int(g) for g in got] == want


def test_block_sum256_exact_on_integers_in_all_256_threads():
    rng = np.random.default_rng(13)
    v = rng.integers(0, 2 ** 20, size=256)
    got = dp.block_sum256(v.astype(np.float64))
    assert [int(g) for g in got] == [sum(int(x) for x in v)] * 256


def test_lane_sums_of_doubles_within_the_bound_of_any_summation_order():
    """|got - exact| <= (n - 1) u sum|v| holds for every order of n - 1 additions (Higham, Accuracy and Stability, 4.2, to
    first order); asserted with the issue's constants 63 u (one wave) and 255 u (block_sum256) whatever the group's size."""
    rng = np.random.default_rng(14)
    worst = 0.0
    for name in LANE_SUMS:
        v = _mixed(rng, 64)
        got = dp.lane_reduce(name, v)
        for l in range(64):
            grp = [float(v[m]) for m in _lanes_of(name, l)]
            err = abs(mpf(float(got[l])) - sum(mpf(x) for x in grp))
            bound = 63 * U * math.fsum(abs(x) for x in grp)
            worst = max(worst, float(err / bound))
            assert err <= bound, (name, l, float(err), bound)
    for width in (32, 64):
        v = _mixed(rng, (64, width))
        got = dp.reduce_scatter(v)
        for l in range(64):
            grp = [float(x) for x in v[:, l // 2 if width == 32 else l]]
            err = abs(mpf(float(got[l])) - sum(mpf(x) for x in grp))
            bound = 63 * U * math.fsum(abs(x) for x in grp)
            worst = max(worst, float(err / bound))
            assert err <= bound, (width, l, float(err), bound)
    _report("lane sums of doubles (63 u sum|v|)", worst)
    v = _mixed(rng, 256)
    got = dp.block_sum256(v)
    exact = sum(mpf(float(x)) for x in v)
    bound = 255 * U * math.fsum(abs(float(x)) for x in v)
    errs = [abs(mpf(float(g)) - exact) for g in got]
    assert max(errs) <= bound
    assert len(set(_bits(got).tolist())) == 1   # one value for the whole block
    _report("block_sum256 of doubles (255 u sum|v|)", max(errs) / bound)


def test_row16_max_on_negative_rows_and_on_a_row_with_one_nan():
    """fmax semantics (recorded in cc_device.hpp): the maximum of all-negative values is the largest of them, not 0; a NaN
    is a missing value -- the row's other fifteen lanes decide, in the NaN's own lane too."""
    rng = np.random.default_rng(15)
    v = -(10.0 ** rng.uniform(-8, 8, size=64))
    got = dp.lane_reduce("row16_max", v)
    for l in range(64):
        assert got[l] == max(v[m] for m in _lanes_of("row16_max", l))
    w = _mixed(rng, 64)
    for nan_lane in (0, 21, 47, 63):
        x = w.copy()
        x[nan_lane] = np.nan
        got = dp.lane_reduce("row16_max", x)
        for l in range(64):
            assert got[l] == max(x[m] for m in _lanes_of("row16_max", l) if m != nan_lane), (nan_lane, l)


# ---------------------------------------------------------------------------------------------------------------------
# Gram contraction: stage_row + gram_rows / gram_operands + gram_products / gram_rows_ahead
# ---------------------------------------------------------------------------------------------------------------------
CANCEL_PAIRS = [(0, 1), (2, 9), (5, 15), (12, 13)]


def _cancelling_rows(rng, passes):
    """Random rows (magnitudes 1e-2 .. 1e2 per row) in which the column pairs CANCEL_PAIRS nearly cancel: the rows come in
    partners (k, k') that hold the same column i, and column j is +column i in row k and -column i in row k', each plus
    1e-9 |column i| of noise -- so entry (i, j) of R^T R is ~1e-9 of sum_k |r_ki| |r_kj|, against which the bound is set.
    (Column j = -column i in EVERY row would make the entry -|column i|^2, with nothing cancelling.)"""
    n = 64 * passes
    R = rng.standard_normal((n, 16)) * 10.0 ** rng.uniform(-2, 2, size=(n, 1))
    perm = rng.permutation(n)
    a, b = perm[: n // 2], perm[n // 2:]
    for i, j in CANCEL_PAIRS:
        R[b, i] = R[a, i]
        R[a, j] = R[a, i] * (1.0 + 1e-9 * rng.standard_normal(n // 2))
        R[b, j] = -R[b, i] * (1.0 + 1e-9 * rng.standard_normal(n // 2))
    return R


def _gram_reference(R):
    """(exact R^T R, sum_k |r_ki| |r_kj|) in mpmath."""
    cols = [[mpf(float(x)) for x in R[:, c]] for c in range(16)]
    ref = [[mp.fdot(cols[i], cols[j]) for j in range(16)] for i in range(16)]
    mag = [[mp.fdot([abs(x) for x in cols[i]], [abs(x) for x in cols[j]]) for j in range(16)] for i in range(16)]
    return ref, mag


@pytest.fixture(scope="module")
def gram_case():
    rng = np.random.default_rng(21)
    R1, R3 = _cancelling_rows(rng, 1), _cancelling_rows(rng, 3)
    return {"R1": R1, "ref1": _gram_reference(R1), "R3": R3, "ref3": _gram_reference(R3)}


def _gram_ratio(got, ref_mag, terms):
    ref, mag = ref_mag
    worst = 0.0
    for i in range(16):
        for j in range(16):
            err, bound = abs(mpf(float(got[i, j])) - ref[i][j]), terms * U * mag[i][j]
            assert err <= bound, (i, j, float(got[i, j]), float(ref[i][j]), float(err), float(bound))
            worst = max(worst, float(err / bound))
    return worst


@pytest.mark.parametrize("form", list(dp.GRAM_FORMS))
def test_gram_of_small_integers_is_the_integer_product_in_all_256_entries(form):
    """Pins the swizzle of stage_row, the row-to-MFMA assignment and the output map exactly: |v| <= 2^10, 64 or 128 rows,
    every partial sum below 2^27."""
    rng = np.random.default_rng(22)
    for passes in (1, 2):
        R = rng.integers(-1024, 1025, size=(64 * passes, 16))
        got = dp.gram(form, R.astype(np.float64))
        assert np.array_equal(got, (R.T.astype(np.int64) @ R.astype(np.int64)).astype(np.float64))
    # one row, one nonzero pair of components at a time: an entry that lands anywhere else shows up as itself
    for row, (ci, cj) in [(0, (0, 15)), (37, (3, 4)), (63, (15, 8))]:
        R = np.zeros((64, 16))
        R[row, ci], R[row, cj] = 3.0, 5.0
        want = np.zeros((16, 16))
        want[ci, ci], want[cj, cj], want[ci, cj], want[cj, ci] = 9.0, 25.0, 15.0, 15.0
        assert np.array_equal(dp.gram(form, R), want)


def test_gram_entries_are_rounded_entry_by_entry_not_relative_to_the_block(gram_case):
    """|got - exact| <= 64 u sum_k |r_ki| |r_kj| for EVERY entry (the bound of a 64-term dot product in any order, fused or
    not), including the pairs that cancel to 1e-9 of that sum."""
    ref, mag = gram_case["ref1"]
    for i, j in CANCEL_PAIRS:
        assert abs(ref[i][j]) < 1e-7 * mag[i][j]   # (the construction does what it says)
    got = dp.gram("gram_rows", gram_case["R1"])
    _report("Gram entries, one pass (64 u sum|a||b|)", _gram_ratio(got, gram_case["ref1"], 64))


def test_gram_accumulates_three_passes_into_the_same_accumulators(gram_case):
    got = dp.gram("gram_rows", gram_case["R3"])
    _report("Gram entries, three passes (192 u sum|a||b|)", _gram_ratio(got, gram_case["ref3"], 192))


def test_gram_schedules_give_the_same_bits(gram_case):
    """cc_device.hpp: "same operands, same order, same accumulators"."""
    for key in ("R1", "R3"):
        a, b, c = (dp.gram_parts(f, gram_case[key]) for f in dp.GRAM_FORMS)
        for part in range(3):   # the block, and each of the two accumulators on its own (their sum alone cannot tell them apart)
            assert _same_bits(a[part], b[part]) and _same_bits(a[part], c[part]), part


@pytest.mark.parametrize("form", list(dp.GRAM_FORMS))
def test_gram_one_nan_poisons_its_row_and_column_and_nothing_else(gram_case, form):
    clean = dp.gram(form, gram_case["R1"])
    for row, c in [(0, 0), (5, 9), (38, 15), (63, 6)]:
        R = gram_case["R1"].copy()
        R[row, c] = np.nan
        got = dp.gram(form, R)
        want_nan = np.zeros((16, 16), dtype=bool)
        want_nan[c, :] = True
        want_nan[:, c] = True
        assert np.array_equal(np.isnan(got), want_nan), (row, c)
        assert np.array_equal(_bits(got)[~want_nan], _bits(clean)[~want_nan])


# ---------------------------------------------------------------------------------------------------------------------
# rsqrt_pos, recip_depth
# ---------------------------------------------------------------------------------------------------------------------
def _positive_inputs():
    rng = np.random.default_rng(31)
    logu = np.ldexp(rng.uniform(1.0, 2.0, size=4096), rng.integers(-1074, 1024, size=4096))
    logu = logu[(logu > 0) & np.isfinite(logu)]
    edges = [SUB_MIN, DBL_MIN, np.nextafter(DBL_MIN, 0.0), np.nextafter(DBL_MIN, 1.0), 1.0, np.nextafter(1.0, 0.0),
             np.nextafter(1.0, 2.0), DBL_MAX] + [math.ldexp(1.0, 2 * k) for k in range(-537, 512)]
    return np.concatenate([logu, np.array(edges, dtype=np.float64)])


def test_rsqrt_pos_within_four_u_of_the_root_over_the_whole_positive_range():
    """Relative error <= 4 u for every finite d > 0, subnormals included: one rounding in e, one in the final FMA, a cubic
    term below u for any estimate better than 2^-17 (a double emulation of the three operations without FMA: 1.65 u)."""
    d = _positive_inputs()
    assert d.min() == SUB_MIN and d.max() == DBL_MAX and d.size > 5000
    got = dp.rsqrt_pos(d)
    worst, at = mpf(0), None
    for x, g in zip(d.tolist(), got.tolist()):
        ref = 1 / mp.sqrt(mpf(x))
        rel = abs(mpf(g) - ref) / ref if math.isfinite(g) else mp.inf
        if rel > worst:
            worst, at = rel, x
    _report(f"rsqrt_pos (4 u relative; worst at d = {at!r})", worst / (4 * U))
    assert worst <= 4 * U, (at, float(worst / U))


def test_recip_depth_within_four_u_away_from_the_ends_of_the_exponent_range():
    """"Within an ulp or two of 1 / z" (cc_rig_dev.hpp) for 2^-500 <= |z| <= 2^500, both signs: <= 4 u relative."""
    d = _positive_inputs()
    d = d[(d >= 2.0 ** -500) & (d <= 2.0 ** 500)]
    assert d.size > 1500
    z = np.concatenate([d, -d])
    got = dp.recip_depth(z)
    worst, at = mpf(0), None
    for x, g in zip(z.tolist(), got.tolist()):
        ref = 1 / mpf(x)
        rel = abs((mpf(g) - ref) / ref) if math.isfinite(g) else mp.inf
        if rel > worst:
            worst, at = rel, x
    _report(f"recip_depth (4 u relative; worst at z = {at!r})", worst / (4 * U))
    assert worst <= 4 * U, (at, float(worst / U))


def test_recip_depth_of_a_degenerate_depth_is_not_finite():
    got = dp.recip_depth(np.array([0.0, -0.0, np.inf, -np.inf]))
    assert not np.isfinite(got).any(), got


# ---------------------------------------------------------------------------------------------------------------------
# quat_plus, quat_plus_tab, quat_to_R
# ---------------------------------------------------------------------------------------------------------------------
def _quaternions(rng, n):
    """Half unit (to rounding), half of norm 1e-3 .. 1e3."""
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[n // 2:] *= 10.0 ** rng.uniform(-3, 3, size=(n - n // 2, 1))
    return q


def _axis_steps(mag):
    return [tuple((s * mag if k == a else 0.0) for k in range(3)) for a in range(3) for s in (1.0, -1.0)]


def _plus_steps(rng):
    """(d, branch) pairs. Below |d| = 1/4 (the series, whose argument n^2 carries its rounding into cos and sin n / n damped
    by n^2) random directions and the axes; from 1/4 up only steps along one axis, whose norm sqrt(d * d) is exactly |d| in
    binary floating point: the conditioning of sin / cos to a rounded |d| is |d| u -- 1e-10 at |d| = 1e6 -- and is a
    property of the question asked, not of the routine that answers it."""
    steps = [((0.0, 0.0, 0.0), "unchanged")]
    for mag in (1e-170, 1e-8, 1e-3, 0.1):
        branch = "unchanged" if mag == 1e-170 else "series"
        steps += [(d, branch) for d in _axis_steps(mag)]
        for _ in range(4):
            v = rng.standard_normal(3)
            steps.append((tuple((mag * v / np.linalg.norm(v)).tolist()), branch))
    steps += [(d, "series") for d in _axis_steps(float(np.nextafter(0.25, 0.0)))]
    for mag in (0.25, float(np.nextafter(0.25, 1.0)), 1.0, math.pi, 10.0, 1e6):
        steps += [(d, "libm") for d in _axis_steps(mag)]
    return steps


def _plus_mp(x, d):
    """ceres::QuaternionManifold::Plus in mpmath -> per component (value, sum of the absolute values of its four terms)."""
    x, d = [mpf(float(v)) for v in x], [mpf(float(v)) for v in d]
    n = mp.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    s = mp.sin(n) / n if n != 0 else mpf(1)
    a = [mp.cos(n), s * d[0], s * d[1], s * d[2]]
    terms = [[a[0] * x[0], -a[1] * x[1], -a[2] * x[2], -a[3] * x[3]],
             [a[0] * x[1], a[1] * x[0], a[2] * x[3], -a[3] * x[2]],
             [a[0] * x[2], -a[1] * x[3], a[2] * x[0], a[3] * x[1]],
             [a[0] * x[3], a[1] * x[2], -a[2] * x[1], a[3] * x[0]]]
    return [(sum(t), sum(abs(v) for v in t)) for t in terms]


@pytest.fixture(scope="module")
def plus_case():
    rng = np.random.default_rng(41)
    xs, steps = _quaternions(rng, 12), _plus_steps(rng)
    X = np.array([x for x in xs for _ in steps])
    D = np.array([d for _ in xs for d, _ in steps])
    branch = [b for _ in xs for _, b in steps]
    return X, D, branch


def test_quat_plus_against_ceres_plus_in_mpmath_on_both_branches(plus_case):
    """Each component within 8 u sum_i |a_i| |x_i| of the exact Plus: the series (<= 0.54 u each for cos n and sin n / n over
    n^2 < 1/16) or OCML's documented 2 ulp for sin / cos, one rounding for a_i = s d_i, four for the dot."""
    X, D, branch = plus_case
    got = dp.quat_plus(X, D)
    worst = {"series": 0.0, "libm": 0.0}
    for k in range(X.shape[0]):
        if branch[k] == "unchanged":   # n2 == 0 (|d| = 1e-170: d * d underflows): x comes back as it went in
            assert _same_bits(got[k], X[k]), (X[k], D[k])
            continue
        for c, (ref, mag) in enumerate(_plus_mp(X[k], D[k])):
            err, bound = abs(mpf(float(got[k, c])) - ref), 8 * U * mag
            assert err <= bound, (X[k].tolist(), D[k].tolist(), c, float(err / (U * mag)))
            worst[branch[k]] = max(worst[branch[k]], float(err / bound))
    _report("quat_plus, series branch (8 u sum|a_i||x_i|)", worst["series"])
    _report("quat_plus, libm branch (8 u sum|a_i||x_i|)", worst["libm"])


def test_quat_plus_tab_gives_the_bits_of_quat_plus(plus_case):
    X, D, _ = plus_case
    assert _same_bits(dp.quat_plus(X, D, tab=True), dp.quat_plus(X, D))


def test_plus_series_table_holds_the_correctly_rounded_taylor_coefficients():
    """kPlusCoef[0..7]: cos n - 1 in n^2, (-1)^(k+1) / (2k + 2)!; [8..15]: sin n / n - 1, (-1)^(k+1) / (2k + 3)!. The last three
    of each half move the result by less than u / 2 over n^2 < 1/16 (|c_14| n^14 <= 2.8e-21): no output of quat_plus_tab can
    show a wrong digit there, so the table is read back and compared itself."""
    want = [float((-1) ** (k + 1) / mp.factorial(2 * k + 2)) for k in range(8)] + \
           [float((-1) ** (k + 1) / mp.factorial(2 * k + 3)) for k in range(8)]
    assert _same_bits(dp.plus_coef(), np.array(want))


def test_quat_to_R_is_the_rotation_of_the_normalised_quaternion():
    """Entrywise within 16 u of the rotation matrix of x / |x|, R^T R - I within 32 u (entries of a rotation are <= 1)."""
    rng = np.random.default_rng(42)
    Q = _quaternions(rng, 64)
    got = dp.quat_to_R(Q)
    worst_r, worst_o = 0.0, 0.0
    for k in range(Q.shape[0]):
        q = [mpf(float(v)) for v in Q[k]]
        nrm = mp.sqrt(sum(v * v for v in q))
        w, x, y, z = [v / nrm for v in q]
        ref = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
               [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
               [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
        R = [[mpf(float(got[k, i, j])) for j in range(3)] for i in range(3)]
        for i in range(3):
            for j in range(3):
                err = abs(R[i][j] - ref[i][j])
                assert err <= 16 * U, (Q[k].tolist(), i, j, float(err / U))
                worst_r = max(worst_r, float(err / (16 * U)))
                orth = abs(sum(R[m][i] * R[m][j] for m in range(3)) - (1 if i == j else 0))
                assert orth <= 32 * U, (Q[k].tolist(), i, j, float(orth / U))
                worst_o = max(worst_o, float(orth / (32 * U)))
    _report("quat_to_R entries (16 u)", worst_r)
    _report("quat_to_R orthogonality (32 u)", worst_o)


# ---------------------------------------------------------------------------------------------------------------------
# pose_grad_proj_max, pose_grad_proj_max_tab
# ---------------------------------------------------------------------------------------------------------------------
def _grad_cases(rng):
    """(q, g, kind): kind 'proj' (|g_rot| < 1/4), 'tangent' (>= 1/4). Near 1/4 along one axis only: there n2 is exact."""
    qs = _quaternions(rng, 8)
    out = []
    for q in qs:
        for gt_mag in (0.0, 1e-12, 1e-3):
            gt = gt_mag * rng.standard_normal(3)
            rots = [((0.0, 0.0, 0.0), "proj")]
            for mag in (1e-12, 1e-10, 1e-6, 1e-3, 0.1):
                v = rng.standard_normal(3)
                rots.append((tuple((mag * v / np.linalg.norm(v)).tolist()), "proj"))
                rots.append((_axis_steps(mag)[int(rng.integers(0, 6))], "proj"))
            rots += [(d, "proj") for d in _axis_steps(float(np.nextafter(0.25, 0.0)))[:2]]
            for mag in (0.25, float(np.nextafter(0.25, 1.0))):
                rots += [(d, "tangent") for d in _axis_steps(mag)[2:4]]
            for mag in (1.0, 10.0, 1e6):
                v = rng.standard_normal(3)
                rots.append((tuple((mag * v / np.linalg.norm(v)).tolist()), "tangent"))
            out += [(q, np.concatenate([np.array(r), gt]), kind) for r, kind in rots]
    return out


@pytest.fixture(scope="module")
def grad_case():
    cases = _grad_cases(np.random.default_rng(51))
    return np.array([c[0] for c in cases]), np.array([c[1] for c in cases]), [c[2] for c in cases]


def test_pose_grad_proj_max_against_the_projected_step_in_mpmath(grad_case):
    """|g_rot| < 1/4: || q - Plus(q, -g_rot) ||_inf joined with |g_t|_inf. Each of the four quaternion components is a sum of
    four products and is held to 8 u times the sum of their absolute values (eps_i); the translation components are exact.
    The maximum of quantities each within eps_i of its exact value is within max eps_i over the components that can win --
    those whose exact value plus eps_i reaches the largest (exact value minus its eps). |g_rot| >= 1/4: the bits of max |g_i|."""
    Q, G, kind = grad_case
    got = dp.pose_grad_proj_max(Q, G)
    worst = 0.0
    for k in range(Q.shape[0]):
        if kind[k] == "tangent":
            assert got[k] == np.abs(G[k]).max(), (Q[k], G[k])
            continue
        w, v0, v1, v2 = [mpf(float(v)) for v in Q[k]]
        g = [mpf(float(v)) for v in G[k]]
        n = mp.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
        c1, s = 1 - mp.cos(n), (mp.sin(n) / n if n != 0 else mpf(1))
        terms = [[c1 * w, -s * g[0] * v0, -s * g[1] * v1, -s * g[2] * v2],
                 [c1 * v0, s * w * g[0], s * g[1] * v2, -s * g[2] * v1],
                 [c1 * v1, s * w * g[1], s * g[2] * v0, -s * g[0] * v2],
                 [c1 * v2, s * w * g[2], s * g[0] * v1, -s * g[1] * v0]]
        plus = [p[0] for p in _plus_mp(Q[k], -G[k, :3])]
        for c in range(4):   # the two ways of writing the reference agree: q - Plus(q, -g) is the sum of these terms
            assert abs((mpf(float(Q[k, c])) - plus[c]) - sum(terms[c])) <= mpf(10) ** -40 * (1 + abs(mpf(float(Q[k, c]))))
        vals = [abs(sum(t)) for t in terms] + [max(abs(g[3]), abs(g[4]), abs(g[5]))]
        eps = [8 * U * sum(abs(v) for v in t) for t in terms] + [mpf(0)]
        ref = max(vals)
        floor = max(v - e for v, e in zip(vals, eps))
        bound = max(e for v, e in zip(vals, eps) if v + e >= floor)
        err = abs(mpf(float(got[k])) - ref)
        assert err <= bound, (Q[k].tolist(), G[k].tolist(), float(err), float(bound))
        if bound > 0:
            worst = max(worst, float(err / bound))
    _report("pose_grad_proj_max (8 u sum|terms| of the winning component)", worst)


def test_pose_grad_proj_max_tab_gives_the_bits_of_pose_grad_proj_max(grad_case):
    Q, G, _ = grad_case
    assert _same_bits(dp.pose_grad_proj_max(Q, G, tab=True), dp.pose_grad_proj_max(Q, G))


def test_pose_grad_proj_max_with_a_nan_rotation_component_reports_the_rest():
    """Recorded in cc_common.hpp: a NaN in g_rot makes n2 NaN, `!(n2 < 0.0625)` takes the tangent branch, and fmax treats the
    NaN as missing -- what comes back is the largest |g_i| of the five other components, finite, in both forms."""
    rng = np.random.default_rng(52)
    Q = _quaternions(rng, 6)
    G = rng.standard_normal((6, 6)) * 10.0 ** rng.uniform(-6, 1, size=(6, 1))
    for k in range(6):
        G[k, k % 3] = np.nan
    want = np.nanmax(np.abs(G), axis=1)
    for tab in (False, True):
        assert _same_bits(dp.pose_grad_proj_max(Q, G, tab=tab), want)


# ---------------------------------------------------------------------------------------------------------------------
# granule / ungranule, untri, persist_spec_radius
# ---------------------------------------------------------------------------------------------------------------------
def test_granule_round_trip_is_bit_exact_and_tagged_in_both_halves():
    rng = np.random.default_rng(61)
    special = [0.0, -0.0, SUB_MIN, -SUB_MIN, float(np.nextafter(DBL_MIN, 0.0)), np.inf, -np.inf, DBL_MAX, 1.0]
    bits = [struct.unpack("<Q", struct.pack("<d", v))[0] for v in special]
    bits += [0x7FF8000000000000, 0x7FF0000000000001, 0xFFF8DEADBEEF1234, 0x7FF4000000ABCDEF, 0xFFFFFFFFFFFFFFFF]   # NaNs with payloads
    bits = np.concatenate([np.array(bits, dtype=np.uint64), rng.integers(0, 2 ** 64, size=4096, dtype=np.uint64)])
    tags = rng.integers(0, 2 ** 32, size=bits.size, dtype=np.uint64).astype(np.uint32)
    tags[:4] = [0, 1, 0xFFFFFFFF, 0x80000000]
    words, back = dp.granule_round_trip(tags, bits)
    assert np.array_equal(back, bits)
    t64 = tags.astype(np.uint64) << np.uint64(32)
    assert np.array_equal(words[:, 0], t64 | (bits & np.uint64(0xFFFFFFFF)))
    assert np.array_equal(words[:, 1], t64 | (bits >> np.uint64(32)))


def test_untri_inverts_the_packed_lower_index():
    want, idx = [], 0
    for i in range(16):
        for j in range(i + 1):
            assert idx == i * (i + 1) // 2 + j
            want.append((i, j))
            idx += 1
    assert len(want) == 136
    assert dp.untri(136).tolist() == [list(p) for p in want]


def test_persist_spec_radius_is_lm_apply_at_quality_one():
    """The workers' speculative radius and lm_apply's radius after an accepted step of quality 1 (2 rho - 1 = 1: the
    divisor is max(1/3, 0) = 1/3) are one expression; also against IEEE double arithmetic in Python."""
    rng = np.random.default_rng(62)
    r = np.concatenate([10.0 ** np.linspace(-32, 16, 97), 10.0 ** rng.uniform(-32, 16, size=400)])
    mx = np.concatenate([np.full(r.size, 1e16), np.full(r.size, 1.0), np.full(r.size, 3e-5), np.full(r.size, 1e32)])
    r = np.tile(r, 4)
    got = dp.spec_radius(r, mx)
    assert _same_bits(got[:, 0], got[:, 1])
    want = np.array([min(m, x / (1.0 / 3.0)) for x, m in zip(r.tolist(), mx.tolist())])
    assert _same_bits(got[:, 0], want)
    assert (got[:, 0] == mx).any() and (got[:, 0] < mx).any()   # both sides of the clamp


# ---------------------------------------------------------------------------------------------------------------------
# Cholesky solves: chol_solve_rows<S>, chol_block4 + chol_backward<false>
# ---------------------------------------------------------------------------------------------------------------------
FAMILIES = ["kappa 1", "kappa 1e6", "kappa 1e12", "unit diagonal"]
BAD_PIVOTS = ["zero", "negative", "+inf", "nan"]


def _spd(rng, S, family):
    """Random SPD from an orthogonal factor and a graded spectrum; 'unit diagonal': a badly row-scaled kappa-1e6 matrix after
    the Jacobi scaling the solver applies, diagonal exactly one."""
    Qf, _ = np.linalg.qr(rng.standard_normal((S, S)))
    kappa = {"kappa 1": 1.0, "kappa 1e6": 1e6, "kappa 1e12": 1e12, "unit diagonal": 1e6}[family]
    A = (Qf * np.logspace(0.0, -math.log10(kappa), S)) @ Qf.T if S > 1 else np.array([[1.0 / math.sqrt(kappa)]])
    if family == "unit diagonal":
        D = 10.0 ** rng.uniform(-3, 3, size=S)
        A = D[:, None] * A * D[None, :]
        sc = 1.0 / np.sqrt(np.diag(A))
        A = sc[:, None] * A * sc[None, :]
        np.fill_diagonal(A, 1.0)
    A = np.tril(A) + np.tril(A, -1).T   # exactly symmetric: the routines read the lower triangle
    return A, rng.standard_normal(S)


def _spoil_pivot(A, j, how):
    """Edit the diagonal so that pivot j of the factorisation is exactly 0, negative, +inf or NaN. (For an exact zero the
    row and the column of j go with it: the pivot is a_jj minus the squares of row j of the factor.)"""
    A = A.copy()
    if how == "zero":
        A[j, :] = 0.0
        A[:, j] = 0.0
    else:
        A[j, j] = {"negative": -1.0, "+inf": np.inf, "nan": np.nan}[how]
    return A


def _backward_error_ratio(A, b, x, gamma_terms):
    """max_i |b - A x|_i / (gamma |L| |L^T| |x|)_i, L the exact Cholesky factor of A, everything in mpmath."""
    S = A.shape[0]
    Am = mp.matrix(A.tolist())
    L = mp.cholesky(Am)
    xm = [mpf(float(v)) for v in x]
    t = [sum(abs(L[k, i]) * abs(xm[k]) for k in range(i, S)) for i in range(S)]       # |L^T| |x|
    bound = [gamma_terms * U * sum(abs(L[i, k]) * t[k] for k in range(i + 1)) for i in range(S)]
    res = [abs(mpf(float(b[i])) - sum(Am[i, k] * xm[k] for k in range(S))) for i in range(S)]
    return max(float(r / bd) for r, bd in zip(res, bound))


@pytest.mark.parametrize("S", [6, 9, 12, 18, 24])
def test_chol_solve_rows_backward_error_contract_and_pivot_report(S):
    """Componentwise backward error |b - A x| <= gamma |L| |L^T| |x|, gamma = (3 S + 9) u: Higham's bound for a Cholesky
    solve (Accuracy and Stability, thm 10.4: gamma_{3n+1}) with the constant raised for the approximate reciprocal root.
    The contract of cc_device.hpp: x the same in all 64 lanes; what lanes >= S and the entries beyond each row's diagonal
    hold does not matter; the return value is whether every pivot was positive and finite."""
    rng = np.random.default_rng(700 + S)
    clean = [_spd(rng, S, fam) for fam in FAMILIES]
    js = sorted({0, S // 2, S - 1})
    bad = [(_spoil_pivot(clean[1][0], j, how), clean[1][1]) for j in js for how in BAD_PIVOTS]

    def lanes(A, b, variant):
        a, bl = np.empty((64, S)), np.empty(64)
        for l in range(64):
            i = min(l, S - 1)                     # (as rig_solve_block: lanes beyond the system repeat its last row)
            a[l], bl[l] = A[i], b[i]              # beyond the diagonal: the symmetric entries
        if variant == 1:                          # other finite values wherever the contract says nobody looks
            for l in range(S):
                a[l, l + 1:] = _mixed(rng, S - l - 1)
            a[S:], bl[S:] = _mixed(rng, (64 - S, S)), _mixed(rng, 64 - S)
        return a, bl

    packs = [lanes(A, b, 0) for A, b in clean] + [lanes(A, b, 1) for A, b in clean] + [lanes(A, b, 0) for A, b in bad]
    x, ok = dp.chol_solve_rows(np.array([p[0] for p in packs]), np.array([p[1] for p in packs]))
    n = len(clean)
    worst = 0.0
    for k, (A, b) in enumerate(clean):
        assert (ok[k] == 1).all() and (ok[n + k] == 1).all(), FAMILIES[k]
        assert all(_same_bits(x[k, l], x[k, 0]) for l in range(64)), FAMILIES[k]
        assert _same_bits(x[n + k], x[k]), FAMILIES[k]
        ratio = _backward_error_ratio(A, b, x[k, 0], 3 * S + 9)
        assert ratio <= 1.0, (FAMILIES[k], ratio)
        worst = max(worst, ratio)
    for k, (j, how) in enumerate((j, how) for j in js for how in BAD_PIVOTS):
        assert (ok[2 * n + k] == 0).all(), (j, how)
    _report(f"chol_solve_rows<{S}> backward error ((3 S + 9) u |L||L^T||x|)", worst)


@pytest.mark.parametrize("S", list(range(1, 64)))
def test_chol_block4_and_backward_substitution_at_every_size_up_to_63(S):
    """Every S the routine's own comment admits (S <= 63), not only the 6 a + 9 b the product reaches: the tile-edge logic
    (n16, ina / inb, a last block narrower than four, ten tiles over three waves) has a different shape at almost every
    size. Matrix and right-hand side (row S) in LDS as rig_solve_block lays them out, 256 threads. Same families, same
    bound, same bad pivots as chol_solve_rows."""
    rng = np.random.default_rng(900 + S)
    clean = [_spd(rng, S, fam) for fam in FAMILIES]
    js = sorted({0, S // 2, S - 1})
    bad = [(_spoil_pivot(clean[1][0], j, how), clean[1][1]) for j in js for how in BAD_PIVOTS]

    def image(A, b):
        M = np.zeros((S + 1, S + 1))
        M[:S, :S] = np.tril(A)
        M[S, :S] = b
        return M

    x, ok = dp.chol_block4(np.array([image(A, b) for A, b in clean + bad]))
    worst = 0.0
    for k, (A, b) in enumerate(clean):
        assert (ok[k] == 1).all(), FAMILIES[k]
        ratio = _backward_error_ratio(A, b, x[k], 3 * S + 9)
        assert ratio <= 1.0, (FAMILIES[k], ratio)
        worst = max(worst, ratio)
    for k, (j, how) in enumerate((j, how) for j in js for how in BAD_PIVOTS):
        assert (ok[len(clean) + k] == 0).all(), (j, how)
    _report(f"chol_block4 S = {S} backward error ((3 S + 9) u |L||L^T||x|)", worst)
