"""k_intr_persist adds the workers' elimination rows up by COLUMN OWNERS (worker c mod G pulls column c of every row and posts one
total; the control reads eighty totals) where leaders used to add sixteen whole rows each. Who pulls which words changes, the sums
do not: every column keeps the operands and the order of the two-level gather (csrc/cc_persist_sum.hpp, checked on the host by
tests/test_persist_sum_order_cpu.py), so the solver has to give, BIT FOR BIT, what it gave before. The goldens of
tests/test_gpu_intr_seam_polls.py stop at 37 workers, fewer than the eighty columns; tests/golden/intr_column_owners_parent.npz was
recorded on the GPU from the parent commit (tests/golden/make_intr_column_owners.py) on 203 ragged frames: with one, two and four
frames per workgroup that is 203, 102 and 51 workers -- owners of one column and thirteen groups with a last one of eleven rows,
seven groups with a last one of six, and fewer workers than columns (workers 0..28 own two). The same three kinds of solve in each
form: (a) default options, every intrinsic free and k3 / p1 / p2 held; (b) a solve from a bad start under a demanding acceptance
threshold, whose rejected and mediocre steps take the miss path (second elimination, the rbox / e3 seam); (c) solve, continued
solve, reset, solve on ONE handle -- the epochs run on from launch to launch, a word an earlier launch left in a box must not
satisfy a later wait."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _generator():
    spec = importlib.util.spec_from_file_location("make_intr_column_owners", os.path.join(HERE, "golden", "make_intr_column_owners.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(HERE, "golden", "intr_column_owners_parent.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def solved(recorded):
    gen = _generator()
    assert list(recorded["points"]) == gen.POINTS and list(np.diff(recorded["in_off"])) == gen.POINTS and len(gen.POINTS) == 203
    return gen.seam_polls().solve_all({k[3:]: v for k, v in recorded.items() if k.startswith("in_")})


def _assert_bit_equal(got_all, want_all, got_key, want_key):
    assert int(got_all[got_key + "iterations"]) == int(want_all[want_key + "iterations"]), (got_key, want_key)
    for field in ("accepted", "costs", "radii", "intr", "q", "t"):
        got, want = np.ascontiguousarray(got_all[got_key + field]), np.ascontiguousarray(want_all[want_key + field])
        assert got.shape == want.shape and got.dtype == want.dtype, (field, got.shape, want.shape)
        diff = np.flatnonzero(got.view(np.uint8).reshape(-1) != want.view(np.uint8).reshape(-1))
        assert diff.size == 0, (got_key, want_key, field, "first differing element", int(diff[0]) // got.itemsize,
                                got.reshape(-1)[diff[0] // got.itemsize], want.reshape(-1)[diff[0] // got.itemsize])


@pytest.mark.parametrize("mask", ["free", "distortion_held"])
@pytest.mark.parametrize("teams", [1, 2, 4])
def test_default_solve_is_bit_equal_to_the_parent_commit(recorded, solved, teams, mask):
    k = "t%d_%s_" % (teams, mask)
    assert int(recorded[k + "iterations"]) >= 3          # (the fixture is a solve, not a start that ends at once)
    _assert_bit_equal(solved, recorded, k, k)


@pytest.mark.parametrize("teams", [1, 2, 4])
def test_solve_over_the_miss_path_is_bit_equal_to_the_parent_commit(recorded, solved, teams):
    k = "t%d_miss_" % teams
    acc = list(recorded[k + "accepted"])
    # every rejected step is a miss (the workers assumed acceptance), and so is the accepted step behind one (the radius is not
    # where the assumption put it): the recording itself has to have taken the second elimination, more than once
    assert acc.count(0) >= 2 and acc.count(1) >= 2, acc
    _assert_bit_equal(solved, recorded, k, k)


@pytest.mark.parametrize("teams", [1, 2, 4])
def test_solves_on_one_handle_are_bit_equal_to_the_parent_commit(recorded, solved, teams):
    k = "t%d_seq" % teams
    assert int(recorded[k + "0_iterations"]) >= 2 and int(recorded[k + "1_iterations"]) >= 1   # (the continued solve had work left)
    _assert_bit_equal(solved, recorded, k + "0_", k + "0_")      # first solve
    _assert_bit_equal(solved, recorded, k + "1_", k + "1_")      # continued solve: the parent's recording of the same sequence
    _assert_bit_equal(solved, recorded, k + "2_", k + "2_")      # after the reset ...
    _assert_bit_equal(solved, recorded, k + "2_", k + "0_")      # ... the first solve again
    _assert_bit_equal(recorded, recorded, k + "2_", k + "0_")
