"""What the oracle does with the scenarios of tests/test_gpu_intr_batch_branches.py, without a GPU: each builder asserts the
outcomes its GPU test relies on (which steps are rejected or invalid, which termination in which iteration, how far every
deciding quantity of the mixed-termination batch is from its threshold)."""
import pytest

from tests import test_gpu_intr_batch_branches as scenarios


@pytest.mark.parametrize("i", range(len(scenarios.REJECT_SETS)))
def test_reject_scenarios(i):
    scenarios._scenario_a(i)


@pytest.mark.parametrize("i", range(len(scenarios.TERMINATION_SETS)))
def test_termination_scenarios(i):
    scenarios._scenario_b(i)


def test_later_gradient_and_unscaled_scenarios():
    scenarios._scenario_b_gradient()
    scenarios._scenario_b_no_jacobi()


def test_mixed_termination_scenario_and_its_margins():
    probs, oracle, margins = scenarios._scenario_b_mixed()
    assert scenarios._terms(oracle) == ["PARAMETER", "NO_CONVERGENCE", "GRADIENT", "PARAMETER", "PARAMETER", "GRADIENT"]
    for p, ms in enumerate(margins):
        for m in ms:
            print(p, *m)
    assert min(m[4] for ms in margins for m in ms) >= scenarios.MIXED_MARGIN


@pytest.mark.parametrize("layout", ["empty_last", "empty_first"])
def test_shape_scenarios(layout):
    scenarios._scenario_c(layout)


def test_empty_invalid_and_tiny_scenarios():
    scenarios._scenario_d()
    scenarios._scenario_e()
    scenarios._scenario_e_late()
    scenarios._scenario_h()
