"""Register budget and kernel set of the per-camera-model rig unit (cc_rig_mixed.hip), checked on the CPU as
tests/test_rigk_fisheye_budgets.py does for its unit (hipcc cross-compiles gfx950 without a GPU; scripts/kernel_regs.py reads the
code object metadata). Each instantiation of the sweep keeps the budget of the homogeneous kernel it restates: the
radial-tangential rows the 168 registers of three waves per SIMD (k_rig_sweep_adjk), the fisheye rows the 256 of two
(k_rig_sweep_adjk_fisheye); no new kernel spills a vector register or uses scratch (DESIGN.md 4.17 has the table)."""
import os

import pytest

from tests.test_kernel_budgets import _table

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

RADTAN = ("k_rig_sweep_adjk_sel<1, 0>", "k_rig_sweep_adjk_sel<4, 0>")
FISHEYE = ("k_rig_sweep_adjk_sel<1, 1>", "k_rig_sweep_adjk_sel<4, 1>")
OTHERS = ("cc::k_rig_obs_cost_mixed", "cc::k_rigk_start_unproject_cam")


def test_no_kernel_of_the_mixed_unit_spills_or_uses_scratch():
    t = _table("cc_rig_mixed.hip")
    for k in RADTAN + FISHEYE + OTHERS:
        assert t[k]["vspill"] == 0 and t[k]["scratch"] == 0, (k, t[k])


def test_each_sweep_keeps_the_register_budget_of_its_model():
    t = _table("cc_rig_mixed.hip")
    for k in RADTAN:
        assert t[k]["vgpr"] + t[k]["agpr"] <= 168, (k, t[k])            # three waves per SIMD, as k_rig_sweep_adjk
    for k in FISHEYE:
        assert t[k]["vgpr"] + t[k]["agpr"] <= 256, (k, t[k])            # two, as k_rig_sweep_adjk_fisheye
    for one, four in (RADTAN, FISHEYE):
        assert t[one]["lds"] <= 16 * 1024 and t[four]["lds"] <= 40 * 1024


def test_the_mixed_unit_is_these_kernels():
    assert set(_table("cc_rig_mixed.hip")) == set(RADTAN + FISHEYE + OTHERS)
