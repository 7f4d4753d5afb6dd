"""Register budget and kernel set of the lens unit of the rig solve with intrinsics (cc_rig_lens.hip: the fisheye model and a
model per camera) and the kernel set of the pixel start's unit (cc_rigk_start.hip), checked on the CPU as
tests/test_kernel_budgets.py does for the other units (hipcc cross-compiles gfx950 without a GPU; scripts/kernel_regs.py reads
the code object metadata).
The sweep k_rig_sweep_lens<NW, MODEL, LIST> keeps the budget of its MODEL's rows: the radial-tangential ones the 168 registers of
three waves per SIMD, where k_rig_sweep_adjk sits; the fisheye ones are compiled for TWO waves per SIMD (256 registers): at 168
the compiler spills 2 (one wave per group) / 11 (four) registers with reloads inside the pass loop; at two it reports 175 / 185
registers, no spill, no scratch. No kernel spills a vector register or uses scratch (DESIGN.md 4.14 and 4.17 have the tables)."""
import os

import pytest

from tests.test_kernel_budgets import _table

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

# k_rig_sweep_lens<waves per group, model (0 radial-tangential, 1 fisheye), groups from a list>
RADTAN = ("k_rig_sweep_lens<1, 0, true>", "k_rig_sweep_lens<4, 0, true>")
FISHEYE_LIST = ("k_rig_sweep_lens<1, 1, true>", "k_rig_sweep_lens<4, 1, true>")
FISHEYE_ALL = ("k_rig_sweep_lens<1, 1, false>", "k_rig_sweep_lens<4, 1, false>")
COSTS = ("cc::k_rig_obs_cost_fisheye", "cc::k_rig_obs_cost_mixed")
START = ("cc::k_rigk_start_unproject", "cc::k_rigk_start_unproject_cam", "cc::k_rigk_start_bearing", "cc::k_rigk_start_bearing_cam")


def test_no_kernel_of_the_lens_unit_spills_or_uses_scratch():
    t = _table("cc_rig_lens.hip")
    for k in RADTAN + FISHEYE_LIST + FISHEYE_ALL + COSTS:
        assert t[k]["vspill"] == 0 and t[k]["scratch"] == 0, (k, t[k])
    t = _table("cc_rigk_start.hip")
    k = "cc::k_rigk_start_unproject_cam"
    assert t[k]["vspill"] == 0 and t[k]["scratch"] == 0, (k, t[k])


def test_each_sweep_keeps_the_register_budget_of_its_model():
    t = _table("cc_rig_lens.hip")
    for k in RADTAN:
        assert t[k]["vgpr"] + t[k]["agpr"] <= 168, (k, t[k])            # three waves per SIMD, as k_rig_sweep_adjk
    for k in FISHEYE_LIST + FISHEYE_ALL:
        assert 168 < t[k]["vgpr"] + t[k]["agpr"] <= 256, (k, t[k])      # two waves per SIMD, and no room at three: see above
    for one, four in (RADTAN, FISHEYE_LIST, FISHEYE_ALL):
        assert t[one]["lds"] <= 16 * 1024 and t[four]["lds"] <= 40 * 1024


def test_the_lens_unit_is_these_kernels():
    assert set(_table("cc_rig_lens.hip")) == set(RADTAN + FISHEYE_LIST + FISHEYE_ALL + COSTS)


def test_the_pixel_start_unit_is_these_kernels():
    assert set(_table("cc_rigk_start.hip")) == set(START)
