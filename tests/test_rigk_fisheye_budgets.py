"""Register budget and kernel set of the fisheye rig unit (cc_rig_fisheye.hip), checked on the CPU as tests/test_kernel_budgets.py
does for the other units (hipcc cross-compiles gfx950 without a GPU; scripts/kernel_regs.py reads the code object metadata).
The sweep is compiled for TWO waves per SIMD (256 registers): at the 168 of three -- where k_rig_sweep_adjk sits -- the compiler
spills 2 (one wave per group) / 11 (four) registers with reloads inside the pass loop; at two it reports 175 / 185 registers,
no spill, no scratch (DESIGN.md 4.14 has the table)."""
import os

import pytest

from tests.test_kernel_budgets import _table

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


def test_fisheye_rig_sweeps_neither_spill_nor_use_scratch():
    t = _table("cc_rig_fisheye.hip")
    for k in ("k_rig_sweep_adjk_fisheye<1>", "k_rig_sweep_adjk_fisheye<4>"):
        assert t[k]["vspill"] == 0 and t[k]["scratch"] == 0, (k, t[k])
        assert 168 < t[k]["vgpr"] + t[k]["agpr"] <= 256, (k, t[k])      # two waves per SIMD, and no room at three: see above
    assert t["k_rig_sweep_adjk_fisheye<1>"]["lds"] <= 16 * 1024 and t["k_rig_sweep_adjk_fisheye<4>"]["lds"] <= 40 * 1024
    assert t["cc::k_rig_obs_cost_fisheye"]["vspill"] == 0 and t["cc::k_rig_obs_cost_fisheye"]["scratch"] == 0


def test_the_fisheye_rig_unit_is_these_kernels():
    assert set(_table("cc_rig_fisheye.hip")) == {"k_rig_sweep_adjk_fisheye<1>", "k_rig_sweep_adjk_fisheye<4>", "cc::k_rig_obs_cost_fisheye"}
