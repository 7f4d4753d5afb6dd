"""The residual-only sweep of k_intr_persist on the CPU: (1) its index map, csrc/cc_persist_pack.hpp, compiled on the host and
checked against the order in which the full sweep's matrix products add the residuals (tests/cpp/persist_pack_map.cpp);
(2) the register allocation of k_intr_persist<1|2|4>, which may not cost more than before the residual-only sweep was added:
the table of the parent commit's cc_intrinsics_persist.hip, cross-compiled for gfx950 with the same compiler
(profiles/r22/intr_final_sweep_ab.txt has both tables)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "camera_calibrator_amd", "csrc")

# vector registers, spilled vector registers, scratch bytes of the parent commit's build
PARENT_TABLE = {"k_intr_persist<1>": (156, 0, 0), "k_intr_persist<2>": (138, 0, 0), "k_intr_persist<4>": (128, 0, 0)}


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host compiler")
def test_the_packed_chains_visit_the_residuals_in_the_full_sweeps_order(tmp_path):
    exe = str(tmp_path / "persist_pack_map")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "persist_pack_map.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) frames, 0 mismatches", r.stdout)
    assert m and int(m.group(1)) == 1100, r.stdout[-500:]


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_the_residual_only_sweep_costs_no_registers():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_regs.py"), os.path.join(CSRC, "cc_intrinsics_persist.hip")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    rows = {}
    for line in r.stdout.splitlines()[1:]:
        m = re.match(r"(\S.*?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)$", line)
        if m:
            rows[m.group(1)] = dict(zip(("vgpr", "agpr", "sgpr", "vspill", "sspill", "scratch", "lds"), map(int, m.groups()[1:])))
    for k, (vgpr, vspill, scratch) in PARENT_TABLE.items():
        assert rows[k]["vgpr"] <= vgpr and rows[k]["vspill"] <= vspill and rows[k]["scratch"] <= scratch, (k, rows[k], "parent", (vgpr, vspill, scratch))
