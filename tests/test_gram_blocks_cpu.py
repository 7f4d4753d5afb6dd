"""The Gram product on 4 x 4 blocks (csrc/cc_gram_blocks.hpp) on the CPU: the index map compiled on the host and checked against
gram_products' order (tests/cpp/gram_blocks_map.cpp) -- one block of every transposed pair, for both chains, exactly once, every
operand lane on the row and component its block needs, the reduction placing all 256 entries, and a host emulation
with one fused multiply-add per term that reproduces the emulation of today's products and reduction bit for bit."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "camera_calibrator_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host compiler")
def test_the_block_products_form_every_entry_as_the_16x16x4_products_do(tmp_path):
    exe = str(tmp_path / "gram_blocks_map")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "gram_blocks_map.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) entries, 0 mismatches", r.stdout)
    assert m and int(m.group(1)) == 6 * 256, r.stdout[-500:]
