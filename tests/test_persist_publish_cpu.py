"""How k_intr_persist hands a finished solve's control block to the host is written once, in csrc/cc_persist_publish.hpp: 36
self-validating words {tag32 : half}, tag = the solve's sequence number. tests/cpp/persist_publish_words.cpp compiles that header
with the host compiler and checks pack / validate / unpack: every class of bit pattern of a double round-trips (+-0, subnormals,
infinities, NaN payloads) in every position; a block in which any one of the 36 words still carries the previous tag is not ready, nor
is a block of all-older tags; the tag after 0xffffffff is 1, not 0, so that a zeroed block never satisfies a wait. The program is
also built with -fsanitize=address,undefined and run as its own executable. No GPU."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "camera_calibrator_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "persist_publish_words.cpp")


def _build_and_run(tmp_path, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "needs a host compiler"
    exe = str(tmp_path / name)
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, SRC, "-o", exe] + extra,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 1000, r.stdout[-500:]
    assert not r.stderr.strip(), r.stderr[-2000:]


def test_tagged_words_round_trip_and_validate(tmp_path):
    _build_and_run(tmp_path, "persist_publish_words", [])


def test_tagged_words_under_the_host_sanitizers(tmp_path):
    _build_and_run(tmp_path, "persist_publish_words_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_kernel_and_host_use_the_one_definition():
    kernel = open(os.path.join(CSRC, "cc_intrinsics_persist.hip")).read()
    host = open(os.path.join(CSRC, "cc_solve_host.hpp")).read()
    for text in (kernel, host):
        assert '#include "cc_persist_publish.hpp"' in text
        assert "publish_tag(" in text and "kPubTaggedAt" in text
    assert "publish_word(" in kernel and "publish_unpack(" in host and "publish_ready(" in host
