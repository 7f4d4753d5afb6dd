"""Register budgets of the hot kernels, checked on the CPU (hipcc cross-compiles gfx950 without a GPU; scripts/kernel_regs.py
reads the code object metadata). Round 4 lost 25 us per launch of k_rig_sweep_adj<1> at BASELINE configs[4] size to ONE scalar
branch + atomic added at the top of the kernel: the register allocation moved from 126 VGPRs / 87 SGPRs without spills to
128 / 66 with ten spilled registers, and nothing but an A/B against the previous round's library on the same box showed it.
These assertions break when a kernel whose speed rests on its allocation leaves it."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_tables = {}


def _table(src):
    if src not in _tables:   # (one cross-compilation per source file and session: ~40 s each)
        _tables[src] = _compile_table(src)
    return _tables[src]


def _compile_table(src):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_regs.py"), os.path.join(ROOT, "camera_calibrator_amd", "csrc", src)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = {}
    for line in r.stdout.splitlines()[1:]:
        m = re.match(r"(\S.*?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)$", line)
        if m:
            rows[m.group(1)] = dict(zip(("vgpr", "agpr", "sgpr", "vspill", "sspill", "scratch", "lds"), map(int, m.groups()[1:])))
    return rows


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_rig_sweeps_keep_their_register_allocation():
    t = _table("cc_rig.hip")
    for k in ("k_rig_sweep_adj<1>", "k_rig_sweep_adj<2>", "k_rig_sweep_adj<4>"):
        assert t[k]["vspill"] == 0 and t[k]["scratch"] == 0, (k, t[k])
    assert t["k_rig_sweep_adj<1>"]["vgpr"] <= 128, t["k_rig_sweep_adj<1>"]      # four waves per SIMD
    for k in ("k_rig_sweep_adjk<1>", "k_rig_sweep_adjk<4>"):
        assert t[k]["vspill"] == 0 and t[k]["vgpr"] <= 168, (k, t[k])            # three waves per SIMD
    # round 5, sweep with intrinsics on plain FMAs: 66 accumulators a wave next to the projection at two waves per SIMD. A second
    # register set of prefetched observations (the pair of passes unrolled) spilled 263 registers INTO the main loop: 607 us per
    # launch against 209 at 8 x 2000 x 500 -- nothing may spill there (the few scalar spills sit in the group's head and tail)
    k2 = t["cc::k_rig_sweep_k2"]
    assert k2["vgpr"] <= 256 and k2["vspill"] <= 4 and k2["scratch"] <= 32, k2
    elims = [k for k in t if k.startswith("k_rig_elim<")]
    assert len(elims) == 8, elims   # (round 5: + the two that read the compact records of k_rig_sweep_k2)
    for k in elims:
        assert t[k]["vspill"] == 0 and t[k]["scratch"] == 0, (k, t[k])            # (sits at the 512-register limit by design)
    # the plain large-rig elimination keeps 136 tile accumulators per thread: compile-time pair indices leave it at 8 spilled
    # vector registers and < 100 scalar ones (table-driven pair indices: 229 + 375 -- the reconstruction of round 3's first
    # version, -DCC_EXP_ELIMBIG_TABLES, which passes the suites all the same: DESIGN.md 4.5 item 4; git show 5a0d480:DESIGN.md for the account)
    for k in ("k_rig_elim_big<false>", "k_rig_elim_big<true>"):
        assert t[k]["vspill"] <= 8 and t[k]["sspill"] <= 100, (k, t[k])
    # frame form of the sweep: a wave per group (ONE) at four waves per SIMD -- its few spills are in the once-per-frame assembly,
    # none in the passes (checked on the ISA in round 4: every scratch access lies behind the kernel's barrier); the loop form
    # is compiled for three waves per SIMD and must not spill at all
    for nw in (1, 2, 4, 8):
        one, loop = t["k_rig_sweep_frame<%d, true>" % nw], t["k_rig_sweep_frame<%d, false>" % nw]
        assert one["vgpr"] <= 128 and one["vspill"] <= 3, (nw, one)
        assert loop["vgpr"] <= 168 and loop["vspill"] == 0 and loop["scratch"] == 0, (nw, loop)
    for k in ("k_rig_persist_w<1>", "k_rig_persist_w<2>"):
        assert t[k]["vspill"] == 0 and t[k]["scratch"] == 0, (k, t[k])
    assert t["k_rig_persist_w<4>"]["vgpr"] <= 128 and t["k_rig_persist_w<4>"]["vspill"] <= 20, t["k_rig_persist_w<4>"]   # (1024 threads; the spills are outside the sweep loop, as in round 3)
    # the lean form's control kernel only ever solves S <= 24: the routines for larger systems are not compiled into it
    # (round 5: with them 378 registers + 25 spilled)
    ctl = t["cc::k_rig_persist_ctl"]
    assert ctl["vgpr"] <= 320 and ctl["vspill"] <= 2 and ctl["scratch"] == 0, ctl


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_intrinsics_kernels_keep_their_register_allocation():
    t = _table("cc_intrinsics_persist.hip")
    for k in ("k_intr_persist<1>", "k_intr_persist<2>"):
        assert t[k]["vspill"] == 0 and t[k]["scratch"] == 0, (k, t[k])
    # 1024-thread workgroups: 128 registers. Until round 5 the control workgroup's code spilled 45 registers (the options copied out
    # of LDS and the per-lane selects of the reduced solve, hoisted out of the round loop) and reloaded nine of them one at a time
    # in front of the 9 x 9 factorisation: 0.9 us per round (profiles/r05/intr_control_spills.jsonl). What is left: four
    # round-level values of the workers.
    assert t["k_intr_persist<4>"]["vgpr"] <= 128 and t["k_intr_persist<4>"]["vspill"] <= 8 and t["k_intr_persist<4>"]["scratch"] <= 40, t["k_intr_persist<4>"]
    t = _table("cc_intrinsics.hip")
    k = "cc::k_intr_sweep"
    assert t[k]["vspill"] == 0 and t[k]["scratch"] == 0 and t[k]["vgpr"] <= 128, (k, t[k])


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_every_rig_kernel_is_a_named_form():
    """Round 5 (prune): the rig path's kernels, by name. A form that is added (or an A/B partner that comes back) has to be
    written down here, next to what it is for -- the first formulation of the sweeps (k_rig_sweep, every column through the
    matrix pipe) and the glued persistent kernel (k_rig_persist) are gone and stay gone."""
    t = _table("cc_rig.hip")
    names = {k.replace("cc::", "").split("(")[0] for k in t}
    forms = {
        # sweeps: per (frame, camera) group with 16 x 16 tiles (large rigs, tests), per frame with compact records (default),
        # with intrinsics on the matrix pipe / tiles and on plain FMAs / compact records
        "k_rig_sweep_adj<1>", "k_rig_sweep_adj<2>", "k_rig_sweep_adj<4>",
        *("k_rig_sweep_frame<%d, %s>" % (n, o) for n in (1, 2, 4, 8) for o in ("true", "false")),
        "k_rig_sweep_adjk<1>", "k_rig_sweep_adjk<4>", "k_rig_sweep_k2",
        # steps behind the sweep
        "k_rig_update", "k_rig_stats", "k_rig_flag_exchange", "k_rig_init", "k_rig_collect", "k_rig_records",
        *("k_rig_elim<%s>" % a for a in ("false, 8, false, false", "false, 8, true, false", "false, 24, true, false", "true, 8, false, false",
                                         "false, 24, false, false", "true, 24, false, false", "true, 8, false, true", "true, 24, false, true")),
        "k_rig_reduce<0>", "k_rig_reduce<2>", "k_rig_reduce<3>", "k_rig_reduce<4>", "k_rig_solve<0>", "k_rig_solve<2>",
        # reduced systems of 128 .. 255 coordinates
        "k_rig_elim_big<false>", "k_rig_elim_big<true>", "k_rig_solve_big<true>", "k_rig_solve_big<false>",
        # the lean persistent form
        "k_rig_persist_w<1>", "k_rig_persist_w<2>", "k_rig_persist_w<4>", "k_rig_persist_ctl",
        # creation / read-back helpers
        "k_rig_expand_xyz", "k_rig_obs_cost",
    }
    assert names == forms, (sorted(names - forms), sorted(forms - names))
    assert not any(n.startswith("k_rig_sweep<") or n.startswith("k_rig_persist<") or n == "k_rig_persist" for n in names)
    # the file split of round 5: the host side + launches stay under 2,500 lines, no part above 2,000
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "camera_calibrator_amd", "csrc")
    sizes = {f: sum(1 for _ in open(os.path.join(root, f))) for f in ("cc_rig.hip", "cc_rig_sweeps.hpp", "cc_rig_steps.hpp", "cc_rig_big.hpp", "cc_rig_lean.hpp", "cc_solve_host.hpp")}
    assert sizes["cc_rig.hip"] < 2500 and max(sizes.values()) < 2500, sizes


# ---- round 6: the product translation units carry no timing / ablation / A-B text -----------------------------------------
# Stage marks, early returns of ablation builds, the exact-arithmetic forms and the all-gather probe live in scripts/variants/*.patch
# (applied to a scratch copy by scripts/build_variant.sh); A/B switches that had been decided were deleted. What is left to switch:
_ALLOWED_ENV = {
    # forms of the solvers the test-suite runs side by side
    "CC_INTR_PERSIST", "CC_INTR_PERSIST_TEAMS", "CC_SWEEP_TILES", "CC_RIG_PERSIST", "CC_RIG_FORCE_BIG", "CC_RIG_SWEEP_FRAME",
    "CC_RIG_SWEEP_WG_WAVES", "CC_RIG_FRAME_WAVES", "CC_RIG_K_COMPACT",
    # test hooks of the persistent forms and of the per-device back-off
    "CC_INTR_PERSIST_TEST_NO_CONTROL", "CC_RIG_PERSIST_TEST_NO_CONTROL", "CC_PERSIST_BACKOFF_CALLS", "CC_PERSIST_BACKOFF_MS",
    # a user's business: launches of several processes / shards that share one device; host-side phase times to stderr
    "CC_INTR_CO_RESIDENT", "CC_RIG_CO_RESIDENT", "CC_RIG_HOST_TIMING",
}
_ALLOWED_IFDEF = {"CC_HAVE_EIGEN", "CC_FORCE_MINI_EIGEN", "__has_include", "Eigen", "Dense", "__HIPCC__"}   # (types.hh: real Eigen when the include path has it)


def _product_sources():
    d = os.path.join(ROOT, "camera_calibrator_amd", "csrc")
    for n in sorted(os.listdir(d)):
        if n.endswith((".hip", ".hpp", ".cpp", ".hh")):
            yield n, open(os.path.join(d, n)).read()


def test_no_timing_or_ablation_text_in_the_product_sources():
    banned = re.compile(r"CC_\w*TIMING(?<!CC_RIG_HOST_TIMING)\b|CC_ABLATE\w*|CC_\w*EXACT_\w+|CC_PERSIST_PROBE\w*|\b[A-Z0-9]+_MARK\(|\bK2_T\(")
    hits = [(n, m.group(0)) for n, text in _product_sources() for m in banned.finditer(text)]
    assert not hits, hits
    for p in ("timing.patch", "exact_arith.patch"):
        assert os.path.exists(os.path.join(ROOT, "scripts", "variants", p)), p


def test_only_the_listed_switches_are_left():
    envs, conds = set(), set()
    for n, text in _product_sources():
        envs |= set(re.findall(r'getenv\("(\w+)"\)', text))
        envs |= set(re.findall(r'persist_test_drop_control\("(\w+)"', text))
        for m in re.finditer(r"^\s*#\s*(?:ifdef|ifndef|if|elif)\s+(.*)$", text, flags=re.M):
            conds |= set(re.findall(r"[A-Za-z_]\w*", m.group(1))) - {"defined"}
    assert envs <= _ALLOWED_ENV, sorted(envs - _ALLOWED_ENV)
    assert conds <= _ALLOWED_IFDEF, sorted(conds - _ALLOWED_IFDEF)


@pytest.mark.parametrize("name", ["timing", "exact_arith"])
def test_variant_patches_still_apply_to_the_product_sources(name, tmp_path):
    """scripts/variants/*.patch carry the text that left the product sources; an edit of a patched region must regenerate them
    (scripts/build_variant.sh says how) -- a patch that no longer applies fails HERE, not on the GPU box in the middle of a measurement."""
    import shutil
    src = os.path.join(ROOT, "camera_calibrator_amd", "csrc")
    dst = tmp_path / "csrc"
    dst.mkdir()
    for n in os.listdir(src):
        if n.endswith((".hip", ".hpp", ".cpp", ".hh")):
            shutil.copy(os.path.join(src, n), dst / n)
    r = subprocess.run(["patch", "-p0", "--dry-run", "-F", "0", "-i", os.path.join(ROOT, "scripts", "variants", name + ".patch")],
                       cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0 and "FAILED" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
