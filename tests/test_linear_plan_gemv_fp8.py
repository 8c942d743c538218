"""The FP8 offer for the GEMV of 1..4 decode rows as a plan decision (LinearEnv::w8v_offered, zonos_amd/csrc/zn_linear_plan.h).
tests/linear_plan_gemv_fp8_check.cpp walks plan_linear over every tune combination, workspace and max-tile setting of the sibling walks, their shapes and
rows (plus half pairs and masked tails), both existing offers off and on, wide_rows off and on, decode and prefill, every prologue and epilogue:
  - w8v_offered defaults to false, and with it false every plan equals today's in every field;
  - w8_offered and w8k_offered leave every GEMV plan unmarked;
  - with it true every plan equals the un-offered one in every field but w8;
  - w8 becomes true exactly for decode GEMV plans with an instantiation (lin_has_w8v, held to a table written out a second time) - never at rows > 4,
    in prefill or on an error plan;
  - every marked plan is linear_plan_launchable, and a w8 flag forced onto a GEMV plan without an instantiation is not;
  - the production plans at default settings - fc1 16384 x 2048, fc2 2048 x 8192, in_proj 8512 and 8384 x 2048, out_proj 2048 x 4096 with the gated
    prologue and with none - read the stream at 1, 2, 3, 4 rows under the offer, mask-free, and at 5 rows are no GEMV and unchanged.
The second test reads the shipped code object's metadata: the gemv8_kernel instantiations exist under names of their own, use no scratch and do not spill."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
# (NCH, KSPLIT, PRO, EPI) of lin_has_w8v, each for R = 2 / 4, FULL false / true, DEPTH 1 / 2
PROJECTIONS = {(4, 1, 1, 2): "fc1", (4, 4, 0, 1): "fc2", (4, 1, 0, 5): "Mamba2 in_proj", (2, 4, 2, 0): "Mamba2 out_proj, gated norm", (2, 4, 0, 0): "Mamba2 out_proj"}


def test_gemv_fp8_offer_marks_only_the_instantiated_gemv_plans(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "linear_plan_gemv_fp8_check"
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "zonos_amd", "csrc"),
                    os.path.join(ROOT, "tests", "linear_plan_gemv_fp8_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and r.stdout.rstrip().endswith("OK")


def test_gemv_fp8_kernels_exist_and_use_no_scratch(tmp_path):
    from zonos_amd import _lib, build
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("llvm tools not available")
    build.build(verbose=False)
    so = shutil.copy(_lib.LIB_PATH, tmp_path / "lib.so")
    subprocess.run([OBJDUMP, "--offloading", str(so)], check=True, capture_output=True, cwd=tmp_path)
    seen = {}
    for co in sorted(tmp_path.glob("lib.so.*gfx950*")):
        notes = subprocess.run([READELF, "--notes", str(co)], check=True, capture_output=True, text=True).stdout
        for k in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", k).group(1)
            m = re.fullmatch(r"_Z12gemv8_kernelILi(\d)ELi(\d)ELi(\d)ELi(\d)ELi(\d)ELb([01])ELi(\d)EEv8GemvArgs", name)
            if m:
                g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, k).group(1))
                seen[tuple(int(x) for x in m.groups())] = dict(scratch=g("private_segment_fixed_size"), spill=g("vgpr_spill_count"), sgpr_spill=g("sgpr_spill_count"),
                                                                vgpr=g("vgpr_count"), threads=g("max_flat_workgroup_size"))
    want = sorted((R, *p, full, depth) for p in PROJECTIONS for R in (2, 4) for full in (0, 1) for depth in (1, 2))
    assert sorted(seen) == want, sorted(seen)
    for key, r in sorted(seen.items()):
        print(key, PROJECTIONS[key[1:5]], r)
        assert r["scratch"] == 0 and r["spill"] == 0 and r["sgpr_spill"] == 0, (key, r)
        assert r["threads"] == 256 and r["vgpr"] <= 512, (key, r)      # one wave per SIMD: the unified register file of a lane
