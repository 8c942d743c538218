"""The FP8 offer for the Mamba2 projections as a plan decision (LinearEnv::w8k_offered, zonos_amd/csrc/zn_linear_plan.h).
tests/linear_plan_mamba_fp8_check.cpp walks plan_linear over rows 1 .. 80, the tune values, workspaces and max-tile settings the sibling walks use,
w8_offered and wide_rows off and on, wide_hybrid 0 .. 4 where it is read, every prologue and epilogue, decode and prefill, and the production (N, K)
pairs of both stacks (plus shapes off the kernels' grids):
  - under w8k_offered every plan equals the un-offered plan in every field but w8 (kernel, row_tiles, row_loop, grid, ...);
  - w8 is set exactly for decode GEMM16K plans with no prologue and either the Mamba2 epilogue at nch 2 or store at nch 4 - never for prefill, for
    rows <= 4, or for the RoPE / residual / fp32 epilogues;
  - every plan is linear_plan_launchable, and a w8 flag forced onto a GEMM16K plan without an FP8 instantiation is not;
  - w8_offered alone still leaves every GEMM16K plan unmarked;
  - at the production shapes and default settings the Mamba2 in_proj (N = 8512, 8384) and out_proj read the stream at every row count from 5 to 80.
The second test reads the shipped code object's metadata: the three FP8 kernels exist under names of their own, use no scratch and do not spill."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
KERNELS = {
    "_Z15gemm16k8_kernelILi5ELi2EEv8GemvArgs": "in_proj, 16 rows per workgroup (EPI_MAMBA, NCH 2)",
    "_Z15gemm16k8_kernelILi0ELi4EEv8GemvArgs": "out_proj, 16 rows per workgroup and row groups on grid y (EPI_STORE, NCH 4)",
    "_Z20gemm16k8_rows_kernelILi2EEv8GemvArgs": "in_proj, the row-tile loop (NCH 2)",
}


def test_mamba_fp8_offer_marks_only_the_two_projections(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "linear_plan_mamba_fp8_check"
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "zonos_amd", "csrc"),
                    os.path.join(ROOT, "tests", "linear_plan_mamba_fp8_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and r.stdout.rstrip().endswith("OK")


def test_mamba_fp8_kernels_exist_and_use_no_scratch(tmp_path):
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
            if "gemm16k8" in name:
                g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, k).group(1))
                seen[name] = dict(scratch=g("private_segment_fixed_size"), spill=g("vgpr_spill_count"), sgpr_spill=g("sgpr_spill_count"), vgpr=g("vgpr_count"),
                                  lds=g("group_segment_fixed_size"), threads=g("max_flat_workgroup_size"))
    assert sorted(seen) == sorted(KERNELS), sorted(seen)
    for name, r in seen.items():
        print(name, KERNELS[name], r)
        assert r["scratch"] == 0 and r["spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        # eight waves per workgroup: the bars tests/test_linear_plan_hybrid_wide.py holds the bf16 row-tile loop to
        assert r["threads"] == 512 and (r["threads"] // 64) * r["vgpr"] <= 4 * 512, (name, r)
        assert r["lds"] <= 160 * 1024, (name, r)
