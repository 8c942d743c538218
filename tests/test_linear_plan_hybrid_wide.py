"""The wide forms of the Mamba2 in_proj in a decode step of 17..64 rows (LinearEnv::wide_hybrid, zonos_amd/csrc/zn_linear_plan.h).
tests/linear_plan_hybrid_wide_check.cpp walks plan_linear over tests/linear_plan_wide_check.cpp's grid of tune values, workspaces, shapes, prologues,
epilogues and row counts (plus the two Mamba2 in_proj shapes, K = 4096 under the Mamba2 epilogue, and 80 rows), with wide_rows off and on:
  - wide_hybrid = 0 (the default every other walk constructs) or 1, wide_rows off, prefill, 16 rows or fewer: every plan equals the plan of an env
    without the field, field for field;
  - wide_hybrid = 2, 3 or 4 (the tune key unset: wide_hybrid_form picks per row count): the only plans that differ are decode plans of more than 16
    rows with kernel == GEMM16K and epi == EPI_MAMBA; they differ only in rows_per_launch (64), row_tiles (ceil(min(rows, 64) / 16)) and row_loop;
    every one of them is linear_plan_launchable; row_loop is set exactly where the form is 3 and the instantiation exists (no prologue, K = 2048);
  - the production plans of the Mamba2 in_proj (no prologue, EPI_MAMBA, N = 8512 and 8384, K = 2048) at 17, 32, 64 and 80 rows are pinned as strings
    for every value of the field, and the Mamba2 out_proj (no prologue, store, 2048 x 4096) is wide with and without it.
The second test reads the shipped code object's metadata: gemm16k_rows_kernel<2> exists (and no other instantiation), uses no scratch, does not
spill, and eight waves of it fit the register file four times over per CU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def test_hybrid_wide_plans_change_only_the_mamba_in_proj_and_are_pinned(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "linear_plan_hybrid_wide_check"
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "zonos_amd", "csrc"),
                    os.path.join(ROOT, "tests", "linear_plan_hybrid_wide_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and r.stdout.rstrip().endswith("OK")


def test_row_tile_loop_kernel_exists_and_uses_no_scratch(tmp_path):
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
            if "gemm16k_rows_kernel" in name:
                g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, k).group(1))
                seen[name] = dict(scratch=g("private_segment_fixed_size"), spill=g("vgpr_spill_count"), vgpr=g("vgpr_count"), lds=g("group_segment_fixed_size"),
                                  threads=g("max_flat_workgroup_size"))
    # <NCH = 2>: the Mamba2 in_proj at K = 2048, what production launches, nothing else
    assert sorted(seen) == ["_Z19gemm16k_rows_kernelILi2EEv8GemvArgs"], sorted(seen)
    for name, r in seen.items():
        print(name, r)
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)
        assert r["threads"] == 512 and (r["threads"] // 64) * r["vgpr"] <= 4 * 512, (name, r)
        assert r["lds"] <= 160 * 1024, (name, r)
