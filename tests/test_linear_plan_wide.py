"""The wide plan of a decode step of 17..64 rows (LinearEnv::wide_rows, zonos_amd/csrc/zn_linear_plan.h): up to 64 activation rows per
weight pass instead of groups of 16.  tests/linear_plan_wide_check.cpp walks plan_linear over tests/linear_plan_check.cpp's grid of tune values,
workspaces, shapes and hand-overs, with the FP8 offer on and off:
  - wide on at 16 rows or fewer, or in prefill: every plan equals the wide-off plan field for field;
  - wide on, decode, rows in {17, 24, 32, 33, 48, 64}: everything that fixes an output bit (kernel family, ksplit, lnp, w8, ln_pro, ln_launch,
    reads / writes of the LayerNorm statistics, and the nwv that orders the tile statistics) is the 16-row plan's; row_tiles = ceil(min(rows, 64) / 16)
    and rows_per_launch = 64 where a wide form exists (gemm16k_kernel's row groups except under the Mamba2 epilogue; the LDS-staged kernel for
    none x residual and {none, LayerNorm} x SiLU gate), 1 and 16 elsewhere; the wide grid covers the weight rows; the partial tiles fit the
    workspace or the plan fell back to groups of 16 (the 1 MiB workspace must show that at least once); LayerNorm is applied exactly once; fc1
    reads statistics only if out_proj writes them;
  - the plans at the production shapes at 32 and 64 rows, bf16 and FP8, are pinned as strings.
The second test reads the shipped code object's metadata: every gemm16w_kernel instantiation (fc1 and fc2, bf16 and FP8, 2 .. 4 row blocks) and
the statistics LayerNorm launch use no scratch, do not spill, and stay inside a CU's 160 KB of LDS."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def test_wide_plans_keep_the_16_row_arithmetic_and_are_pinned(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "linear_plan_wide_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "zonos_amd", "csrc"),
                    os.path.join(ROOT, "tests", "linear_plan_wide_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and r.stdout.rstrip().endswith("OK")


def test_wide_kernels_use_no_scratch_and_fit_the_lds(tmp_path):
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
            if name.startswith("_Z14gemm16w_kernel") or name.startswith("_Z20ln_from_stats_kernel"):
                g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, k).group(1))
                seen[name] = dict(scratch=g("private_segment_fixed_size"), spill=g("vgpr_spill_count"), vgpr=g("vgpr_count"), lds=g("group_segment_fixed_size"),
                                  threads=g("max_flat_workgroup_size"))
    wide = sorted(n for n in seen if "gemm16w" in n)
    # <EPI_RESID | EPI_SILU, bf16 | FP8, 2 | 3 | 4 row blocks>: what production launches, nothing else
    assert wide == sorted(f"_Z14gemm16w_kernelILi{epi}ELb{w8}ELi{rb}EEv8GemvArgs" for epi in (1, 2) for w8 in (0, 1) for rb in (2, 3, 4)), wide
    assert sum("ln_from_stats" in n for n in seen) == 2, sorted(seen)
    for name, r in seen.items():
        print(name, r)
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)
        assert r["lds"] <= 160 * 1024, (name, r)
        assert (r["threads"] // 64) * r["vgpr"] <= 4 * 512, (name, r)
    rb4 = seen["_Z14gemm16w_kernelILi1ELb0ELi4EEv8GemvArgs"]
    assert 2 * 64 * 264 * 2 <= rb4["lds"] <= 2 * 64 * 264 * 2 + 64, rb4          # Ws + Xs (the output tile reuses Ws) and the ticket flag
