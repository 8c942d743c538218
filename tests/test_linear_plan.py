"""Which kernel serves a linear of 1..64 rows is a value: plan_linear (zonos_amd/csrc/zn_linear_plan.h) returns a LinearPlan, and the launchers
of zn_api.hip only follow it.  The header has no HIP in it, so tests/linear_plan_check.cpp walks the very function the library calls: rows 1..16,
17, 24, 64 x every prologue x every epilogue x every combination of the tune values a decision reads (ZN_TUNE_SMALL_M_LDS,
ZN_TUNE_NO_SPLIT_SMALL_M, ZN_TUNE_FC1_LN_LAUNCH, ZN_TUNE_NO_PREFILL_GEMM16K; ZN_TUNE_GEMM16K_MAX_TILES 0 / 64 / 200) x decode and prefill x the
(N, K) of test_small_m_linear_shapes_vs_fp32_reference plus fc1's.  Every plan names a kernel launch_linear holds an instantiation of (the
header's own table, which the launcher's `if constexpr` guards read too) or carries an error; fc1 reads LayerNorm statistics only when the
out_proj plan made under the same settings writes them, and those are written only by gemm16k_kernel<EPI_RESID> at N = 16 * ZN_G16_LNT; split-K
plans fit the partial-tile buffer and the ticket array; GEMV grids cover their units and are mask-free only when exact; the tiled GEMM is planned
only for K a multiple of its 32-wide fragments ((200, 136) is in the walk for that).

The last check pins the plans at the production shapes (in_proj, out_proj, fc1, fc2, heads at 2, 4, 6, 16 rows and a 48-row prefill, default
settings).  The table was written down after the ordered kernel launch list (name, grid, workgroup size) of generations at those row counts and
of a short and a long prefill had been compared between this dispatch and the launch-while-deciding functions it replaced, and found identical
(profiles/linear_plan_launch_trace_*.txt)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_linear_plans_are_launchable_consistent_and_pinned(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "linear_plan_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "zonos_amd", "csrc"),
                    os.path.join(ROOT, "tests", "linear_plan_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and r.stdout.rstrip().endswith("OK")
