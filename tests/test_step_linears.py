"""The decode step's table of linears (zonos_amd/csrc/zn_step_linears.h) computes the plans the call sites of zn_api.hip computed before it existed.
tests/step_linears_check.cpp holds, as typed-in literals, prologue, epilogue, N, K, GEMV target, statistics hand-off and FP8 offer of each of the 13 linears - the
transformer block's in_proj, first out_proj (double_out_proj), out_proj, fc1, fc2 and the heads; the hybrid stack's Mamba2 in_proj and out_proj and its attention
layers' in_proj, out_proj, fc1, fc2 and heads - at the widths of synth.FULL_CFG, CHAIN_CFG, TINY_CFG, HYBRID_FULL_CFG and HYBRID_TINY_CFG, of a hybrid stack with
two norm groups, and of hybrid stacks whose in_proj cannot carry RoPE in its epilogue (half-split rotary; a qkv bias).  It walks rows 1 .. 80, FP8 streams offered
and not, ZN_TUNE_FP8_SMALL_ROWS unset / 2 / 3, ZN_TUNE_WIDE_ROWS unset / 1, ZN_TUNE_WIDE_HYBRID unset / 1 / 2 / 3, ZN_TUNE_FC1_LN_LAUNCH unset / 2, the workspace
present and absent, fc1 with and without statistics handed in, and asserts at every point:
  - plan_step_linear's plan equals plan_linear called with the literals, in every LinearPlan field;
  - the plan has no error and is linear_plan_launchable for the literal (prologue, epilogue) pair;
  - the table's description of the linear is the literal one."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_linears_table_plans_what_the_call_sites_planned(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "step_linears_check"
    subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "zonos_amd", "csrc"),
                    os.path.join(ROOT, "tests", "step_linears_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and r.stdout.rstrip().endswith("OK")
