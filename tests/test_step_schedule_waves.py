"""The static tile schedules of the whole-step kernels built with six compute waves per streaming workgroup (-DZN_SK_CW=6), replayed on the
CPU like the shipped ones (tests/test_step_schedule.py), and the cover of the fullest streaming workgroup's share of every matrix by the
T_* of both wave counts at the Zonos-v0.1 shapes (the inequalities of zn_api.hip's stack_variant_ok)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_six_wave_schedules_replay_without_hazards_and_cover_the_shares(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "step_schedule_waves_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-I", os.path.join(ROOT, "zonos_amd", "csrc"), "-I", os.path.join(ROOT, "tests"),
                    os.path.join(ROOT, "tests", "step_schedule_waves_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and r.stdout.count("\n") == 9
