"""A generation's host rules (zonos_amd/csrc/zn_gen_state.h) answer what the entry points of zn_api.hip answered before the header existed.
tests/gen_state_check.cpp holds, as typed-in literals, the return code and the whole message of every refusal, and asserts on the CPU:
  - call order: each of the 15 entry points of the table against no generation, a generation begun, with a row table, with prefix shifts, prefilled, a session
    opened, a session with a busy slot, an ended generation - accepted, or ZN_ERR_STATE with the full message (zn_sample_first accepts an ended generation);
  - request rules: every refusal tests/test_gpu_requests.py, test_gpu_prefix_rows.py, test_gpu_ragged.py, test_gpu_serve.py and test_gpu_mixed.py provoke, and the
    accepting neighbour of each bound (windows 0 / 64 against -1 / 65, max_new_tokens 1 / the budget against 0 / budget + 1, prefixes 0 / p_call, rows of 1 / S
    positions, an admission that meets max_len and the code buffer's width exactly against one more, max_new_tokens = INT32_MAX without a signed overflow), pairs
    in either order and rows apart, each of pair_partner's six reasons;
  - derived values: rem, shift, any, uniform, rows_unequal2;
  - slots: admit, steps, retire, admit - len_hi is the longest busy slot after every call, zn_decode_steps refuses exactly at slot_len + n > max_len;
  - eligibility for the persistent kernels: one of the 32 combinations of the five flags;
  - reset: begin() on a record with every field changed equals a fresh record with the same arguments.
The refusals the program prints ("label | code | message") are then compared, sorted, with profiles/gen_state_refusals_parent.txt: what the parent commit's library
answered to the same calls on an MI355X.  The program runs twice: optimised, and under AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program: nothing is preloaded)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gen_state_answers_what_the_entry_points_answered(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    listings = []
    for name, flags in (("gen_state_check", ["-O2"]), ("gen_state_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp_path / name
        subprocess.run([gxx, "-std=c++17", *flags, "-Wall", "-I", os.path.join(ROOT, "zonos_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "gen_state_check.cpp"), "-o", str(exe)], check=True)
        r = subprocess.run([str(exe)], capture_output=True, text=True)
        print(r.stdout)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "FAIL" not in r.stdout and r.stdout.rstrip().endswith("OK")
        listings.append(sorted(line for line in r.stdout.splitlines() if " | " in line))
    # the literals are the parent's: every refusal the program printed is the line the library of the parent commit answered on an MI355X
    # (tools/gen_refusals.py).  On that tool's handle zn_set_mlp_fp8 and zn_set_mamba_fp8 refuse its widths before they ask about the generation.
    apart = ("order: zn_set_mlp_fp8,", "order: zn_set_mamba_fp8,")
    with open(os.path.join(ROOT, "profiles", "gen_state_refusals_parent.txt")) as f:
        parent = sorted(line.rstrip("\n") for line in f if not line.startswith(apart))
    assert len(parent) == 137 and listings[0] == listings[1]
    assert [line for line in listings[0] if not line.startswith(apart)] == parent
