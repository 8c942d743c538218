"""tests/step_ring_depth_check.cpp: for every register-fed slot of the shipped whole-step and chain schedules, the number of later tile
requests of the same wave that are outstanding when the slot is contracted.  With ZN_SK_NBUF = ZN_CH_NBUF = 3 register buffers a wave
runs two requests ahead inside an op; the deferral (requests for another op's tiles wait for the publish, but for the first ZN_SK_EARLY = 1
of an op) lets the ring of the whole-step kernels run down to 1 at the end of an op, the chain's (no early request) to 0.  tests/test_step_ring_isa.py holds the built kernels' waits against these figures."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ring_depths_of_the_shipped_schedules(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "step_ring_depth_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "zonos_amd", "csrc"), "-I", os.path.join(ROOT, "tests"), "-Wno-unused-function",
                    os.path.join(ROOT, "tests", "step_ring_depth_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout + r.stderr
    got = {line.split(": ")[0]: [int(t.split(":")[1]) for t in line.split(": ")[1].split()] for line in r.stdout.splitlines() if not line.startswith("replay")}
    assert len(got) == 9
    for name, d in got.items():
        assert max(d) == 2 and d[-1] == 0, (name, d)              # never more than NBUF - 1 ahead; nothing behind a block's last tile
    # step_kernel<4,1,7,4,4,6>: 6 + 4 + 4 register-fed tiles (fc1's first is parked); one early request per op keeps a tile behind an op's last
    assert got["step<4,1,7,4,4,6>"] == [2, 2, 2, 2, 2, 1, 2, 2, 2, 1, 2, 2, 1, 0]
    # chain_kernel: op 0 has one request behind it, op 1 re-reads op 0's buffers with two
    assert got["chain<4,1,8,4,5>"][:2] == [1, 2]
