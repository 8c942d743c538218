"""The compute waves' register ring of the persistent decode kernels is as deep in the built code as the static schedule says.

A compute wave requests a weight tile (two rows, 2 NCH `global_load_dwordx4 ... nt`) ZN_SK_NBUF / ZN_CH_NBUF tiles ahead of its
contraction.  The compiler turns "this buffer has landed" into `s_waitcnt vmcnt(N)`: N younger loads may still be outstanding.  While
the loads of a tile stood under a wave-uniform `if (tile exists)`, the path that skipped them joined the path that issued them, and on
the skipping path the PREVIOUS tile's loads are the youngest - so every wait for an older buffer was vmcnt(0 .. 7): contracting tile k
drained the requests for k + 1 and k + 2.  In the parent of the change that added this file, no wait of step_kernel, step_r1_kernel or
chain_kernel had 16 <= vmcnt <= 62 (one vmcnt(63) in front of a barrier; the histogram of step_kernel<4,1,7,4,4,6> was vmcnt(0) x 97,
(1) x 41, (5) x 24, (4) x 22, (7) x 23, then 15 and below).  The requests are now unconditional in control flow (an absent tile reads a
dummy address without the lane offset and is never contracted), and this test disassembles the built library to hold that:

  * per kernel, the last vmcnt wait before the last `v_dot2c_f32_bf16` of each register-fed tile is at least (loads per tile) x (later
    requests the schedule has outstanding at that slot, tests/step_ring_depth_check.cpp).  Loads per tile is 2 NCH: 8 at d_model 2048,
    2 in the three d_model 512 chain instantiations.  A "tile" in the disassembly is a straight-line stretch (no branch, no barrier) with
    exactly one tile's dot products.  The compiler lays the unrolled slots out in an order of its own, so the two lists are compared
    SORTED: the k-th largest wait covers the k-th largest figure.  That is weaker than slot by slot - a shallow slot could hide behind a
    deep one of another op - but the number of deep waits is held.  Stretches that wait for no load at all (tiles parked in LDS; the
    pre-block's tiles wait vmcnt(0) and sort last) are not compared at d_model 2048, where there are at least as many waiting stretches
    as register-fed slots;
  * at d_model 512 a tile is two loads and an op one or two tiles, so some register-fed tiles have been retired by a wait that stands
    between the stretches and their own stretch has none: such a stretch drains nothing and counts as covering any figure.  To keep
    that from hiding a drained ring, the kernel must also have at least four waits with 4 <= vmcnt <= 62.  The parent's three kernels
    have 2, 1 and 2 (histograms (0) x 20, (1) x 13, (2) x 4, (3) x 2, (4) x 2 and alike) and waits of 1 and 0 in their stretches: both
    assertions fail on the parent's library; the fixed kernels have 12, 6 and 9;
  * each d_model 2048 kernel has a wait with 16 <= vmcnt <= 62 - the parent had none;
  * the weight loads are still `global_load_dwordx4` with `nt`, one site per request of the schedule;
  * no more `flat_load` than the parent's one per kernel.
"""
import os
import re
import shutil
import subprocess

import pytest

from zonos_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
ENDS_BLOCK = ("s_cbranch", "s_branch", "s_barrier", "s_endpgm", "s_setpc")

# kernel symbol prefix -> (depth-check line, NCH, activation rows, requests per block, fc2 slots left out)
#   fc2 slots left out: in chain_kernel the wave sweeps fc2's input from the hand-off granules itself, and loads return in order, so the
#   sweep's own wait has retired the first min(T_FC2, ZN_CH_NBUF) tiles of fc2, requested before it: their stretches need no wait.
KERNELS = {
    "_Z11step_kernelILi4ELi1ELi7ELi4ELi4ELi6EE": ("step<4,1,7,4,4,6>", 4, 2, 16, 0),
    "_Z11step_kernelILi4ELi1ELi8ELi4ELi5ELi8EE": ("step<4,1,8,4,5,8>", 4, 2, 18, 0),
    "_Z11step_kernelILi4ELi2ELi9ELi5ELi5ELi12EE": ("step<4,2,9,5,5,12>", 4, 2, 21, 0),
    "_Z14step_r1_kernelILi4ELi1ELi7ELi4ELi4ELi6EE": ("step<4,1,7,4,4,6>", 4, 1, 16, 0),
    "_Z14step_r1_kernelILi4ELi1ELi8ELi4ELi5ELi8EE": ("step<4,1,8,4,5,8>", 4, 1, 18, 0),
    "_Z14step_r1_kernelILi4ELi2ELi9ELi5ELi5ELi12EE": ("step<4,2,9,5,5,12>", 4, 1, 21, 0),
    "_Z12chain_kernelILi4ELi1ELi8ELi4ELi5EE": ("chain<4,1,8,4,5>", 4, 2, 18, 3),
    "_Z12chain_kernelILi4ELi1ELi8ELi4ELi0EE": ("chain<4,1,8,4,0>", 4, 2, 13, 3),
    "_Z12chain_kernelILi4ELi1ELi8ELi4ELi2EE": ("chain<4,1,8,4,2>", 4, 2, 15, 3),
    "_Z12chain_kernelILi1ELi1ELi2ELi1ELi5EE": ("chain<1,1,2,1,5>", 1, 2, 9, 1),
    "_Z12chain_kernelILi1ELi1ELi2ELi1ELi0EE": ("chain<1,1,2,1,0>", 1, 2, 4, 1),
    "_Z12chain_kernelILi1ELi1ELi2ELi1ELi1EE": ("chain<1,1,2,1,1>", 1, 2, 5, 1),
}


@pytest.fixture(scope="module")
def depths(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("ring") / "step_ring_depth_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "zonos_amd", "csrc"), "-I", os.path.join(ROOT, "tests"), "-Wno-unused-function",
                    os.path.join(ROOT, "tests", "step_ring_depth_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout + r.stderr
    # "name: op:depth op:depth ..." -> name -> [(op, depth)]
    return {line.split(": ")[0]: [tuple(int(v) for v in t.split(":")) for t in line.split(": ")[1].split()] for line in r.stdout.splitlines() if not line.startswith("replay")}


@pytest.fixture(scope="module")
def kernels_isa(tmp_path_factory):
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    from zonos_amd import build
    build.build(verbose=False)
    tmp = tmp_path_factory.mktemp("isa")
    so = shutil.copy(_lib.LIB_PATH, tmp / "lib.so")
    subprocess.run([OBJDUMP, "--offloading", str(so)], check=True, capture_output=True, cwd=tmp)       # writes the bundles next to the copy
    out = {}
    for co in sorted(tmp.glob("lib.so.*gfx950*")):
        txt = subprocess.run([OBJDUMP, "-d", str(co)], check=True, capture_output=True, text=True).stdout
        name = None
        for line in txt.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
            if m:
                name = m.group(1)
                out[name] = []
            elif name and line.strip():
                out[name].append(line.split("//")[0].strip())
    assert out, "no gfx950 code object found in the library"
    return out


def _vmcnts(ins):
    return [int(v) for l in ins if l.startswith("s_waitcnt") for v in re.findall(r"vmcnt\((\d+)\)", l)]


def _tile_waits(ins, dots_per_tile):
    """Last vmcnt wait in front of the last dot product of every straight-line stretch that contracts exactly one tile; None where the
    stretch waits for no load at all (a tile parked in LDS, or one that an earlier wait has retired)."""
    blocks, cur = [], []
    for l in ins:
        cur.append(l)
        if l.startswith(ENDS_BLOCK):
            blocks.append(cur)
            cur = []
    blocks.append(cur)
    out = []
    for b in blocks:
        dots = [i for i, l in enumerate(b) if l.startswith("v_dot2c_f32_bf16")]
        if len(dots) != dots_per_tile:
            continue
        w = _vmcnts(b[:dots[-1]])
        out.append(w[-1] if w else None)
    return out


@pytest.mark.parametrize("prefix", sorted(KERNELS))
def test_register_fed_tiles_wait_with_the_schedules_depth(kernels_isa, depths, prefix):
    line, nch, rows, n_req, swept = KERNELS[prefix]
    names = [n for n in kernels_isa if n.startswith(prefix)]
    assert len(names) == 1, names
    ins = kernels_isa[names[0]]
    per_tile = 2 * nch                                            # loads of a request: two weight rows, NCH chunks of 16 bytes per lane
    sched = depths[line]
    fc2 = [i for i, (op, _) in enumerate(sched) if op == 3][:swept]
    assert len(fc2) == swept
    want = sorted((per_tile * d for i, (_, d) in enumerate(sched) if i not in fc2), reverse=True)
    waits = _tile_waits(ins, 2 * nch * rows * 4)                  # two rows x NCH chunks x activation rows x four dot2 per 16 bytes
    got = sorted((w for w in waits if w is not None), reverse=True)
    if nch == 1:
        got = [99] * waits.count(None) + got                      # d_model 512: a stretch without a wait counts as one that drains nothing (docstring)
    print(names[0], "schedule:", want, "built:", got, "stretches without a wait:", waits.count(None))
    assert len(got) >= len(want), f"{names[0]}: {len(got)} single-tile stretches that wait for loads, the schedule has {len(want)} register-fed slots"
    for k, (g, w) in enumerate(zip(got, want)):
        assert g >= w, f"{names[0]}: the {k}-th deepest tile waits vmcnt({g}), the schedule has {w} later loads outstanding"
    deep = [v for v in _vmcnts(ins) if 2 * per_tile <= v <= 62]
    assert len(deep) >= (1 if nch > 1 else 4), f"{names[0]}: {len(deep)} waits leave two requested tiles in flight"
    nt = [l for l in ins if l.startswith("global_load_dwordx4") and re.search(r"\bnt\b", l)]
    pre_tiles = 2 if line.startswith("step") else 0
    assert len(nt) == per_tile * (n_req + pre_tiles), (len(nt), per_tile * (n_req + pre_tiles))
    assert sum(1 for l in ins if l.startswith("flat_load")) <= 1
