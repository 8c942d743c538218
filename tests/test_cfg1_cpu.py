"""Generation without guidance (cfg_scale == 1) - the parts that need no GPU.

* The identity the GPU tests of tests/test_gpu_cfg1.py stand on: a guided run whose unconditional rows equal its conditional rows
  gives exactly the conditional logits (u + (c - u) s == u when c == u bit for bit), so the unchanged oracle on [c ‖ c] at
  cfg_scale=2 is a reference for the unguided path on [c].
* The one-row whole-step kernel (step_r1_kernel, zn_step_kernel.h) in the shipped code object, checked the way tests/test_abi.py
  checks step_kernel: no scratch, no spills, one workgroup per CU, granule hand-offs with write-through stores and sc1 loads.
* generate()'s row checks at cfg_scale == 1."""
import os
import re
import shutil
import subprocess

import pytest
import torch

from oracle import zonos_oracle as zo
from zonos_amd import _lib, synth

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
R1 = "_Z14step_r1_kernel"


def test_guided_logits_on_equal_rows_are_the_conditional_logits():
    cfg = synth.TINY_CFG
    w = synth.zonos_state_dict(cfg, 77)
    c = synth.conditioning(77, "cfg1.cond", 1, 9, cfg["d_model"])
    for scale in (2.0, 3.5):
        both = zo.compute_logits(w, torch.cat([c, c], 0), zo.setup_cache(cfg, 2, 16), cfg, scale)
        one = zo.compute_logits(w, c, zo.setup_cache(cfg, 1, 16), cfg, 1.0)
        assert both.shape == one.shape == (1, 9, 1025)
        assert torch.equal(both, one), scale


def _lib_path():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    return _lib.LIB_PATH


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    if not (os.path.exists(OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("llvm tools not available")
    tmp = tmp_path_factory.mktemp("cfg1_isa")
    so = shutil.copy(_lib_path(), tmp / "lib.so")
    subprocess.run([OBJDUMP, "--offloading", str(so)], check=True, capture_output=True, cwd=tmp)
    return sorted(tmp.glob("lib.so.*gfx950*"))


@pytest.fixture(scope="module")
def r1_isa(code_objects):
    out = {}
    for co in code_objects:
        txt = subprocess.run([OBJDUMP, "-d", str(co)], check=True, capture_output=True, text=True).stdout
        name = None
        for line in txt.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
            if m:
                name = m.group(1)
                if name.startswith(R1):
                    out[name] = []
            elif name in out and line.strip():
                out[name].append(line.split("//")[0].strip())
    return out


def test_one_row_kernel_uses_no_scratch_and_fits_one_workgroup_per_cu(code_objects):
    seen = {}
    for co in code_objects:
        notes = subprocess.run([READELF, "--notes", str(co)], check=True, capture_output=True, text=True).stdout
        for k in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", k).group(1)
            if name.startswith(R1):
                g = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, k).group(1))
                seen[name] = dict(scratch=g("private_segment_fixed_size"), spill=g("vgpr_spill_count"), vgpr=g("vgpr_count"),
                                  lds=g("group_segment_fixed_size"), threads=g("max_flat_workgroup_size"))
    assert len(seen) == 3, sorted(seen)                  # the whole-step kernel's three static schedules (<= 6 / 8 / 12 key blocks)
    for name, r in seen.items():
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)
        assert (r["threads"] // 64) * r["vgpr"] <= 4 * 512, (name, r)
        assert r["lds"] + 128 * 1024 <= 160 * 1024, (name, r)         # + ZN_SK_DYN_LDS


def test_one_row_kernel_handoffs_are_granules_and_sc1_loads(r1_isa):
    assert len(r1_isa) == 3, sorted(r1_isa)
    for n, ins in r1_isa.items():
        assert not any(l.startswith("scratch_") for l in ins), n
        x4 = [l for l in ins if l.startswith("buffer_load_dwordx4")]
        # the attention workgroups' K / V prefetch (cache rows of earlier launches): plain loads, 16 (K of the block) + 16 (full-width V)
        # per issue site, two sites (kernel start, end of a block) - as in step_kernel; every other 16-byte load is a sweep of handed-off bytes
        plain = [l for l in x4 if " sc1" not in l]
        assert len(plain) == 64, (n, len(plain))
        assert len(x4) - len(plain) >= 20, n
        x2 = [l for l in ins if l.startswith("buffer_load_dwordx2")]
        assert x2 and all(" sc1" in l for l in x2), n                 # e sums of the partials
        granules = [l for l in ins if l.startswith("global_store_dwordx2") and " sc1" in l]
        assert len(granules) >= 3, n
        assert not any(l.startswith("global_atomic_add") and "sc1" in l for l in ins), n


def test_generate_row_checks_without_guidance():
    """cfg_scale == 1 takes exactly batch_size conditional rows: [cond ‖ uncond] still raises AssertionError (the reference's
    assert, model.py:399), other counts ValueError, and B rows pass the checks (here on to the device check: no GPU)."""
    from zonos_amd.testing import build_model
    model, _ = build_model(synth.TINY_CFG, 77, "cpu")
    d = synth.TINY_CFG["d_model"]
    c2 = synth.conditioning(77, "cond", 2, 6, d)
    with pytest.raises(AssertionError):
        model.generate(c2, max_new_tokens=4, cfg_scale=1.0)
    with pytest.raises(ValueError):
        model.generate(synth.conditioning(77, "cond", 3, 6, d), max_new_tokens=4, cfg_scale=1.0, batch_size=2)
    with pytest.raises(ValueError):
        model.generate(c2[:1], max_new_tokens=4, cfg_scale=2.0)
    with pytest.raises(_lib.ZonosHipError, match="MI355X only"):
        model.generate(c2[:1], max_new_tokens=4, cfg_scale=1.0)
    with pytest.raises(_lib.ZonosHipError, match="MI355X only"):
        model.generate(synth.conditioning(77, "cond", 3, 6, d), max_new_tokens=4, cfg_scale=1.0, batch_size=3)
