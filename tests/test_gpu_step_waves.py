"""The whole-step decode kernels (csrc/zn_step_kernel.h) divide a streaming workgroup's tiles among ZN_SK_CW compute waves (4, or 6 with
-DZN_SK_CW=6: no helper waves, the compute waves contract the pre-block and stage the LayerNorm parameters, fc2's input reaches them through
LDS).  Which wave contracts a tile does not enter the arithmetic, so whatever the count the kernels must reproduce the launches path
(zn_debug_tune(ZN_TUNE_PERSISTENT, 2)) and the per-block chain path (zn_debug_tune(ZN_TUNE_WHOLE_STEP, 2)) bit for bit: codes and the logits of
every step.  A few decode steps at each place where the static schedule changes: one key block (pre-block, first graph), across 512 keys
(the streaming-workgroup count changes mid-run), the second and third instantiation (7 and 9 key blocks), the one-row kernel, and the
form with block 0's in_proj as a launch of its own (ZN_TUNE_STACK_PRE = 2).  A hand-off timeout is an error."""
import pytest
import torch

from zonos_amd import _lib, synth
from zonos_amd.testing import build_model

pytestmark = pytest.mark.gpu
GREEDY = {"temperature": 0.0}
SEED = 1234
WS, PE, PRE = _lib.ZN_TUNE_WHOLE_STEP, _lib.ZN_TUNE_PERSISTENT, _lib.ZN_TUNE_STACK_PRE


@pytest.fixture(scope="module")
def full():
    model, _ = build_model(synth.FULL_CFG, SEED, "cuda:0")
    return model


def _traced(model, cond, pre, new, cfg_scale):
    tr = {"logits": []}
    o = model.generate(cond, audio_prefix_codes=pre, max_new_tokens=new, cfg_scale=cfg_scale, sampling_params=GREEDY, _trace=tr)
    return o.cpu(), torch.stack(tr["logits"]).cpu()


def _case(model, rows, prefix, new, stack_pre=1):
    """Contexts 24 + prefix + 1 ... + new.  rows = 2: guided (step_kernel); rows = 1: cfg_scale = 1 (step_r1_kernel; the per-block chain serves
    two rows only, so the one-row run is compared with the launches path alone)."""
    eng = model.engine(1)
    c = synth.conditioning(SEED, "cond", 1, 24, 2048).to("cuda:0")
    cond, scale = (torch.cat([c, c], 0), 2.0) if rows == 2 else (c, 1.0)
    pre = torch.from_numpy(synth.randint(SEED, f"waves.prefix{prefix}", (1, 9, prefix), 1024)).to("cuda:0") if prefix else None
    try:
        eng.call("zn_debug_eos_bias", float("-inf"))
        eng.call("zn_debug_tune", PRE, stack_pre)
        t0 = eng.counters()["handoff_timeouts"]
        o1, l1 = _traced(model, cond, pre, new, scale)                          # single-step launches
        assert eng.lib.zn_decode_path_detail(eng.h) == 2, "the whole-step kernel did not serve this configuration"
        og = model.generate(cond, audio_prefix_codes=pre, max_new_tokens=new, cfg_scale=scale, sampling_params=GREEDY).cpu()      # 8-step graphs
        assert eng.lib.zn_decode_path_detail(eng.h) == 2
        assert o1.shape[-1] == prefix + new and torch.equal(og, o1)
        others = [("launches", {PE: 2}, 0)] + ([("chain", {WS: 2}, 1)] if rows == 2 else [])
        for name, tune, detail in others:
            for k, v in tune.items():
                eng.call("zn_debug_tune", k, v)
            o, l = _traced(model, cond, pre, new, scale)
            assert eng.lib.zn_decode_path_detail(eng.h) == detail, (name, eng.lib.zn_decode_path_detail(eng.h))
            for k in tune:
                eng.call("zn_debug_tune", k, 1)
            assert torch.equal(o, o1), name
            assert l.shape == l1.shape and torch.equal(l.view(torch.int32), l1.view(torch.int32)), name
        assert eng.counters()["handoff_timeouts"] == t0 == 0
    finally:
        for k in (WS, PE, PRE):
            eng.call("zn_debug_tune", k, 1)
        eng.call("zn_debug_eos_bias", 0.0)


@pytest.mark.parametrize("prefix,new", [(5, 16), (480, 16), (3050, 8), (4074, 8)], ids=["30-46", "505-521", "7-blocks", "9-blocks"])
def test_guided_whole_step_kernel_is_bit_identical(full, prefix, new):
    """One key block; 1 -> 2 key blocks mid-run; just past 3072 keys (second static schedule); just past 4096 keys (third)."""
    _case(full, 2, prefix, new)


@pytest.mark.parametrize("prefix,new", [(5, 16), (480, 16)], ids=["30-46", "505-521"])
def test_one_row_whole_step_kernel_is_bit_identical(full, prefix, new):
    _case(full, 1, prefix, new)


def test_guided_whole_step_kernel_behind_an_in_proj_launch_is_bit_identical(full):
    """ZN_TUNE_STACK_PRE = 2: block 0's in_proj is a launch of its own, the kernel starts without the pre-block."""
    _case(full, 2, 5, 16, stack_pre=2)
