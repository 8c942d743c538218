"""The one-row whole-step kernel (step_r1_kernel, cfg_scale = 1) in its second and third instantiation - 7 and 9 key blocks, which
tests/test_gpu_step_waves.py reaches with two rows only.  Every instantiation issues the tile requests of its static schedule
unconditionally (an absent tile reads a dummy address and is never contracted), and the workgroups' shares - hence which tiles are absent -
differ with the attention workgroup count, so each is run: a few decode steps just past 3072 and just past 4096 keys must reproduce the
launches path (zn_debug_tune(ZN_TUNE_PERSISTENT, 2)) bit for bit, codes and the logits of every step, without a hand-off timeout.  (The
per-block chain serves two rows only, so the one-row runs have the launches path as their only comparison.)"""
import pytest
import torch

from zonos_amd import _lib, synth
from zonos_amd.testing import build_model

pytestmark = pytest.mark.gpu
GREEDY = {"temperature": 0.0}
SEED = 1234
PE = _lib.ZN_TUNE_PERSISTENT


@pytest.fixture(scope="module")
def full():
    model, _ = build_model(synth.FULL_CFG, SEED, "cuda:0")
    return model


def _traced(model, cond, pre, new):
    tr = {"logits": []}
    o = model.generate(cond, audio_prefix_codes=pre, max_new_tokens=new, cfg_scale=1.0, sampling_params=GREEDY, _trace=tr)
    return o.cpu(), torch.stack(tr["logits"]).cpu()


def _case(model, prefix, new):
    """One row, contexts 24 + prefix + 1 ... + new."""
    eng = model.engine(1)
    cond = synth.conditioning(SEED, "cond", 1, 24, 2048).to("cuda:0")
    pre = torch.from_numpy(synth.randint(SEED, f"ring.prefix{prefix}", (1, 9, prefix), 1024)).to("cuda:0")
    try:
        eng.call("zn_debug_eos_bias", float("-inf"))
        t0 = eng.counters()["handoff_timeouts"]
        o1, l1 = _traced(model, cond, pre, new)                                 # single-step launches of the whole-step kernel
        assert eng.lib.zn_decode_path_detail(eng.h) == 2, "the whole-step kernel did not serve this configuration"
        og = model.generate(cond, audio_prefix_codes=pre, max_new_tokens=new, cfg_scale=1.0, sampling_params=GREEDY).cpu()      # 8-step graphs
        assert eng.lib.zn_decode_path_detail(eng.h) == 2
        assert o1.shape[-1] == prefix + new and torch.equal(og, o1)
        eng.call("zn_debug_tune", PE, 2)
        o, l = _traced(model, cond, pre, new)
        assert eng.lib.zn_decode_path_detail(eng.h) == 0, eng.lib.zn_decode_path_detail(eng.h)
        assert torch.equal(o, o1)
        assert l.shape == l1.shape and torch.equal(l.view(torch.int32), l1.view(torch.int32))
        assert eng.counters()["handoff_timeouts"] == t0 == 0
    finally:
        eng.call("zn_debug_tune", PE, 1)
        eng.call("zn_debug_eos_bias", 0.0)


@pytest.mark.parametrize("prefix,new", [(3050, 8), (4074, 8)], ids=["7-blocks", "9-blocks"])
def test_one_row_whole_step_kernel_past_six_key_blocks_is_bit_identical(full, prefix, new):
    """Just past 3072 keys (step_r1_kernel<4,1,8,4,5,8>) and just past 4096 keys (step_r1_kernel<4,2,9,5,5,12>)."""
    _case(full, prefix, new)
