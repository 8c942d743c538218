"""The codes-only FP8 KV cache (Zonos.set_kv_cache("fp8-only"), zn_set_kv_fp8_only) without a GPU: the ABI surface, the mode
strings, the plans and the byte counts per row count, and the attainability of the GPU test's interval for the prefill attention on codes."""
import ctypes as C
import os
import re

import pytest
import torch

from zonos_amd import _lib, quant, synth
from zonos_amd import testing as T
from zonos_amd.testing import build_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("zn_set_kv_fp8_only", "zn_kv_cache_plan", "zn_op_attn_prefill_rows_fp8")
ROWS = (1, 4, 5, 16, 64)


def test_abi_surface():
    assert _lib.ZN_TUNE_KV_FP8 == 25 and _lib.ZN_TUNE_NKEYS == 26, "the mode adds no tune key"
    header = open(os.path.join(ROOT, "include", "zonos_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\bint %s\(zn_handle h," % name, header), f"{name} is not declared in include/zonos_hip.h"
    assert _lib.SIGNATURES["zn_op_attn_prefill_rows_fp8"] == _lib.SIGNATURES["zn_op_attn_prefill_rows"]
    from zonos_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
    out = (C.c_int32 * 3)()
    assert lib.zn_set_kv_fp8_only(None, 1) == -1 and lib.zn_kv_cache_plan(None, 8, out) == -1
    assert lib.zn_op_attn_prefill_rows_fp8(None, None, None, 8, None, 4, 1, 0, None, None) == -1


def test_mode_strings():
    model, _ = build_model(synth.TINY_CFG, 77, "cpu")
    assert quant.KV_CACHE_MODES == ("bf16", "fp8", "fp8-only")
    for mode in ("fp8-only", "fp8", "fp8-only", "bf16"):
        assert model.set_kv_cache(mode) is model and model.kv_cache == mode
    for bad in ("fp4", "fp8_only", "FP8-ONLY", ""):
        with pytest.raises(ValueError):
            model.set_kv_cache(bad)
    assert model.kv_cache == "bf16"


def test_hybrid_model_is_refused():
    model, _ = build_model(synth.HYBRID_TINY_CFG, 77, "cpu")
    with pytest.raises(ValueError, match="hybrid"):
        model.set_kv_cache("fp8-only")
    assert model.kv_cache == "bf16" and model.kv_cache_plan(16) == {"rounded": False, "attention_reads": "bf16", "bf16_cache": True}


def test_plans_and_bytes_per_row_count():
    model, _ = build_model(synth.TINY_CFG, 77, "cpu")
    bb = model.config.backbone
    hkv, hd = bb.attn_cfg["num_heads_kv"], bb.d_model // bb.attn_cfg["num_heads"]
    max_len = 450                                              # (rounded up to 456, a multiple of 8, as setup_cache does)
    full = lambda rows: bb.n_layer * rows * 456 * 2 * hkv * hd * 2
    off = {"rounded": False, "attention_reads": "bf16"}
    on = {"rounded": True, "attention_reads": "fp8"}
    for rows in ROWS:
        assert model.kv_fp8_plan(rows) == off and model.kv_cache_plan(rows) == {**off, "bf16_cache": True}
        assert model.kv_cache_bytes(rows, max_len) == {"bf16": full(rows), "codes": 0}
    model.set_kv_cache("fp8")
    for rows in ROWS:
        want = on if rows >= 5 else off
        assert model.kv_fp8_plan(rows) == want, rows
        assert model.kv_cache_plan(rows) == {**want, "bf16_cache": True}, f"'fp8' keeps both caches ({rows} rows)"
        assert model.kv_cache_bytes(rows, max_len) == {"bf16": full(rows), "codes": full(rows) // 2 if rows >= 5 else 0}, rows
    model.set_kv_cache("fp8-only")
    for rows in ROWS:
        want = on if rows >= 5 else off
        assert model.kv_fp8_plan(rows) == want, f"kv_fp8_plan keeps its two keys and their meaning ({rows} rows)"
        # below 5 rows the mode is inert: the bf16 cache is needed and nothing is rounded; from 5 rows on there is no bf16 cache
        assert model.kv_cache_plan(rows) == {**want, "bf16_cache": rows < 5}, rows
        assert model.kv_cache_bytes(rows, max_len) == ({"bf16": 0, "codes": full(rows) // 2} if rows >= 5 else {"bf16": full(rows), "codes": 0}), rows
    with pytest.raises(ValueError):
        model.kv_cache_plan(0)
    with pytest.raises(ValueError):
        model.kv_cache_bytes(8, 0)


def test_session_bytes_at_the_checkpoint_dimensions():
    """The table of DESIGN.md 4.1l: 64 rows x 6144 positions x 26 layers at the Zonos-v0.1 dimensions."""
    lib = _lib.load()
    zc = _lib.zn_config(d_model=2048, n_layer=26, n_heads=16, n_heads_kv=4)
    bf16 = 26 * lib.zn_kv_bytes_per_layer(C.byref(zc), 64, 6144)
    codes = 26 * lib.zn_kv_fp8_bytes_per_layer(C.byref(zc), 64, 6144)
    assert bf16 == 26 * 64 * 6144 * 2048 and codes * 2 == bf16
    assert [round(n / 1e9, 1) for n in (bf16, bf16 + codes, codes)] == [20.9, 31.4, 10.5]


def test_the_interval_is_attainable_on_the_dequantised_operands():
    """The GPU bar of tests/test_gpu_kv_fp8_only.py: the kernels' arithmetic in plain fp32 (attention_restatement) on K and V rounded to the E4M3
    grid stays inside attention_reference's float64 interval on the same operands, for every prefill case; no case saturates, and the rounding
    changes every case."""
    cases = T.attention_cases_prefill()
    assert len(cases) == 106
    for c in cases:
        t = T.attention_case_tensors(c)
        (_, k8), (_, v8) = quant.kv_round_e4m3(t["k"]), quant.kv_round_e4m3(t["v"])
        assert float(torch.maximum(k8.float().abs().max(), v8.float().abs().max())) < 448.0, f"{c.name}: an operand reaches the saturation value"
        assert not torch.equal(k8.view(torch.int16), t["k"].view(torch.int16)) and not torch.equal(v8.view(torch.int16), t["v"].view(torch.int16)), c.name
        ref = T.attention_reference(t["q"], k8, v8, t["scale"], t["visible"])
        got = T.attention_restatement(t["q"], k8, v8, t["scale"], t["visible"], span=t["span"])
        res = T.attention_compare(got, ref, c.name, quiet=True)
        assert res.ok and res.outside == 0 and res.nonfinite == 0, res.line(c.name)
