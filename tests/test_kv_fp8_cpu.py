"""The FP8 KV cache without a GPU: the rounding's specification (zonos_amd/quant.py kv_round_e4m3) over every bf16 bit pattern, the ABI surface
of the mode, the model's plan per row count, and the refusal of a hybrid model."""
import ctypes as C

import pytest
import torch

from zonos_amd import _lib, quant, synth
from zonos_amd.testing import build_model


@pytest.fixture(scope="module")
def every_bf16():
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    q, dq = quant.kv_round_e4m3(x)
    return x, q, dq


def test_dequantised_values_are_exact_idempotent_and_monotone(every_bf16):
    x, q, dq = every_bf16
    assert q.dtype == torch.uint8 and dq.dtype == torch.bfloat16 and q.shape == x.shape == dq.shape
    ok = ~torch.isnan(x)
    table = quant.e4m3_value_table()
    # exact in bf16: the bf16 value IS the code's value, nothing rounded on the way
    assert torch.equal(dq[ok].double(), table[q[ok].long()])
    q2, dq2 = quant.kv_round_e4m3(dq)
    assert torch.equal(dq2.view(torch.int16)[ok], dq.view(torch.int16)[ok]) and torch.equal(q2[ok], q[ok])
    # monotone: sorted by value, the finite inputs' images never decrease
    fin = torch.isfinite(x)
    order = torch.argsort(x[fin].double(), stable=True)
    img = dq[fin].double()[order]
    assert bool((img[1:] >= img[:-1]).all())


def test_error_bounds_saturation_and_nan(every_bf16):
    x, q, dq = every_bf16
    xd, d = x.double(), dq.double()
    normal = (xd.abs() >= 2.0 ** -6) & (xd.abs() <= 448)
    assert bool(((d - xd).abs()[normal] <= 2.0 ** -4 * xd.abs()[normal]).all())
    small = xd.abs() < 2.0 ** -6
    assert float((d - xd).abs()[small].max()) <= 2.0 ** -10
    big = (xd.abs() > 448) & ~torch.isnan(xd)                       # finite values beyond the range and both infinities
    assert int(big.sum()) > 0 and bool(torch.isinf(xd[big]).any())
    assert torch.equal(d[big], torch.sign(xd[big]) * 448) and set(q[big].tolist()) == {0x7E, 0xFE}
    nan = torch.isnan(xd)
    assert int(nan.sum()) == 254 and bool(torch.isnan(d[nan]).all()) and set(q[nan].tolist()) == {0x7F, 0xFF}
    assert bool(((q[nan] >> 7).bool() == torch.signbit(xd[nan])).all())
    assert not bool(torch.isnan(d[~nan]).any()) and not bool(((q[~nan] & 0x7F) == 0x7F).any())
    # the sign survives a rounding to zero
    assert int(q[x.view(torch.int16) == -32768]) == 0x80 and bool(torch.signbit(d[(xd < 0) & (d == 0)]).all())


def test_codes_decode_through_the_weight_format_table(every_bf16):
    """One element format for weights and K/V: a KV code is the weight quantiser's code of the same value in a row whose scale exponent is 0."""
    x, q, dq = every_bf16
    ok = ~torch.isnan(x)
    assert torch.equal(quant.dequantize_rows_fp8(q[ok][None], torch.zeros(1, dtype=torch.int8))[0].view(torch.int16), dq[ok].view(torch.int16))
    row = torch.tensor([448.0, -300.0, 17.3, 0.0117, -2.0 ** -9, 2.0 ** -10, 3.0 * 2.0 ** -10, 0.0], dtype=torch.bfloat16)[None]      # amax 448: exponent 0
    wq, wexp, wdq = quant.quantize_rows_fp8(row)
    kq, kdq = quant.kv_round_e4m3(row)
    assert int(wexp[0]) == 0 and torch.equal(wq, kq) and torch.equal(wdq.view(torch.int16), kdq.view(torch.int16))


def test_abi_surface():
    assert _lib.ZN_TUNE_KV_FP8 == 25 and _lib.ZN_TUNE_NKEYS == 26
    for name in ("zn_set_kv_fp8", "zn_kv_fp8_bytes_per_layer", "zn_gen_bind_kv_fp8", "zn_kv_fp8_plan"):
        assert name in _lib.SIGNATURES
    from zonos_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    assert hasattr(lib, "zn_set_kv_fp8")
    zc = _lib.zn_config(d_model=2048, n_layer=26, n_heads=16, n_heads_kv=4, d_ff=8192, n_codebooks=9, vocab_head=1025, vocab_embed=1032, eos_id=1024,
                        mask_id=1025, rope_positions=16384, double_out_proj=1, norm_eps=1e-5)
    # one byte per element: half of the bf16 cache, whose own query keeps its result
    assert lib.zn_kv_bytes_per_layer(C.byref(zc), 64, 450) == 64 * 450 * 2 * 4 * 128 * 2
    assert lib.zn_kv_fp8_bytes_per_layer(C.byref(zc), 64, 450) == 64 * 450 * 2 * 4 * 128
    assert lib.zn_set_kv_fp8(None, 1) == -1 and lib.zn_kv_fp8_plan(None, 8, None) == -1 and lib.zn_gen_bind_kv_fp8(None, None) == -1


def test_plan_per_row_count_and_default():
    model, _ = build_model(synth.TINY_CFG, 77, "cpu")
    assert model.kv_cache == "bf16"
    for rows in (1, 4, 5, 16, 17, 64, 65):
        assert model.kv_fp8_plan(rows) == {"rounded": False, "attention_reads": "bf16"}
    assert model.set_kv_cache("fp8") is model and model.kv_cache == "fp8"
    for rows in (1, 4):
        assert model.kv_fp8_plan(rows) == {"rounded": False, "attention_reads": "bf16"}, rows
    for rows in (5, 16, 17, 64, 65):
        assert model.kv_fp8_plan(rows) == {"rounded": True, "attention_reads": "fp8"}, rows
    model.set_kv_cache("bf16")
    assert model.kv_cache == "bf16" and model.kv_fp8_plan(16) == {"rounded": False, "attention_reads": "bf16"}
    with pytest.raises(ValueError):
        model.set_kv_cache("fp4")
    with pytest.raises(ValueError):
        model.kv_fp8_plan(0)


def test_hybrid_model_is_refused():
    model, _ = build_model(synth.HYBRID_TINY_CFG, 77, "cpu")
    with pytest.raises(ValueError, match="hybrid"):
        model.set_kv_cache("fp8")
    assert model.kv_cache == "bf16" and model.kv_fp8_plan(16) == {"rounded": False, "attention_reads": "bf16"}
    assert model.set_kv_cache("bf16").kv_cache == "bf16"
