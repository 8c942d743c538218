"""Weight-only FP8 for the MLP projections: OCP E4M3 codes with one power-of-two scale per weight row.

This module is the specification (pure torch, runs on the CPU); the device kernels of zonos_amd/csrc/zn_fp8_kernels.h are tested against
it bit for bit.

`quantize_rows_fp8(W: bf16 [N, K]) -> (q: uint8 [N, K], exp: int8 [N], Wdq: bf16 [N, K])`

Scale exponent, per row: amax = max |w| and k = ceil(log2(amax / 448)), the smallest k with amax <= 448 * 2^k, taken from the bits of
amax (amax = m * 2^e, 1 <= m < 2: k = e - 8 when m <= 1.75, else e - 7), not through a float log2.  k is clamped to [-100, 100]; a zero
row has k = 0.  The inputs are finite.

Codes: q = RNE_e4m3fn(w * 2^-k) (the product is exact: a power of two), saturating at +-448.  Inside the clamp |w * 2^-k| <= 448 by the
choice of k, so saturation is reachable only through the clamp.  The sign bit of w is kept (a negative value that rounds to zero gives
0x80).  The NaN codes 0x7F and 0xFF are never produced.

Dequantised copy: Wdq = value(q) * 2^k.  A code has 3 mantissa bits and bf16 has 7, and the smallest non-zero magnitude inside the clamp
is 2^-9 * 2^-100 = 2^-109, a normal bf16 (no denormals), the largest 448 * 2^100: Wdq is exact in bf16.

Properties (tests/test_fp8_cpu.py):
  * quantisation is idempotent on Wdq: quantize_rows_fp8(Wdq) returns Wdq again, bit for bit (q and exp may shift together by one
    binade: a row whose largest scaled magnitude rounds down to 224 is re-scaled to 448 at k - 1, which doubles every code value exactly);
  * inside the clamp, |Wdq - w| <= 2^-4 |w| where the code is in E4M3's normal range (|w * 2^-k| >= 2^-6: half an ulp of 3 mantissa bits)
  * and |Wdq - w| <= 2^-10 * 2^k where it is in the subnormal range (half of the fixed step 2^-9).

The mode built on this (Zonos.quantize_mlp_fp8) is lossy with respect to the checkpoint, by these bounds, and exact with respect to its
own dequantised weights: the model's bf16 parameters are replaced by Wdq, and the FP8 bytes are a compressed stream of exactly those.
"""
from __future__ import annotations

import torch

E4M3_MAX = 448.0
EXP_MIN, EXP_MAX = -100, 100
KV_FP8_MIN_ROWS = 5          # the FP8 KV cache (Zonos.set_kv_cache) is in effect from this many rows per decode step on; below it is inert
KV_CACHE_MODES = ("bf16", "fp8", "fp8-only")      # Zonos.set_kv_cache: no FP8 cache | codes beside the bf16 cache | the codes alone


def e4m3_value_table() -> torch.Tensor:
    """float64 [256]: the value of every byte code from the OCP E4M3 definition (1 sign, 4 exponent bits of bias 7, 3 mantissa bits; no
    infinities; S.1111.111 is NaN)."""
    out = []
    for c in range(256):
        s, e, m = c >> 7, (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            v = float("nan")
        elif e == 0:
            v = m * 2.0 ** -9
        else:
            v = (1 + m / 8) * 2.0 ** (e - 7)
        out.append(-v if s else v)
    return torch.tensor(out, dtype=torch.float64)


def row_exponents(W: torch.Tensor) -> torch.Tensor:
    """int8 [N]: the scale exponent of each row of W (bf16 [N, K]), from the bits of the row's largest magnitude."""
    assert W.dtype == torch.bfloat16 and W.dim() == 2
    mag = (W.contiguous().view(torch.int16).to(torch.int32) & 0x7FFF).amax(dim=1)      # bf16 magnitudes order like their bit patterns
    e, f = mag >> 7, mag & 0x7F
    k = e - 127 - 8 + (f > 96).to(torch.int32)                                        # m = 1 + f / 128 > 1.75  <=>  f > 96
    k = torch.where(e == 0, torch.full_like(k, EXP_MIN), k)                           # bf16 denormals lie below 448 * 2^-100
    k = k.clamp(EXP_MIN, EXP_MAX)
    return torch.where(mag == 0, torch.zeros_like(k), k).to(torch.int8)


def encode_e4m3(v: torch.Tensor, negative: torch.Tensor) -> torch.Tensor:
    """uint8 codes of float64 magnitudes v >= 0: round to nearest, ties to even, saturating at 448; `negative` sets the sign bit."""
    v = v.clamp(max=2.0 ** 20)                       # (anything above 448 saturates; keeps the arithmetic below far from overflow)
    _, ex = torch.frexp(v)                           # v = mant * 2^ex, mant in [0.5, 1)
    e = (ex - 1).clamp(min=-6)                       # binade of v, the subnormal range shares the step of the lowest normal binade
    step = torch.ldexp(torch.ones_like(v), e - 3)
    r = torch.round(v / step) * step                 # torch.round: half to even; every operand is exact in float64
    r = r.clamp(max=E4M3_MAX)
    _, ex = torch.frexp(r)
    e = ex - 1
    normal = r >= 2.0 ** -6
    field = torch.where(normal, e + 7, torch.zeros_like(e))
    mant = torch.where(normal, (r / torch.ldexp(torch.ones_like(r), e) - 1) * 8, r * 2.0 ** 9)
    code = (field.to(torch.int32) << 3) | mant.to(torch.int32) | (negative.to(torch.int32) << 7)
    return code.to(torch.uint8)


def dequantize_rows_fp8(q: torch.Tensor, exp: torch.Tensor) -> torch.Tensor:
    """bf16 [N, K] = value(q) * 2^exp per row (exact)."""
    vals = e4m3_value_table()[q.long()]
    w = torch.ldexp(vals, exp.to(torch.int32)[:, None].expand_as(vals))
    return w.to(torch.float32).to(torch.bfloat16)


def quantize_rows_fp8(W: torch.Tensor):
    """See the module docstring.  W: bf16 [N, K] on any device (computed on the CPU) -> (q uint8 [N, K], exp int8 [N], Wdq bf16 [N, K])."""
    W = W.detach().cpu()
    exp = row_exponents(W)
    k = exp.to(torch.int32)[:, None]
    wd = W.to(torch.float64)
    v = torch.ldexp(wd.abs(), (-k).expand_as(wd))
    q = encode_e4m3(v, torch.signbit(wd))
    return q, exp, dequantize_rows_fp8(q, exp)


def kv_round_e4m3(x: torch.Tensor):
    """The FP8 KV cache's rounding (Zonos.set_kv_cache("fp8") and "fp8-only" - the codes beside the bf16 cache, or the codes alone; the KV
    appends of zonos_amd/csrc are tested against it bit for bit).
    x: bf16, any shape -> (codes uint8, dequantised bf16), both of x's shape.

    The element rounding of the weight format above at scale exponent 0: code = RNE_e4m3fn(x), value(code) exact in bf16.  No scale is
    applied - the fused append epilogue holds two elements of a head vector per thread and cannot take an absmax (per-layer static scales
    are a possible follow-up).  Finite values beyond +-448 saturate there, and so do the infinities; a NaN keeps its sign and takes the NaN
    code (0x7F / 0xFF), whose dequantised value is a NaN.  The sign bit is kept (-0 and negative values that round to zero give 0x80).
    |dq - x| <= 2^-4 |x| for 2^-6 <= |x| <= 448 (half an ulp of 3 mantissa bits), <= 2^-10 below (half of the subnormal step 2^-9).
    Idempotent: the dequantised values round to themselves and to the same codes."""
    assert x.dtype == torch.bfloat16
    xd = x.detach().cpu().to(torch.float64)
    nan = torch.isnan(xd)
    neg = torch.signbit(xd)
    q = encode_e4m3(torch.where(nan, torch.zeros_like(xd), xd.abs()), neg)
    q = torch.where(nan, torch.full_like(q, 0x7F) | (neg.to(torch.uint8) << 7), q)
    dq = e4m3_value_table()[q.long()].to(torch.float32).to(torch.bfloat16)
    return q, dq
