"""The FP8 weight format on the CPU: zonos_amd/quant.py is the specification the device kernels are held to (tests/test_gpu_fp8.py), so it is
checked here against the E4M3 definition itself - a table built from the bit fields, not from torch's cast - against torch.float8_e4m3fn where
torch defines the value, and on its stated properties: the dequantised weights are exact bf16, quantising them again returns them, the error
bounds of the docstring hold, the NaN codes never appear.  Then the plan: tests/linear_plan_fp8_check.cpp walks plan_linear's FP8 offer over the
grid of tests/linear_plan_check.cpp."""
import os
import shutil
import subprocess

import pytest
import torch

from zonos_amd import quant as Q
from zonos_amd import testing as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bf = torch.bfloat16


def definition_table():
    """value of every byte code, written out from the format: sign, 4 exponent bits (bias 7), 3 mantissa bits; exponent 0 is subnormal
    (mantissa / 8 * 2^-6); S.1111.111 is NaN and there are no infinities."""
    vals = {}
    for sign in (0, 1):
        for e in range(16):
            for m in range(8):
                code = (sign << 7) | (e << 3) | m
                if e == 15 and m == 7:
                    vals[code] = None
                    continue
                mag = (m / 8.0) * 2.0 ** -6 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7)
                vals[code] = -mag if sign else mag
    return vals


def bits(t):
    return t.contiguous().view(torch.int16)


def test_every_code_decodes_to_the_definition():
    tab, ref = Q.e4m3_value_table(), definition_table()
    finite = [c for c in range(256) if ref[c] is not None]
    assert len(finite) == 254 and max(abs(ref[c]) for c in finite) == 448.0 == Q.E4M3_MAX
    for c in range(256):
        if ref[c] is None:
            assert c in (0x7F, 0xFF) and bool(torch.isnan(tab[c]))
        else:
            assert float(tab[c]) == ref[c], c
    assert bool(torch.signbit(tab[0x80])) and float(tab[0x80]) == 0.0
    # torch's own E4M3 wherever it defines a value
    f8 = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float64)
    ok = ~torch.isnan(f8)
    assert int(ok.sum()) == 254 and torch.equal(f8[ok], tab[ok])
    # and the dequantiser over every finite code at the exponents the device test uses: exact, and exact in bf16
    q = torch.tensor(finite, dtype=torch.uint8).repeat(7, 1)
    exps = torch.tensor([-100, -17, -1, 0, 1, 17, 100], dtype=torch.int8)
    w = Q.dequantize_rows_fp8(q, exps)
    for i, k in enumerate(exps.tolist()):
        for j, c in enumerate(finite):
            assert float(w[i, j].double()) == ref[c] * 2.0 ** k, (c, k)
    nz = w.double().abs()[w.double() != 0]
    assert float(nz.min()) == 2.0 ** -109 and float(nz.min()) >= 2.0 ** -126, "the smallest magnitude is a normal bf16"


def check_properties(W, label, clamped=()):
    """The docstring's properties on bf16 [N, K]; `clamped`: rows whose amax lies outside the clamp (saturation, no error bound)."""
    q, exp, Wdq = Q.quantize_rows_fp8(W)
    assert q.dtype == torch.uint8 and exp.dtype == torch.int8 and Wdq.dtype == bf and q.shape == W.shape == Wdq.shape and exp.shape == (W.shape[0],)
    assert not bool(((q & 0x7F) == 0x7F).any()), f"{label}: a NaN code"
    assert int(exp.min()) >= Q.EXP_MIN and int(exp.max()) <= Q.EXP_MAX
    tab = Q.e4m3_value_table()
    exact = tab[q.long()] * torch.exp2(exp.double())[:, None]
    assert bool(torch.isfinite(exact).all())
    assert torch.equal(Wdq.double(), exact), f"{label}: Wdq is not code * 2^k exactly"
    assert torch.equal(bits(Wdq.to(bf)), bits(Wdq)) and torch.equal(Wdq.float().to(bf).double(), exact)
    assert torch.equal(torch.signbit(Wdq), torch.signbit(W)), f"{label}: a sign changed"
    # idempotent on Wdq
    q2, exp2, Wdq2 = Q.quantize_rows_fp8(Wdq)
    assert torch.equal(bits(Wdq2), bits(Wdq)), f"{label}: quantising the dequantised weights changed them"
    assert bool((((exp2 == exp) & (q2 == q).all(1)) | ((exp2 == exp - 1) & (tab[q2.long()] == 2 * tab[q.long()]).all(1)) | (Wdq == 0).all(1)).all())
    # the scale exponent is the smallest k with amax <= 448 * 2^k
    amax = W.double().abs().amax(1)
    inside = torch.ones(W.shape[0], dtype=torch.bool)
    inside[list(clamped)] = False
    k = exp.double()
    nzr = inside & (amax > 0)
    assert bool((amax[nzr] <= 448.0 * torch.exp2(k[nzr])).all()) and bool(((amax[nzr] > 448.0 * torch.exp2(k[nzr] - 1)) | (k[nzr] == Q.EXP_MIN)).all())
    assert bool((exp[amax == 0] == 0).all())
    # error bounds inside the clamp
    w, d = W.double()[inside], Wdq.double()[inside]
    scaled = w.abs() * torch.exp2(-k[inside])[:, None]
    normal = scaled >= 2.0 ** -6
    err = (d - w).abs()
    assert bool((err[normal] <= 2.0 ** -4 * w.abs()[normal]).all()), f"{label}: normal-range bound"
    sub_bound = (2.0 ** -10 * torch.exp2(k[inside]))[:, None].expand_as(err)
    assert bool((err[~normal] <= sub_bound[~normal]).all()), f"{label}: subnormal-range bound"
    assert bool((scaled <= 448.0).all()), f"{label}: saturation inside the clamp"
    return q, exp, Wdq


@pytest.mark.parametrize("shape", T.FP8_MATRIX_SHAPES)
def test_properties_on_seeded_matrices(shape):
    W = T.fp8_seeded_matrix(*shape)
    q, exp, _ = check_properties(W, str(shape))
    assert len(set(exp.tolist())) >= 8, "the rows' exponents should differ"
    assert bool(((q & 0x78) == 0).any()) and bool(((q & 0x7F) == 0x7E).any()), "subnormal codes and the largest code both occur"
    # torch's cast of the exactly scaled weights rounds the same way
    scaled = (W.double() * torch.exp2(-exp.double())[:, None]).float()
    assert torch.equal(q.view(torch.float8_e4m3fn).double(), scaled.to(torch.float8_e4m3fn).double())


def test_adversarial_rows():
    W, names = T.fp8_adversarial_rows()
    clamped = [i for i, n in enumerate(names) if n.startswith("beyond the clamp")]
    assert len(clamped) == 2
    q, exp, Wdq = check_properties(W, "adversarial", clamped)
    row = {n: i for i, n in enumerate(names)}
    tab = Q.e4m3_value_table()
    val = lambda n: (tab[q[row[n]].long()] * 2.0 ** int(exp[row[n]])).tolist()
    assert int(exp[row["zero"]]) == 0 and not bool(q[row["zero"]].any())
    assert q[row["negative zero"], 0] == 0x80
    one = q[row["one element"]]
    assert int((one != 0).sum()) == 1 and (int(one[2]) & 0x7F) >= 0x78, "a lone element sits in the top binade of the codes"
    for j in (-20, 0, 9):
        assert int(exp[row[f"amax 448*2^{j}"]]) == j and q[row[f"amax 448*2^{j}"], 0] == 0x7E
        assert int(exp[row[f"amax 446*2^{j}"]]) == j and q[row[f"amax 446*2^{j}"], 0] == 0xFE          # 446 rounds to 448: no saturation involved
        assert int(exp[row[f"amax 450*2^{j}"]]) == j + 1 and q[row[f"amax 450*2^{j}"], 0] == 0x76     # 225 -> 224
    # ties go to the even mantissa, both ways
    assert int(exp[row["midpoints"]]) == 0
    assert val("midpoints")[:15] == [448.0, 16.0, -20.0, 20.0, 24.0, 1.0, -1.25, 2.0, 256.0, -224.0, 2.0 ** -6, 2.0 ** -6 + 2.0 ** -8, 32.0, -32.0, 256.0]
    s = 2.0 ** -9
    assert val("subnormal codes")[:14] == [448.0, 0.0, -0.0, 2 * s, 2 * s, -4 * s, s, 0.0, 8 * s, 8 * s, 4 * s, s, s, 0.0]
    # beyond the clamp: saturation at +-448 * 2^100, nothing non-finite; and everything below half a step vanishes
    big, small = row["beyond the clamp, large"], row["beyond the clamp, small"]
    assert int(exp[big]) == 100 and int(exp[small]) == -100
    assert q[big, :8].tolist() == [0x7E, 0xFE, 0x7E, 0x7E, 0x00, 0x01, 0x00, 0x7E]
    assert q[small, :8].tolist() == [0x00, 0x80, 0x00, 0x02, 0x01, 0x82, 0x00, 0x00]
    assert bool(torch.isfinite(Wdq.float()).all()) and float(Wdq[big].double().abs().max()) == 448.0 * 2.0 ** 100


def test_fp8_offer_in_the_linear_plan(tmp_path):
    """w8 is set only for decode GEMM16S plans of fc1 / fc2 and only when offered; offering changes no other field of any plan; with the offer
    off every plan equals the default-env plan."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "linear_plan_fp8_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "zonos_amd", "csrc"),
                    os.path.join(ROOT, "tests", "linear_plan_fp8_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in r.stdout and r.stdout.rstrip().endswith("OK")


def test_fp8_instantiations_are_the_production_ones():
    """The FP8 instantiations of gemm16s_kernel are what production launches - fc1 <EPI_SILU, {2, 4} | 64, {0, 1}>, fc2 <EPI_RESID, {2, 4} | 64, 0> - and
    nothing else.  (Their names match the pattern by which tests/test_abi.py finds the kernels whose split-K hand-off it disassembles.)"""
    import re
    from zonos_amd import _lib, build
    build.build(verbose=False)
    names = set(re.findall(rb"_Z14gemm16s_kernelILi(\d+)ELi(\d+)ELb([01])EEv8GemvArgs", open(_lib.LIB_PATH, "rb").read()))    # symbol tables of the library
    w8 = sorted((int(e), int(s), int(l)) for e, s, l in names if int(s) & 64)
    assert w8 == [(1, 66, 0), (1, 68, 0), (2, 66, 0), (2, 66, 1), (2, 68, 0), (2, 68, 1)], w8
