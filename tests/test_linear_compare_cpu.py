"""The interval comparator of the fused linears (zonos_amd.testing.linear_fused_reference / linear_fused_compare) on the CPU.

(a) A stand-in for the kernels - torch fp32 matmul, fp32 layer_norm -> bf16, the epilogue in fp32 with the rounding points of gemv_epilogue -
lies inside [lo, hi] on EVERY element of EVERY case of tests/test_gpu_linear_fused.py's table, and on those inputs at most 1 % of any row's
normalised activations sit at a bf16 rounding boundary: the reference alone stays inside its own bar, with no tolerance constant.
(b) Each of seven subtly wrong kernels, written as a mutation of the stand-in, is rejected on at least one element."""
import numpy as np
import pytest
import torch

from zonos_amd import testing as T
from zonos_amd.backbone._hip import ROPE_POSITIONS, rope_table
from zonos_amd.testing import (LF_F32, LF_PRO_LN, LF_PRO_NONE, LF_RESID, LF_ROPE_KV, LF_SILU, LF_STORE, LinearCase, linear_case_positions,
                               linear_case_reference, linear_case_tensors, linear_fused_compare)

EPS = 1e-5
bf = torch.bfloat16


@pytest.fixture(scope="module")
def ropes():
    return {hd: rope_table(ROPE_POSITIONS, hd) for hd in (128, 64)}


def standin(c: LinearCase, t: dict, rope=None, mut: str = "", at=(0, 0)):
    """The fused linear in torch fp32.  `mut`: one of the wrong kernels of part (b), applied at (row, column) `at`."""
    r, n = at
    W = t["W"].float()
    K = c.K
    if c.pro == LF_PRO_NONE:
        xt = t["x"]
    elif c.pro == LF_PRO_LN:
        x = t["x"].float()
        xt = torch.nn.functional.layer_norm(x, (K,), t["ln_w"].float(), t["ln_b"].float(), EPS).to(bf)
        if mut == "ln_tile":              # row r: the statistics of the 16-column tile n never arrive
            keep = torch.ones(K, dtype=torch.bool)
            keep[16 * n:16 * n + 16] = False
            mu, var = x[r, keep].mean(), x[r, keep].var(unbiased=False)
            xt[r] = ((x[r] - mu) / torch.sqrt(var + EPS) * t["ln_w"].float() + t["ln_b"].float()).to(bf)
    else:
        g = t["gv"]
        xt = ((g * (1.0 / torch.sqrt((g * g).mean(-1, keepdim=True) + EPS))) * t["ln_w"].float()).to(bf)
    xf = xt.float()
    acc = xf @ W.T
    if mut == "drop8":                    # the last 8 K-elements of one output
        acc[r, n] -= (xf[r, -8:] * W[n, -8:]).sum()
    if mut == "tile_row":                 # one 16-column tile taken from the neighbouring row
        acc[r, 16 * n:16 * n + 16] = acc[r + 1, 16 * n:16 * n + 16]
    if mut == "slice_twice":              # the first of four split-K slices of a row added twice
        acc[r] += xf[r, :K // 4] @ W[:, :K // 4].T
    rb = lambda v: v.to(bf).float()
    if c.epi == LF_STORE:
        return (acc + t["bias"].float()).to(bf) if c.bias else acc.to(bf)
    if c.epi == LF_F32:
        return rb(acc)
    if c.epi == LF_RESID:
        return (t["resid"].float() + (acc if mut == "resid_before" else rb(acc))).to(bf)
    if c.epi == LF_SILU:
        F = c.N // 2
        y, g = rb(acc[:, :F]), rb(acc[:, F:])
        if mut == "swap":
            y, g = g, y
        return (y * rb(g / (1.0 + torch.exp(-g)))).to(bf)
    assert c.epi == LF_ROPE_KV
    _, pos = linear_case_positions(c)
    if mut == "pos-1":
        pos = pos - 1
    nr = (2048 // c.hd + 512 // c.hd) * c.hd
    v = rb(acc)
    tab = rope[pos.clamp(0, ROPE_POSITIONS - 1)]
    j = torch.arange(nr // 2) % (c.hd // 2)
    cs, sn = tab[:, j, 0], tab[:, j, 1]
    x0, x1 = v[:, 0:nr:2].clone(), v[:, 1:nr:2].clone()
    v[:, 0:nr:2], v[:, 1:nr:2] = rb(x0 * cs - x1 * sn), rb(x1 * cs + x0 * sn)
    return v.to(bf)


def _inside(c, t, ropes, x=None):
    ref = linear_case_reference(c, t, EPS, ropes.get(c.hd), ROPE_POSITIONS)
    got = standin(c, t, ropes.get(c.hd))
    res = linear_fused_compare(got, ref, c.label)
    assert res.ok and res.violations == 0, (c.label, res)
    assert ref.ambiguous <= T.LF_AMBIGUOUS_CAP, (c.label, ref.ambiguous)
    assert res.eq_mid > 0.5, (c.label, res)           # (sanity of mid itself: the stand-in mostly lands on the epilogue of the exact sum)
    return got


FAMILIES = [("gemv", K) for K in T._GEMV_KS_NCH] + [("rope", 128), ("rope", 64), ("gemm16k", 0), ("gemm16s", 0), ("gemm16", 0), ("prefill", 0)]


def cases_of(family, arg):
    return {"gemv": lambda: T.linear_cases_gemv(arg), "rope": lambda: T.linear_cases_rope(arg), "gemm16k": T.linear_cases_gemm16k,
            "gemm16s": T.linear_cases_gemm16s, "gemm16": T.linear_cases_gemm16, "prefill": T.linear_cases_prefill}[family]()


@pytest.mark.parametrize("family,arg", FAMILIES)
def test_standin_lies_inside_the_interval_on_every_case(family, arg, ropes, capsys):
    cases = cases_of(family, arg)
    assert len(cases) >= 18
    for c in cases:
        _inside(c, linear_case_tensors(c), ropes)
    capsys.readouterr()                                # (hundreds of lines; the GPU run's are the record)


@pytest.mark.parametrize("rows", T.LF_PAIR_ROWS)
def test_standin_lies_inside_the_interval_on_the_statistics_pair(rows, ropes, capsys):
    """fc1 normalises the bf16 rows its producer stored: here the stand-in's, on the GPU the out kernel's own."""
    for k_out, Ns in ((2048, [f[0] for f in T.LF_PAIR_FC1]), (4096, [2560])):
        x1 = None
        for N in Ns:
            out, fc1 = T.linear_cases_pair(rows, N, k_out)
            if x1 is None:
                x1 = _inside(out, linear_case_tensors(out), ropes)
            _inside(fc1, linear_case_tensors(fc1, x=x1), ropes)
    capsys.readouterr()


# ---------------------------------------------------------------------------------------------- (b) wrong kernels
def _rejected(c, t, ropes, mut, at, x=None):
    ref = linear_case_reference(c, t, EPS, ropes.get(c.hd), ROPE_POSITIONS)
    assert linear_fused_compare(standin(c, t, ropes.get(c.hd)), ref, c.label).ok
    res = linear_fused_compare(standin(c, t, ropes.get(c.hd), mut=mut, at=at), ref, f"{c.label}, mutation {mut}")
    assert not res.ok and res.violations >= 1, (mut, res)
    return res


def test_dropped_k_tail_is_rejected(ropes):
    c = LinearCase("gemm16s", LF_PRO_NONE, LF_STORE, 5, 96, 256)
    res = _rejected(c, linear_case_tensors(c), ropes, "drop8", (3, 95))
    assert res.violations == 1 and res.worst == (3, 95)


def test_tile_from_the_neighbouring_row_is_rejected(ropes):
    c = LinearCase("gemm16k", LF_PRO_NONE, LF_F32, 16, 72, 2048)
    res = _rejected(c, linear_case_tensors(c), ropes, "tile_row", (14, 4))           # the clamped edge tile: columns 64..71
    assert 1 <= res.violations <= 8 and res.worst[0] == 14 and res.worst[1] >= 64


def test_gate_and_value_swapped_is_rejected(ropes):
    c = LinearCase("gemm16s", LF_PRO_NONE, LF_SILU, 5, 96, 256)
    _rejected(c, linear_case_tensors(c), ropes, "swap", (0, 0))


def test_residual_added_before_the_rounding_is_rejected(ropes):
    """An input on which bf16(resid + acc) and bf16(resid + bf16(acc)) differ: acc = 1 + 1.5 * 2^-9 rounds to 1 (by 0.5 * 2^-9, far more than
    the sum's error bound), resid = 2^-9; after the rounding 1 + 2^-9 -> 1, before it 1 + 2.5 * 2^-9 -> 1 + 2^-7."""
    c = LinearCase("gemv", LF_PRO_NONE, LF_RESID, 1, 16, 8)
    x = torch.zeros(1, 8)
    x[0, :2] = 1.0
    W = torch.zeros(16, 8)
    W[:, 0], W[:, 1] = 1.0, 1.5 * 2.0 ** -9
    t = dict(x=x.to(bf), W=W.to(bf), resid=torch.full((1, 16), 2.0 ** -9).to(bf))
    ref = linear_case_reference(c, t, EPS)
    assert torch.equal(ref.lo, ref.hi) and float(ref.lo[0, 0]) == 1.0
    res = _rejected(c, t, ropes, "resid_before", (0, 0))
    assert res.violations == 16
    assert float(standin(c, t, mut="resid_before")[0, 0]) == 1.0 + 2.0 ** -7


def test_split_k_slice_added_twice_is_rejected(ropes):
    c = LinearCase("gemm16s", LF_PRO_NONE, LF_RESID, 16, 2048, 8192)
    res = _rejected(c, linear_case_tensors(c), ropes, "slice_twice", (9, 0))
    assert res.worst[0] == 9 and res.violations > 1024


def test_layernorm_statistics_missing_a_tile_is_rejected(ropes):
    c = LinearCase("gemm16s", LF_PRO_LN, LF_SILU, 5, 2560, 2048)
    res = _rejected(c, linear_case_tensors(c), ropes, "ln_tile", (2, 77))
    assert res.worst[0] == 2


def test_rope_at_the_previous_position_is_rejected(ropes):
    for c in (T.linear_cases_rope(128)[3], T.linear_cases_rope(64)[-1]):
        assert c.epi == LF_ROPE_KV
        res = _rejected(c, linear_case_tensors(c), ropes, "pos-1", (0, 0))
        assert res.worst[1] < 2560                  # q or k: v does not rotate


def test_comparator_rejects_nan_and_shape_mismatch(ropes):
    c = LinearCase("gemv", LF_PRO_NONE, LF_STORE, 2, 72, 264)
    t = linear_case_tensors(c)
    ref = linear_case_reference(c, t, EPS)
    got = standin(c, t).float()
    got[1, 7] = float("nan")
    res = linear_fused_compare(got, ref, "NaN")
    assert not res.ok and res.violations == 1 and res.worst == (1, 7)
    with pytest.raises(ValueError):
        linear_fused_compare(got[:, :-1], ref)
    assert np.isfinite(ref.lo.numpy()).all() and bool((ref.lo <= ref.mid).all()) and bool((ref.mid <= ref.hi).all())
