"""The interval comparator of the attention kernels (zonos_amd.testing.attention_reference / attention_compare) on the CPU.

(a) fexp_u20_np, the numpy restatement of zn_fexp_u20, is measured against float64 exp over a dense grid of fp32 arguments: the measured maximum
is printed and AT_FEXP_ETA is the next power of two above it.
(b) On EVERY case of tests/test_gpu_attention.py's tables, torch CPU scaled_dot_product_attention on the bf16 tensors (the reference's own op) and
a plain fp32 restatement of the kernels' arithmetic lie inside [lo, hi] at every element, the float64 reference is finite, every spotlight key
holds at least half of its query's weight, and the restatement gives the same bits whatever the tail holds.
(c) Each of ten wrong kernels, written as a variant of the restatement, is rejected by attention_compare on the case named beside it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from zonos_amd import testing as T
from zonos_amd.testing import attention_case_tensors, attention_compare, attention_reference, attention_restatement

DECODE = {c.name: c for c in T.attention_cases_decode()}
PREFILL = {c.name: c for c in T.attention_cases_prefill()}
_REFS: dict = {}


def case_ref(c):
    if c.name not in _REFS:
        t = attention_case_tensors(c)
        _REFS[c.name] = (t, attention_reference(t["q"], t["k"], t["v"], t["scale"], t["visible"]))
    return _REFS[c.name]


def test_case_names_are_unique():
    assert len(DECODE) == len(T.attention_cases_decode()) and len(PREFILL) == len(T.attention_cases_prefill())


def test_fexp_u20_measured_error_sets_eta():
    err, at, n = T.fexp_u20_max_rel_error()
    print(f"\n[attention eta_exp] max |fexp_u20 / exp - 1| = {err:.6g} at x = {at:.6f} over {n} fp32 arguments of [ln(FLT_MIN), 0]; "
          f"AT_FEXP_ETA = 2^{int(np.log2(T.AT_FEXP_ETA))} = {T.AT_FEXP_ETA:.6g}")
    assert n > 4_000_000
    assert T.AT_FEXP_ETA == 2.0 ** int(np.ceil(np.log2(err))), "the constant is the next power of two above the measured maximum"
    assert abs(err - T.AT_FEXP_MEASURED) <= 1e-8, "the figure written beside the constant is the measured one"
    x = np.array([0.0, -1.0, -87.0, -87.4, -1000.0, np.nan, -np.inf], dtype=np.float32)
    y = T.fexp_u20_np(x)
    assert y[0] < 1.0 and abs(y[0] - 1.0) < 1.2e-4 and abs(y[1] / np.exp(-1.0) - 1.0) < 1.2e-4 and y[2] > 0.0
    assert (y[3:] == 0.0).all(), "below ln(FLT_MIN), and for NaN, the function returns 0"


def sdpa(c, t):
    """torch CPU SDPA as oracle/zonos_oracle.py calls it (is_causal for S > 1, enable_gqa), row by row over the row's own keys; with keys cached
    before the first position (base > 0) the causal mask is passed as a mask."""
    out = torch.full(t["q"].shape, float("nan"), dtype=torch.bfloat16)
    for r in range(c.R):
        if c.kind == "decode":
            L = int(c.lens[r])
            out[r:r + 1] = F.scaled_dot_product_attention(t["q"][r:r + 1], t["k"][r:r + 1, :, :L], t["v"][r:r + 1, :, :L], enable_gqa=True)
            continue
        Sv = int(c.lens[r]) if c.ragged else c.S
        q, k, v = t["q"][r:r + 1, :, :Sv], t["k"][r:r + 1, :, :c.base + Sv], t["v"][r:r + 1, :, :c.base + Sv]
        if c.base == 0:
            out[r:r + 1, :, :Sv] = F.scaled_dot_product_attention(q, k, v, is_causal=Sv > 1, enable_gqa=True)
        else:
            out[r:r + 1, :, :Sv] = F.scaled_dot_product_attention(q, k, v, attn_mask=t["visible"][r, :Sv, :c.base + Sv], enable_gqa=True)
    return out


def with_tail(c, t, tail, first_only=False):
    k, v = t["k"].clone(), t["v"].clone()
    bits = int(tail, 16)
    bits = bits - 65536 if bits >= 32768 else bits
    for r in range(c.R):
        s0 = int(t["start"][r])
        s1 = s0 + 1 if first_only else c.cap
        k.view(torch.int16)[r, :, s0:s1] = bits
        v.view(torch.int16)[r, :, s0:s1] = bits
    return k, v


def _inside(cases):
    worst = 0.0
    for c in cases:
        t, ref = case_ref(c)
        assert bool(torch.isfinite(ref.exact).all() and torch.isfinite(ref.lo).all() and torch.isfinite(ref.hi).all()), c.name
        for r, h, s, key in t["spots"]:
            assert float(ref.wmax[r, h, s]) >= 0.5 and int(ref.tmax[r, h, s]) == key, (c.name, r, h, s, key, float(ref.wmax[r, h, s]))
        if c.family in ("spot", "spot_next") and not (c.kind == "prefill" and c.family == "spot_next"):
            assert t["spots"], c.name
        a = attention_compare(sdpa(c, t), ref, c.name + " | torch CPU SDPA", quiet=True)
        rs = attention_restatement(t["q"], t["k"], t["v"], t["scale"], t["visible"], t["span"])
        b = attention_compare(rs, ref, c.name + " | fp32 restatement", quiet=True)
        assert a.ok and a.outside == 0 and a.nonfinite == 0, (c.name, a)
        assert b.ok and b.outside == 0 and b.nonfinite == 0, (c.name, b)
        k2, v2 = with_tail(c, t, "0x7FC0")
        rs2 = attention_restatement(t["q"], k2, v2, t["scale"], t["visible"], t["span"])
        ok = ref.valid[:, None, :, None].expand_as(ref.lo)
        assert torch.equal(rs2.view(torch.int16)[ok], rs.view(torch.int16)[ok]), c.name
        worst = max(worst, a.headroom, b.headroom)
        print(f"[attention {c.name}] SDPA headroom {a.headroom:.3f}, restatement {b.headroom:.3f}, Theta max {float(ref.theta.max()):.3g}")
    return worst


def test_sdpa_and_restatement_inside_the_interval_decode():
    print(f"\nworst headroom {_inside(DECODE.values()):.3f}")


@pytest.mark.parametrize("hd", [128, 64, 32])
def test_sdpa_and_restatement_inside_the_interval_prefill(hd):
    print(f"\nworst headroom {_inside([c for c in PREFILL.values() if c.hd == hd]):.3f}")


# ---------------------------------------------------------------------------------------------- ten wrong kernels
def _roll_rows(vis):
    return torch.roll(vis, 1, 0)


def mutant(name, c, t):
    q, k, v, vis, span, scale = t["q"], t["k"], t["v"], t["visible"].clone(), t["span"], t["scale"]
    mut = ""
    last = vis.long().sum(-1) - 1                                            # [R][Sq] newest visible key
    if name == "drop_newest":
        for r in range(c.R):
            for s in range(vis.shape[1]):
                if last[r, s] > 0:
                    vis[r, s, last[r, s]] = False
    elif name == "extra_key":
        for r in range(c.R):
            if int(t["start"][r]) < c.cap:
                vis[r, :, int(t["start"][r])] |= vis[r].any(-1)
    elif name == "no_rescale":
        mut = "no_rescale"
    elif name == "no_max":
        mut = "no_max"
    elif name == "head_mod":
        hq, hkv = c.heads
        idx = [h % hkv for h in range(hq)]
        k, v = k[:, idx], v[:, idx]
    elif name == "kv_swapped":
        k, v = v, k
    elif name in ("causal_plus", "causal_minus"):
        tt, ss = torch.arange(c.cap), torch.arange(c.S)
        d = 1 if name == "causal_plus" else -1
        vis = (tt[None, None, :] <= (c.base + ss[None, :, None] + d).clamp(min=0)) & vis.any(-1, keepdim=True)
    elif name == "neighbour_length":
        vis = _roll_rows(vis)
    elif name == "no_scale":
        scale = 1.0
    elif name == "tail_unmasked":
        k, v = with_tail(c, t, "0x7FC0", first_only=True)
        mut = "tail_unmasked"
    else:
        raise ValueError(name)
    return attention_restatement(q, k, v, scale, vis, span, mut=mut)


MUTANTS = [
    ("drop_newest", "d128g4 r5 cap1032", DECODE),                 # 1  the newest key is dropped (L - 1 visible)
    ("extra_key", "d128g4 r2 cap520", DECODE),                    # 2  one key past the context is included (it would have been the spotlight)
    ("no_rescale", "d128g4 rise cap1536", DECODE),                # 3  f_j = 1 at more than 512 keys
    ("no_max", "d128g4 fall cap512", DECODE),                     # 4  no max subtraction: exp(100) overflows
    ("head_mod", "d128g4 r2 cap512", DECODE),                     # 5  kv head = head % Hkv instead of head // G
    ("kv_swapped", "d64g4 r2 cap512", DECODE),                    # 6  K and V swapped
    ("causal_plus", "p128g4 mfma spot_next S767", PREFILL),                 # 7a position s sees one key past base + s
    ("causal_minus", "p128g4 valu spot S20+500", PREFILL),             # 7b ... or one fewer
    ("neighbour_length", "d128g4 r16 cap1032", DECODE),           # 8  a row takes its neighbour's length
    ("neighbour_length", "p64g4 valu spot S21 ragged", PREFILL),       # 8  ... or row_len
    ("no_scale", "d32g4 r5 cap1032", DECODE),                     # 9  the scale is missing
    ("tail_unmasked", "d128g4 r2 cap1032", DECODE),               # 10 a NaN in the first key past the context reaches the output
]


@pytest.mark.parametrize("name,case,table", MUTANTS, ids=[f"{m[0]}@{m[1]}".replace(" ", "_") for m in MUTANTS])
def test_wrong_kernels_are_rejected(name, case, table):
    c = table[case]
    t, ref = case_ref(c)
    good = attention_compare(attention_restatement(t["q"], t["k"], t["v"], t["scale"], t["visible"], t["span"]), ref, case, quiet=True)
    assert good.ok, "the unmutated restatement must pass on the case that rejects the mutant"
    bad = attention_compare(mutant(name, c, t), ref, f"{case} | mutant {name}")
    assert not bad.ok and (bad.outside > 0 or bad.nonfinite > 0), (name, case, bad)
    if name in ("no_max", "tail_unmasked"):
        assert bad.nonfinite > 0, (name, bad)
