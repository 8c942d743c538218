"""GPU parity tests of the AR decode path: HIP (through the C ABI) vs the CPU oracle and vs the committed golden
fixtures recorded from the reference (tests/golden/make_golden.py).

Bars.  Integer bookkeeping (delay pattern, EOS cadence, output length) is bit-exact.  Logits are bf16-valued
fp32: the HIP path rounds at the same points as the reference but sums in a different
order, so a teacher-forced step may differ from the reference in a small fraction of logits by one bf16 ulp of a
hidden value; the tests state the tolerance they use and require greedy indices to be identical wherever the
reference's own top-2 margin exceeds that tolerance."""
import numpy as np
import pytest
import torch

from oracle import zonos_oracle as zo
from zonos_amd import _lib, synth
from zonos_amd.backbone import HipEngine
from zonos_amd.testing import build_model

pytestmark = pytest.mark.gpu
GREEDY = {"temperature": 0.0}


def _gold(golden_dir, name):
    return np.load(f"{golden_dir}/{name}.npz")


@pytest.fixture(scope="module")
def tiny():
    model, w = build_model(synth.TINY_CFG, 77, "cuda:0")
    cond = synth.conditioning(77, "cond", 2, 6, synth.TINY_CFG["d_model"])
    return model, w, cond


@pytest.fixture(scope="module")
def full():
    model, w = build_model(synth.FULL_CFG, 1234, "cuda:0")
    return model, w


def _teacher_forced(model, cond, max_new, inputs, prefix=None):
    """Run generate() feeding the reference's tokens back after every step; returns per-step logits."""
    tr = {"logits": []}
    inp = torch.from_numpy(inputs.astype(np.int32)).to("cuda:0")      # [steps, B, 9]

    def hook(step_idx, delayed, col):
        k = step_idx + 1
        if k < inp.shape[0]:
            delayed[:, :, col] = inp[k]
    tr["after_step"] = hook
    model.generate(cond.to("cuda:0"), audio_prefix_codes=prefix, max_new_tokens=max_new, sampling_params=GREEDY, _trace=tr)
    return torch.stack(tr["logits"]).cpu().numpy()


def _ref_variation(head):
    """The reference's OWN variation at the Zonos-v0.1 dimensions (tests/golden/ref_thread_sensitivity.json, recorded by
    tools/ref_thread_sensitivity.py from the real reference run with 1, 2, 3, 5 and 8 host threads; `head` = "gaussian" | "peaky"):
    (largest teacher-forced |dlogit| between two thread counts, largest reference top-2 margin at which two thread counts disagreed on an
    argmax).  Two runs whose logits lie within d of each other can only disagree on an argmax whose margin is <= 2 d: "decisive" in the
    full-dims tests below means a reference margin above 2 d, and the HIP path's own |dlogit| against the 8-thread reference must not
    exceed d - i.e. the HIP path is held to the reference's own reproducibility, not to a hand-picked tolerance."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_thread_sensitivity.json")) as f:
        h = json.load(f)["heads"][head]
    return float(h["largest_tf_abs_dlogit"]), float(h["largest_margin_of_any_disagreement"])


def _teacher_forced_tokens(model, cond, g, dec_margin=0.5):
    """Teacher-forced greedy tokens over every step of a golden run: returns (fraction of (step, codebook) pairs whose
    HIP argmax equals the reference token, all pairs with reference margin > dec_margin equal?)."""
    got = _teacher_forced(model, cond, int(g["max_new"]), g["inputs"])
    inputs = g["inputs"].astype(np.int64)
    ga = []
    for k in range(got.shape[0]):
        lg = torch.from_numpy(got[k])
        if k > 0:
            lg = zo.repetition_penalty(lg, torch.from_numpy(inputs[max(0, k - 2):k]).permute(1, 2, 0), 3.0, 2)
        ga.append(lg.argmax(-1).numpy())
    ga = np.stack(ga)
    ref = g["tokens"].astype(np.int64)
    agree = ga == ref
    decisive = g["margin"] > dec_margin
    print(f"\n[teacher-forced tokens] {agree.shape[0]} steps: equal on {agree.mean():.4f} of pairs; decisive(>{dec_margin}) {decisive.mean():.3f}, "
          f"all decisive equal: {bool(agree[decisive].all())}")
    bad = np.argwhere(~agree)
    if len(bad):
        ms = sorted((float(g["margin"][a, b, c]) for a, b, c in bad), reverse=True)
        print(f"  {len(bad)} disagreements; their reference margins, largest first: {ms[:12]}")
    return float(agree.mean()), bool(agree[decisive].all())


def _compare_logits(got, ref, margin, name, tol, dec=None):
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin)
    diff = np.abs(np.where(fin, got - ref, 0.0))
    exact = float((diff == 0).mean())
    print(f"\n[{name}] steps={len(ref)} exact-equal logits {exact:.4f}  max|diff| {diff.max():.4g}  mean|diff| {diff.mean():.3g}")
    assert diff.max() <= tol, (name, diff.max())
    # greedy index equality wherever the reference margin is decisive
    ga, ra = np.where(fin, got, -np.inf).argmax(-1), np.where(fin, ref, -np.inf).argmax(-1)
    dec = 2 * tol if dec is None else dec
    decisive = margin > dec
    print(f"[{name}] decisive (margin>{dec}) {decisive.mean():.3f} of (step,codebook) pairs; argmax equal on all pairs: {(ga == ra).mean():.4f}")
    assert np.array_equal(ga[decisive], ra[decisive])
    return exact


def test_tiny_teacher_forced_logits_vs_reference(golden_dir, tiny):
    model, _, cond = tiny
    g = _gold(golden_dir, "tiny_gen")
    got = _teacher_forced(model, cond, int(g["max_new"]), g["inputs"])
    ref = g["logits"]
    assert got.shape == ref.shape
    # margins were recorded after the repetition penalty (the quantity argmax sees); compare pre-penalty logits
    _compare_logits(got, ref, np.full(ref.shape[:3], np.inf) if False else g["margin"], "tiny", tol=0.05)


def _free_run(model, cond, g, name):
    out = model.generate(cond.to("cuda:0"), max_new_tokens=int(g["max_new"]), sampling_params=GREEDY).cpu().numpy()
    ref = g["out"].astype(np.int64)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    frames = int((out == ref).all(axis=(0, 1)).cumprod().sum())
    print(f"\n[{name} free-run] identical frames from start: {frames}/{ref.shape[2]}; token match {(out == ref).mean():.4f}")
    return frames, float((out == ref).mean())


def test_tiny_free_running_gaussian_logits_bit_exact(golden_dir, tiny):
    """Free-running greedy on the Gaussian-logit synthetic model (only ~57 % of its (step, codebook) pairs have a top-2
    margin above the bf16 noise floor): every one of the reference's 24 frames must come out identical — north_star
    bar 1, "bit-exact codebook indices under greedy decode", on the configuration the reference itself can run."""
    model, _, cond = tiny
    g = _gold(golden_dir, "tiny_gen")
    frames, match = _free_run(model, cond, g, "tiny gaussian")
    assert frames == g["out"].shape[2] and match == 1.0, (frames, match)


def test_tiny_free_running_bit_exact_on_decisive_margins(golden_dir):
    """Peaky-head tiny model (99 % decisive margins): free-running greedy indices vs the reference, 96 frames."""
    model, _ = build_model(synth.TINY_CFG, 77, "cuda:0", peaky=True)
    cond = synth.conditioning(77, "cond", 2, 6, synth.TINY_CFG["d_model"])
    g = _gold(golden_dir, "tiny_gen_peaky")
    frames, match = _free_run(model, cond, g, "tiny peaky")
    assert frames == g["out"].shape[2] and match == 1.0, (frames, match)       # all 96 frames identical to the reference's
    agree, dec = _teacher_forced_tokens(model, cond, g)
    assert agree > 0.97 and dec, (agree, dec)


def test_tiny_generate_with_audio_prefix(golden_dir, tiny):
    model, _, cond = tiny
    g = _gold(golden_dir, "tiny_gen_prefix")
    P = int(g["prefix_len"])
    pre = torch.from_numpy(synth.randint(77, "prefix", (1, 9, P), 1024)).to("cuda:0")
    got = _teacher_forced(model, cond, int(g["max_new"]), g["inputs"], prefix=pre)
    _compare_logits(got, g["logits"], g["margin"], "tiny+prefix", tol=0.05)


def _override_run(model, cond, tokens, max_new, force=None, prefix=None):
    eng = model.engine(1)
    tk = torch.from_numpy(tokens.astype(np.int32)).to("cuda:0").contiguous()      # [calls, B, 9]
    eng.call("zn_debug_token_override", tk.data_ptr(), tk.shape[0])
    try:
        out = model.generate(cond.to("cuda:0"), audio_prefix_codes=prefix, max_new_tokens=max_new, sampling_params=GREEDY)
        torch.cuda.synchronize()
    finally:
        eng.call("zn_debug_token_override", None, 0)
    return out.cpu().numpy()


def test_bookkeeping_bit_exact_under_reference_token_stream(golden_dir, tiny):
    """K9/A11/A12: with the reference's recorded raw token stream substituted for the sampler's output, the frame
    writes, EOS staging (tensor_ops.py:155-211), stop-check cadence (tensor_ops.py:90-103), truncation and code
    mapping (model.py:511-539) must reproduce the reference output bit for bit, including its length."""
    model, _, cond = tiny
    g = _gold(golden_dir, "tiny_gen")
    out = _override_run(model, cond, g["tokens"], int(g["max_new"]))
    assert np.array_equal(out, g["out"].astype(np.int64))
    e = _gold(golden_dir, "tiny_eos")
    for key in [k for k in e.files if k.startswith("out_")]:
        s = int(key.split("_")[1])
        out = _override_run(model, cond, e[f"tokens_{s}"], int(e["max_new"]))
        assert out.shape == e[key].shape, (s, out.shape, e[key].shape)
        assert np.array_equal(out, e[key].astype(np.int64)), s
    pre = torch.from_numpy(synth.randint(77, "prefix", (1, 9, int(e["prefix_len"])), 1024)).to("cuda:0")
    for key in [k for k in e.files if k.startswith("pout_")]:
        s = int(key.split("_")[1])
        out = _override_run(model, cond, e[f"ptokens_{s}"], int(e["p_max_new"]), prefix=pre)
        assert np.array_equal(out, e[key].astype(np.int64)), s


def test_forced_eos_output_length_matches_reference(golden_dir, tiny):
    """Same cadence check with the device sampler in the loop: force codebook-0 EOS at step s through the logits
    (as the golden run did) and require the reference's output length."""
    model, _, cond = tiny
    g = _gold(golden_dir, "tiny_eos")
    eng = model.engine(1)
    try:
        for key in [k for k in g.files if k.startswith("out_")]:
            s = int(key.split("_")[1])
            eng.lib.zn_debug_force_eos(eng.h, s)
            out = model.generate(cond.to("cuda:0"), max_new_tokens=int(g["max_new"]), sampling_params=GREEDY)
            assert tuple(out.shape) == g[key].shape, (s, out.shape, g[key].shape)
    finally:
        eng.lib.zn_debug_force_eos(eng.h, -1)


@pytest.mark.parametrize("fused_limit", [512, 1], ids=["fused-launch", "two-pass"])
def test_attention_decode_vs_cpu_sdpa(full, fused_limit):
    """zn_op_attn_decode vs torch CPU SDPA (the op the reference calls at _torch.py:415) on random bf16 q/K/V at
    L = 1..1500: bit-equal fraction must exceed 0.99 (the kernel reproduces the 512-key blocking, fexp_u20 /
    libm exp split, bf16 P and reciprocal-multiply of the CPU flash kernel; residual = fp32 summation order).
    Both launch shapes: the fused one (scores in LDS via MFMA + pass 2 in one launch: KV capacities of one 512-key block) and the
    scores launch + the per-block P.V pass with its in-order combine (every longer capacity; also forced for the short ones)."""
    import torch.nn.functional as F
    model, _ = full
    eng = model.engine(1)
    eng.call("zn_debug_tune", _lib.ZN_TUNE_ATTN_FUSED_MAX_KEYS, fused_limit)
    st = _lib.stream_ptr()
    gen = torch.Generator().manual_seed(0)
    for L in (1, 5, 16, 17, 31, 300, 512, 513, 530, 900, 1500):
        cap = min(L + 3, 512) if (fused_limit > 1 and L <= 512) else 1504      # the launch shape follows the cache's capacity
        q = torch.randn(2, 16, 1, 128, generator=gen).to(torch.bfloat16)
        kv = torch.randn(2, cap, 2, 4, 128, generator=gen).to(torch.bfloat16)
        ref = F.scaled_dot_product_attention(q, kv[:, :L, 0].transpose(1, 2), kv[:, :L, 1].transpose(1, 2), enable_gqa=True)
        qd = q.transpose(1, 2).reshape(2, 2048).contiguous().to("cuda:0")
        kvd = kv.to("cuda:0")
        lengths = torch.full((2,), L - 1, dtype=torch.int32, device="cuda:0")
        out = torch.empty(2, 2048, dtype=torch.bfloat16, device="cuda:0")
        eng.call("zn_op_attn_decode", qd.data_ptr(), kvd.data_ptr(), cap, lengths.data_ptr(), None, out.data_ptr(), 2, st)
        torch.cuda.synchronize()
        got = out.cpu().view(2, 16, 128)
        r = ref[:, :, 0]
        eq = float((got.view(torch.int16) == r.contiguous().view(torch.int16)).float().mean())
        print(f"\n[attn L={L}] bit-equal {eq:.5f} max|d| {(got.float() - r.float()).abs().max().item():.3g}")
        assert eq > 0.99, (L, eq)
    eng.call("zn_debug_tune", _lib.ZN_TUNE_ATTN_FUSED_MAX_KEYS, 512)


def test_attention_long_context_split_pass_vs_cpu_sdpa(full):
    """KV capacities above 512 run the P.V pass as one workgroup per 512-key block with a ticketed in-order combine
    (acc = acc * f_j + pv_j, the reference's recurrence): same bar as the other launch shapes, contexts up to 4600 keys."""
    import torch.nn.functional as F
    model, _ = full
    eng = model.engine(1)
    st = _lib.stream_ptr()
    gen = torch.Generator().manual_seed(1)
    cap = 4608
    kv = torch.randn(2, cap, 2, 4, 128, generator=gen).to(torch.bfloat16)
    kvd = kv.to("cuda:0")
    for L in (1, 512, 513, 2049, 3000, 4600):
        q = torch.randn(2, 16, 1, 128, generator=gen).to(torch.bfloat16)
        ref = F.scaled_dot_product_attention(q, kv[:, :L, 0].transpose(1, 2), kv[:, :L, 1].transpose(1, 2), enable_gqa=True)
        qd = q.transpose(1, 2).reshape(2, 2048).contiguous().to("cuda:0")
        lengths = torch.full((2,), L - 1, dtype=torch.int32, device="cuda:0")
        out = torch.empty(2, 2048, dtype=torch.bfloat16, device="cuda:0")
        for rep in range(2):        # twice: the arrival tickets must be back at zero after a launch
            eng.call("zn_op_attn_decode", qd.data_ptr(), kvd.data_ptr(), cap, lengths.data_ptr(), None, out.data_ptr(), 2, st)
        torch.cuda.synchronize()
        got = out.cpu().view(2, 16, 128)
        r = ref[:, :, 0]
        eq = float((got.view(torch.int16) == r.contiguous().view(torch.int16)).float().mean())
        print(f"\n[attn split L={L}] bit-equal {eq:.5f} max|d| {(got.float() - r.float()).abs().max().item():.3g}")
        assert eq > 0.99, (L, eq)


def test_attention_value_column_split_is_bit_identical(full):
    """Batches of 3..8 utterances launch TWO workgroups per (row, kv head[, 512-key block]), each with all the scores / P of the pair and
    part of the value columns (attn_block_kernel<..., DS>; zn_debug_tune(ZN_TUNE_ATTN_SPLIT_COLS, 2) forces it, (ZN_TUNE_ATTN_SPLIT_COLS, 1) forbids it).  A column of P.V depends
    on P and its own V column only, so the outputs must be the SAME BITS as the unsplit launches: 16 rows of ragged lengths (one block, the
    512 / 513 boundary, several blocks, a row of one key), both launch shapes, twice each (the split shape's tickets return to zero); one
    case against torch CPU SDPA as well, so that the common value is the right one."""
    import torch.nn.functional as F
    model, _ = full
    eng = model.engine(8)
    st = _lib.stream_ptr()
    gen = torch.Generator().manual_seed(5)
    R = 16
    try:
        for cap, lens in ((512, [1, 2, 15, 16, 17, 63, 64, 65, 100, 255, 256, 300, 449, 480, 511, 512]),
                          (1024, [1, 30, 511, 512, 513, 514, 528, 529, 600, 767, 768, 769, 1000, 1022, 1023, 1024]),
                          (1536, [1, 30, 511, 512, 513, 514, 600, 1000, 1023, 1024, 1025, 1100, 1400, 1500, 1535, 1536])):
            q = torch.randn(R, 16, 1, 128, generator=gen).to(torch.bfloat16)
            kv = torch.randn(R, cap, 2, 4, 128, generator=gen).to(torch.bfloat16)
            qd = q.transpose(1, 2).reshape(R, 2048).contiguous().to("cuda:0")
            kvd = kv.to("cuda:0")
            lengths = torch.tensor([l - 1 for l in lens], dtype=torch.int32, device="cuda:0")
            outs = {}
            for mode in (1, 2):
                eng.call("zn_debug_tune", _lib.ZN_TUNE_ATTN_SPLIT_COLS, mode)
                out = torch.full((R, 2048), float("nan"), dtype=torch.bfloat16, device="cuda:0")
                for rep in range(2):
                    eng.call("zn_op_attn_decode", qd.data_ptr(), kvd.data_ptr(), cap, lengths.data_ptr(), None, out.data_ptr(), R, st)
                torch.cuda.synchronize()
                outs[mode] = out.cpu()
            assert torch.isfinite(outs[2].float()).all()
            assert torch.equal(outs[1].view(torch.int16), outs[2].view(torch.int16)), cap
            r0 = 9
            L = lens[r0]
            ref = F.scaled_dot_product_attention(q[r0:r0 + 1], kv[r0:r0 + 1, :L, 0].transpose(1, 2), kv[r0:r0 + 1, :L, 1].transpose(1, 2), enable_gqa=True)[0, :, 0]
            eq = float((outs[2][r0].view(16, 128).view(torch.int16) == ref.contiguous().view(torch.int16)).float().mean())
            print(f"\n[attn value-column split, capacity {cap}] 16 rows bit-identical to the unsplit launches; row {r0} (L = {L}) vs CPU SDPA bit-equal {eq:.5f}")
            assert eq > 0.99
    finally:
        eng.call("zn_debug_tune", _lib.ZN_TUNE_ATTN_SPLIT_COLS, 3)


@pytest.mark.parametrize("kernel", [1, 2], ids=["mfma", "valu"])
def test_attention_prefill_vs_cpu_sdpa(full, kernel):
    """zn_op_attn_prefill vs torch CPU SDPA(is_causal=True) — the S > 1 call of _torch.py:415 — on random bf16 q/K/V at
    S = 10, 77, 257, 807, 1300 (below/above the CPU flash kernel's query splits of 32/64/256, across 512-key blocks,
    ragged last tiles): bit-equal fraction > 0.99 for both kernels (matrix-core tiles at head size 128; the VALU
    kernel that serves the other head sizes), residual = fp32 summation order."""
    import torch.nn.functional as F
    model, _ = full
    eng = model.engine(1)
    eng.call("zn_debug_tune", _lib.ZN_TUNE_PREFILL_ATTN_VALU, kernel)
    st = _lib.stream_ptr()
    gen = torch.Generator().manual_seed(2)
    try:
        for S in (10, 77, 257, 807, 1300):
            cap = S + 5
            q = torch.randn(2, 16, S, 128, generator=gen).to(torch.bfloat16)
            kv = torch.randn(2, cap, 2, 4, 128, generator=gen).to(torch.bfloat16)
            ref = F.scaled_dot_product_attention(q, kv[:, :S, 0].transpose(1, 2), kv[:, :S, 1].transpose(1, 2), is_causal=True, enable_gqa=True)
            qd = q.transpose(1, 2).reshape(2, S, 2048).contiguous().to("cuda:0")
            kvd = kv.to("cuda:0")
            out = torch.full((2, S, 2048), float("nan"), dtype=torch.bfloat16, device="cuda:0")
            eng.call("zn_op_attn_prefill", qd.data_ptr(), kvd.data_ptr(), cap, out.data_ptr(), S, 2, st)
            torch.cuda.synchronize()
            got = out.cpu().view(2, S, 16, 128).transpose(1, 2).contiguous()
            eq = float((got.view(torch.int16) == ref.contiguous().view(torch.int16)).float().mean())
            print(f"\n[prefill attn kernel={kernel} S={S}] bit-equal {eq:.5f} max|d| {(got.float() - ref.float()).abs().max().item():.3g}")
            assert eq > 0.99, (S, eq)
    finally:
        eng.call("zn_debug_tune", _lib.ZN_TUNE_PREFILL_ATTN_VALU, 1)


@pytest.mark.parametrize("n_kv", [8, 4, 1], ids=["group1", "group2", "group8"])
def test_attention_other_group_sizes_vs_cpu_sdpa(n_kv):
    """Head size 128 with GQA groups of 1, 2 and 8 query heads per kv head (the checkpoints use 4): prefill attention on
    the matrix cores (64 / G positions per workgroup) and decode attention (both launch shapes) against torch CPU SDPA,
    same bit-equality bar as the group-4 tests."""
    import torch.nn.functional as F
    cfg = dict(d_model=1024, n_layer=1, num_heads=8, num_heads_kv=n_kv, d_ff=256)
    model, _ = build_model(cfg, 5, "cuda:0")
    eng = model.engine(1)
    st = _lib.stream_ptr()
    gen = torch.Generator().manual_seed(3)
    for S in (37, 300, 700):
        cap = S + 3
        q = torch.randn(2, 8, S, 128, generator=gen).to(torch.bfloat16)
        kv = torch.randn(2, cap, 2, n_kv, 128, generator=gen).to(torch.bfloat16)
        k, v = kv[:, :S, 0].transpose(1, 2), kv[:, :S, 1].transpose(1, 2)
        ref = F.scaled_dot_product_attention(q, k, v, is_causal=True, enable_gqa=True)
        qd = q.transpose(1, 2).reshape(2, S, 1024).contiguous().to("cuda:0")
        kvd = kv.to("cuda:0")
        out = torch.full((2, S, 1024), float("nan"), dtype=torch.bfloat16, device="cuda:0")
        eng.call("zn_op_attn_prefill", qd.data_ptr(), kvd.data_ptr(), cap, out.data_ptr(), S, 2, st)
        torch.cuda.synchronize()
        got = out.cpu().view(2, S, 8, 128).transpose(1, 2).contiguous()
        eq = float((got.view(torch.int16) == ref.contiguous().view(torch.int16)).float().mean())
        print(f"\n[prefill attn G={8 // n_kv} S={S}] bit-equal {eq:.5f}")
        assert eq > 0.99, (n_kv, S, eq)
        # decode: the last position alone over the same keys
        refd = F.scaled_dot_product_attention(q[:, :, -1:], k, v, enable_gqa=True)[:, :, 0]
        qd1 = q[:, :, -1].reshape(2, 1024).contiguous().to("cuda:0")
        lengths = torch.full((2,), S - 1, dtype=torch.int32, device="cuda:0")
        for fused_limit in (512, 1):                                     # S = 37, 300: the fused launch and the two passes; 700: two passes
            eng.call("zn_debug_tune", _lib.ZN_TUNE_ATTN_FUSED_MAX_KEYS, fused_limit)
            o1 = torch.empty(2, 1024, dtype=torch.bfloat16, device="cuda:0")
            eng.call("zn_op_attn_decode", qd1.data_ptr(), kvd.data_ptr(), cap, lengths.data_ptr(), None, o1.data_ptr(), 2, st)
            torch.cuda.synchronize()
            eqd = float((o1.cpu().view(2, 8, 128).view(torch.int16) == refd.contiguous().view(torch.int16)).float().mean())
            assert eqd > 0.99, (n_kv, S, fused_limit, eqd)
    eng.call("zn_debug_tune", _lib.ZN_TUNE_ATTN_FUSED_MAX_KEYS, 512)


def test_layer0_decode_vs_reference_block(golden_dir, full):
    """One decode step of block 0 at Zonos-v0.1-transformer dims over a synthetic KV history (L = 1, 17, 900):
    reference TransformerBlock output (golden) vs zn_op_layer_decode."""
    model, w = full
    g = _gold(golden_dir, "full_layer0")
    eng = model.engine(1)
    st = _lib.stream_ptr()
    for L in (1, 17, 900):
        x = synth.conditioning(1234, f"ops.x.{L}", 2, 1, 2048)[:, 0].contiguous().to("cuda:0")
        kv = torch.from_numpy(synth.normal(1234, f"ops.kv.{L}", (2, 904, 2, 4, 128))).to(torch.bfloat16).to("cuda:0")
        lengths = torch.full((2,), L - 1, dtype=torch.int32, device="cuda:0")
        eng.call("zn_op_layer_decode", 0, x.data_ptr(), kv.data_ptr(), 904, lengths.data_ptr(), None, 2, st)
        torch.cuda.synchronize()
        y = x.cpu().view(torch.int16).numpy().reshape(2, 1, 2048)
        ref = g[f"y_{L}"]
        knew = kv[:, L - 1, 0].contiguous().cpu().view(torch.int16).numpy()
        k_exact = float((knew == g[f"knew_{L}"]).mean())
        yf = torch.from_numpy(y).view(torch.bfloat16).float().numpy()
        rf = torch.from_numpy(ref).view(torch.bfloat16).float().numpy()
        exact = float((y == ref).mean())
        print(f"\n[layer0 L={L}] new-K bit-equal {k_exact:.5f}; output bit-equal {exact:.5f}; max|diff| {np.abs(yf - rf).max():.4g}")
        assert k_exact > 0.995
        assert exact > 0.9      # one-ulp flips from fp32 summation order propagate through out_proj x2 -> MLP
        assert np.abs(yf - rf).max() <= 2.0 ** -5 * max(1.0, np.abs(rf).max())


def test_layer0_per_op_bit_equality_vs_reference_block(golden_dir, full):
    """Where the one-ulp differences of a block come from (north_star bar 1 at the real dimensions): every op of reference
    TransformerBlock 0 fed with the REFERENCE's own input for that op (forward hooks on the reference's modules, recorded by
    tests/golden/make_golden.py --only ops), so that each op's own rounding disagreements show without the amplification of the
    ops before it.  LayerNorm: fp32 statistics + ((x - mean) * rstd) * g + b reproduce torch's CPU kernel to ~1e-5 of the elements
    (its (x * rstd + (-mean * rstd)) * g + b association differs on that order only: measured on the CPU).
    A GEMV's fp32 summation order differs from oneDNN's: ~1e-4 .. 1e-3 of its bf16 outputs land on the other side of a rounding
    boundary.  One flipped input of the next GEMV then moves ~2 % of ITS outputs by an ulp - which is how 99.9 % per op becomes
    93 - 99 % at the block's output (test_layer0_decode_vs_reference_block).  The floors below are the measured values minus a margin."""
    model, w = full
    g = _gold(golden_dir, "full_layer0")
    eng = model.engine(1)
    st = _lib.stream_ptr()
    dev = "cuda:0"
    p = "backbone.layers.0."
    W = {k: w[p + k].to(dev).contiguous() for k in ("norm.weight", "norm.bias", "norm2.weight", "norm2.bias", "mixer.in_proj.weight",
                                                    "mixer.out_proj.weight", "mlp.fc1.weight", "mlp.fc2.weight")}

    def bits(name, L):
        return torch.from_numpy(g[f"{name}_{L}"].astype(np.int16)).view(torch.bfloat16).reshape(2, -1).contiguous().to(dev)

    def linear(x, Wt, ln=None):
        out = torch.empty(2, Wt.shape[0], dtype=torch.bfloat16, device=dev)
        eng.call("zn_op_linear", x.data_ptr(), ln[0].data_ptr() if ln else None, ln[1].data_ptr() if ln else None, Wt.data_ptr(), out.data_ptr(),
                 2, Wt.shape[0], Wt.shape[1], st)
        return out

    def layernorm(x, wn, bn):
        out = torch.empty_like(x)
        eng.call("zn_op_layernorm", x.data_ptr(), wn.data_ptr(), bn.data_ptr(), out.data_ptr(), 2, x.shape[1], st)
        return out
    floors = {"n1": 0.9995, "qkv": 0.995, "o1": 0.995, "o2": 0.995, "n2": 0.9995, "u": 0.995, "f": 0.99}
    for L in (1, 17, 900):
        x = synth.conditioning(1234, f"ops.x.{L}", 2, 1, 2048)[:, 0].contiguous().to(dev)
        got = {
            "n1": layernorm(x, W["norm.weight"], W["norm.bias"]),
            "qkv": linear(bits("n1", L), W["mixer.in_proj.weight"]),                       # pre-RoPE q | k | v from the reference's n1
            "o1": linear(bits("a", L), W["mixer.out_proj.weight"]),
            "o2": linear(bits("o1", L), W["mixer.out_proj.weight"]),
            "n2": layernorm(bits("x1", L), W["norm2.weight"], W["norm2.bias"]),
            "u": linear(bits("n2", L), W["mlp.fc1.weight"]),
            "f": linear(bits("m", L), W["mlp.fc2.weight"]),
        }
        torch.cuda.synchronize()
        line = []
        for name, t in got.items():
            ref = bits(name, L)
            same = float((t.view(torch.int16) == ref.view(torch.int16)).float().mean())
            worst = float((t.float() - ref.float()).abs().max() / ref.float().abs().max().clamp_min(1e-6))
            line.append(f"{name} {same:.5f}")
            assert same >= floors[name], (L, name, same)
            assert worst <= 2.0 ** -7, (L, name, worst)                                     # never more than an ulp of the largest value
        print(f"\n[layer0 per-op, reference inputs, L={L}] bit-equal: " + "  ".join(line))


def test_layer0_16_row_path_per_op_vs_reference_block(golden_dir, full):
    """The 5..16-row kernels on the reference's recorded tensors of block 0, each op fed with the REFERENCE's input (the two recorded rows tiled
    to 16) through zn_op_linear_fused: in_proj with LayerNorm as gemm16k_kernel's prologue, out_proj twice, the out_proj -> fc1 pair with the
    LayerNorm statistics handed over (fc1 fed with the out kernel's own x1), fc2 through the split-K kernel.  Every output lies inside the
    float64 interval of zonos_amd.testing.linear_fused_reference, and the bit-equal share against the recorded tensor is at least the 2-row
    floor of test_layer0_per_op_bit_equality_vs_reference_block (qkv, o1, o2: 0.995; f: 0.99).  x1 and m have no 2-row entry there: their
    floors are the lowest shares measured on an MI355X over L = 1, 17, 900 minus 0.002 (profiles/linear_fused_gpu_tests.txt): x1 1.00000 -> 0.998,
    m 0.99951 -> 0.99751; the 2-row GEMV path on the same inputs, printed beside them, gives x1 1.00000 and m 0.99945."""
    import ctypes as C
    from zonos_amd import testing as T
    model, w = full
    g = _gold(golden_dir, "full_layer0")
    eng = model.engine(8)
    st = _lib.stream_ptr()
    dev = "cuda:0"
    p = "backbone.layers.0."
    Wc = {k: w[p + k].contiguous() for k in ("norm.weight", "norm.bias", "norm2.weight", "norm2.bias", "mixer.in_proj.weight", "mixer.out_proj.weight",
                                             "mlp.fc1.weight", "mlp.fc2.weight")}
    Wd = {k: v.to(dev) for k, v in Wc.items()}
    floors = {"qkv": 0.995, "o1": 0.995, "o2": 0.995, "f": 0.99, "x1": 0.998, "m": 0.99751}

    def fused(R, pro, epi, x, wname, ln=None, resid=None, want=0, have=0, expect=()):
        Wt = Wd[wname]
        N, K = Wt.shape
        out = torch.full((R, N // 2 if epi == T.LF_SILU else N), float("nan"), dtype=torch.bfloat16, device=dev)
        xd = x.to(dev).contiguous()
        keep = [xd, resid.to(dev).contiguous() if resid is not None else None]
        op = _lib.zn_linear_op(pro=pro, epi=epi, rows=R, N=N, K=K, target_blocks=512, want_ln_stats_out=want, ln_stats_in=have, x=xd.data_ptr(), W=Wt.data_ptr(),
                               out=out.data_ptr(), resid=keep[1].data_ptr() if resid is not None else None,
                               ln_w=Wd[ln + ".weight"].data_ptr() if ln else None, ln_b=Wd[ln + ".bias"].data_ptr() if ln else None)
        eng.call("zn_op_linear_fused", C.byref(op), st)
        torch.cuda.synchronize()
        plan = op.plan_dict()
        for k, v in expect:
            assert plan[k] == v, (wname, k, plan)
        ref = T.linear_fused_reference(pro, epi, Wc[wname], x=x, ln_w=Wc[ln + ".weight"] if ln else None, ln_b=Wc[ln + ".bias"] if ln else None, resid=resid,
                                       eps=eng.zc.norm_eps)
        got = out.cpu()
        res = T.linear_fused_compare(got, ref, f"layer 0, {R} rows, {wname} {plan['kernel']}")
        assert res.ok, (wname, res)
        return got

    def rec(name, L, R):
        t = torch.from_numpy(g[f"{name}_{L}"].astype(np.int16)).view(torch.bfloat16).reshape(2, -1)
        return t.repeat(R // 2, 1).contiguous()
    for R, L in [(16, L) for L in (1, 17, 900)] + [(2, L) for L in (1, 17, 900)]:      # (2 rows: the GEMV path on the same inputs, printed beside the 16-row shares)
        ex = (lambda *e: e) if R == 16 else (lambda *e: ())
        x = synth.conditioning(1234, f"ops.x.{L}", 2, 1, 2048)[:, 0].repeat(R // 2, 1).contiguous()
        got = {"qkv": fused(R, T.LF_PRO_LN, T.LF_STORE, x, "mixer.in_proj.weight", ln="norm", expect=ex(("kernel", "GEMM16K"), ("ln_pro", 1))),
               "o1": fused(R, T.LF_PRO_NONE, T.LF_STORE, rec("a", L, R), "mixer.out_proj.weight", expect=ex(("kernel", "GEMM16K"), ("nch", 2))),
               "o2": fused(R, T.LF_PRO_NONE, T.LF_STORE, rec("o1", L, R), "mixer.out_proj.weight", expect=ex(("kernel", "GEMM16K"))),
               "x1": fused(R, T.LF_PRO_NONE, T.LF_RESID, rec("o1", L, R), "mixer.out_proj.weight", resid=x, want=1,
                           expect=ex(("kernel", "GEMM16K"), ("writes_ln_stats", 1)))}
        got["m"] = fused(R, T.LF_PRO_LN, T.LF_SILU, got["x1"], "mlp.fc1.weight", ln="norm2", have=int(R == 16),
                         expect=ex(("kernel", "GEMM16S"), ("lnp", 1), ("reads_ln_stats", 1), ("ksplit", 1)))
        got["f"] = fused(R, T.LF_PRO_NONE, T.LF_STORE, rec("m", L, R), "mlp.fc2.weight", expect=ex(("kernel", "GEMM16S"), ("ksplit", 8)))
        line = []
        for name, t in got.items():
            same = float((t.view(torch.int16) == rec(name, L, R).view(torch.int16)).float().mean())
            line.append(f"{name} {same:.5f}")
            assert R != 16 or same >= floors[name], (L, name, same)
        print(f"\n[layer0 per-op, {R} rows, reference inputs, L={L}] bit-equal: " + "  ".join(line))


def test_full_dims_teacher_forced_vs_reference(golden_dir, full):
    model, _ = full
    g = _gold(golden_dir, "full_gen")
    cond = synth.conditioning(1234, "cond", 2, int(g["l_c"]), 2048)
    got = _teacher_forced(model, cond, int(g["max_new"]), g["inputs"])
    steps = g["logit_steps"]
    spread, flip = _ref_variation("gaussian")
    print(f"\n[full] the reference's own variation across host thread counts: max |dlogit| {spread}, largest margin of an argmax flip {flip}")
    _compare_logits(got[steps], g["logits"], g["margin"][steps], "full", tol=spread, dec=spread)       # |dlogit| <= the reference's own spread; argmax equal beyond it
    # greedy tokens of every step vs the reference's tokens, on decisive margins
    ref_tok = g["tokens"].astype(np.int64)              # [calls, 1, 9]
    bias_free = got.copy()
    ga = []
    inputs = g["inputs"].astype(np.int64)
    for k in range(got.shape[0]):
        lg = torch.from_numpy(bias_free[k])
        if k > 0:
            hist = torch.from_numpy(inputs[max(0, k - 2):k]).permute(1, 2, 0) if k >= 2 else torch.from_numpy(inputs[:k]).permute(1, 2, 0)
            lg = zo.repetition_penalty(lg, hist, 3.0, 2)
        ga.append(lg.argmax(-1).numpy())
    ga = np.stack(ga)
    decisive = g["margin"] > spread
    agree = (ga == ref_tok)
    worst = float(g["margin"][~agree].max()) if (~agree).any() else 0.0
    print(f"\n[full] greedy tokens equal on {agree.mean():.4f} of all (step,codebook); decisive (margin > {spread}) pairs {decisive.mean():.3f}; "
          f"largest reference margin of a HIP-vs-reference flip {worst} (the reference against itself: {flip})")
    assert agree[decisive].all()


def test_full_dims_free_running(golden_dir, full):
    """Zonos-v0.1-transformer dims, free-running greedy.  Gaussian-logit heads: reported (near-ties, see above).
    Peaky heads (decisive margins): indices must equal the reference's for a long prefix of the 160 frames."""
    model, _ = full
    g = _gold(golden_dir, "full_gen")
    cond = synth.conditioning(1234, "cond", 2, int(g["l_c"]), 2048)
    _free_run(model, cond, g, "full gaussian")
    gp = _gold(golden_dir, "full_gen_peaky")
    heads = torch.cat([torch.from_numpy(synth.peaky_heads(1234, f"heads.{i}.weight", 1025, 2048)).to(torch.bfloat16) for i in range(9)], 0)
    keep = model.fused_heads.weight.data.clone()
    try:
        model.fused_heads.weight.data.copy_(heads.to("cuda:0"))
        _free_run(model, cond, gp, "full peaky")
        # peaky logits reach |l| ~ 100-200 where one bf16 ulp is 0.5-1.0; the reference itself, run with another thread count, moves them by
        # up to `spread` and flips argmaxes at margins up to `flip`: "decisive" = margin > spread
        spread, flip = _ref_variation("peaky")
        print(f"\n[full peaky] the reference's own variation: max |dlogit| {spread}, largest margin of an argmax flip {flip}")
        agree, dec = _teacher_forced_tokens(model, cond, gp, dec_margin=spread)
    finally:
        model.fused_heads.weight.data.copy_(keep)
    assert agree > 0.95 and dec, (agree, dec)


def test_baseline_length_generation_properties(full):
    """BASELINE config 2 at full size (B = 1, L_c = 24, 861 new tokens, EOS suppressed: 868 decode steps through the fused
    and the two-pass attention launch shapes, 8-step and single-step graphs), checked through size-independent
    properties, since the oracle needs minutes for it: output shape and code range; run-to-run determinism; causality
    (a 200-token run of the same utterance reproduces the long run's frames, up to its last 8: there the upper codebooks'
    delayed columns are cut off by the end of the loop, the reference's own tail behaviour); the replayed multi-step graphs
    give the codes of single-step launches."""
    model, _ = full
    eng = model.engine(1)
    cond = synth.conditioning(1234, "cond", 2, 24, 2048).to("cuda:0")
    eng.call("zn_debug_eos_bias", float("-inf"))
    try:
        a = model.generate(cond, max_new_tokens=861, sampling_params=GREEDY)
        b = model.generate(cond, max_new_tokens=861, sampling_params=GREEDY)
        short = model.generate(cond, max_new_tokens=200, sampling_params=GREEDY)
        eng.call("zn_debug_tune", _lib.ZN_TUNE_GRAPH_RUNS, 1)                      # single-step launches only
        c = model.generate(cond, max_new_tokens=861, sampling_params=GREEDY)
    finally:
        eng.call("zn_debug_tune", _lib.ZN_TUNE_GRAPH_RUNS, 2)
        eng.call("zn_debug_eos_bias", 0.0)
    assert tuple(a.shape) == (1, 9, 861) and a.dtype == torch.int64
    assert int(a.min()) >= 0 and int(a.max()) <= 1023
    assert torch.equal(a, b)
    assert tuple(short.shape) == (1, 9, 200) and torch.equal(a[..., :192], short[..., :192])
    assert torch.equal(a[:, 0, :200], short[:, 0])       # codebook 0 is not delayed: equal to the end
    assert torch.equal(a, c)


def test_config5_long_prefix_prefill_vs_reference(golden_dir, full):
    """BASELINE config 5's prefill at full dims against the REFERENCE: a 30 s audio prefix (2584 codes) + 8 new tokens
    through the reference's own generate() (tests/golden/make_golden.py --only longfull).  Batched prefill over 24 + 2585
    positions (MFMA GEMMs + matrix-core causal attention), then decode steps at a 2.6 k context (split P.V pass),
    teacher-forced on the reference's inputs: logits within 0.1 (the full-dims bar), greedy index equal where the
    reference's margin is decisive."""
    import os
    path = f"{golden_dir}/full_gen_longprefix.npz"
    if not os.path.exists(path):
        pytest.skip("fixture full_gen_longprefix.npz not generated")
    model, _ = full
    g = np.load(path)
    P = int(g["prefix_len"])
    cond = synth.conditioning(1234, "cond", 2, int(g["l_c"]), 2048)
    pre = torch.from_numpy(synth.randint(1234, "longprefix", (1, 9, P), 1024)).to("cuda:0")
    got = _teacher_forced(model, cond, int(g["max_new"]), g["inputs"], prefix=pre)
    steps = g["logit_steps"]
    spread, _ = _ref_variation("gaussian")                 # the reference's own |dlogit| across host thread counts (64-step run at short contexts)
    _compare_logits(got[steps], g["logits"], g["margin"][steps], f"config5 prefix {P}", tol=spread, dec=spread)


def test_config5_longform_generation_properties(full):
    """BASELINE config 5 at full size (P = 2584 prefix codes + 2584 new tokens, context 5.2 k, EOS suppressed), through
    size-independent properties: shape / range, run-to-run determinism, the prefix is returned unchanged, causality (a
    run with fewer new tokens reproduces the long run's frames), and the whole-step kernel (attention workgroups per key block,
    6 blocks here) and the per-op launches (scores launch + per-block P.V launch) give the SAME logits under one token stream
    (one attention arithmetic on every path since round 4)."""
    model, _ = full
    eng = model.engine(1)
    P, N = 2584, 2584
    cond = synth.conditioning(1234, "cond", 2, 24, 2048).to("cuda:0")
    pre = torch.from_numpy(synth.randint(1234, "longprefix", (1, 9, P), 1024)).to("cuda:0")
    eng.call("zn_debug_eos_bias", float("-inf"))
    try:
        a = model.generate(cond, audio_prefix_codes=pre, max_new_tokens=N, sampling_params=GREEDY)
        b = model.generate(cond, audio_prefix_codes=pre, max_new_tokens=N, sampling_params=GREEDY)
        short = model.generate(cond, audio_prefix_codes=pre, max_new_tokens=200, sampling_params=GREEDY)
    finally:
        eng.call("zn_debug_eos_bias", 0.0)
    assert tuple(a.shape) == (1, 9, P + N) and int(a.min()) >= 0 and int(a.max()) <= 1023
    assert torch.equal(a[..., :P], pre.to(torch.int64))
    assert torch.equal(a, b)
    assert tuple(short.shape) == (1, 9, P + 200) and torch.equal(a[..., :P + 192], short[..., :P + 192])
    # whole-step kernel vs the per-op launches, same token stream
    toks = synth.randint(5, "c5.stream", (80, 1, 9), 1024).astype(np.int32)      # covers all 1 + 64 + 8 sampling calls
    out1, l1 = _override_generate(model, cond.cpu(), toks, 64, 1, prefix=pre)
    eng.call("zn_debug_tune", _lib.ZN_TUNE_PERSISTENT, 2)                            # per-op launches
    try:
        out2, l2 = _override_generate(model, cond.cpu(), toks, 64, 1, prefix=pre)
    finally:
        eng.call("zn_debug_tune", _lib.ZN_TUNE_PERSISTENT, 1)
    assert torch.equal(out1, out2)
    d = max(float(np.abs(np.where(np.isfinite(x), x - y, 0.0)).max()) for x, y in zip(l1, l2))
    print(f"\n[config 5] whole-step kernel vs per-op launches over 73 calls at context 2.6 k: max |dlogit| {d:.4g}")
    assert d == 0.0


def test_rope_table_limit_full_dims_properties(full):
    """Config 5's stress variant: max_seqlen = 16384, the RoPE table's limit (_torch.py:206), at full dims.
    KV capacity 16384 positions x 2 rows x 26 layers = 1.7 GB; prefill of 16344 positions then 32 new tokens.  Properties:
    shape, prefix returned unchanged, determinism, graph replay == single-step launches; one position more is refused."""
    model, _ = full
    eng = model.engine(1)
    N, L_c = 32, 24
    P = 16384 - L_c - 9 - N
    cond = synth.conditioning(1234, "cond", 2, L_c, 2048).to("cuda:0")
    pre = torch.from_numpy(synth.randint(1234, "limitprefix", (1, 9, P), 1024)).to("cuda:0")
    eng.call("zn_debug_eos_bias", float("-inf"))
    try:
        a = model.generate(cond, audio_prefix_codes=pre, max_new_tokens=N, sampling_params=GREEDY)
        b = model.generate(cond, audio_prefix_codes=pre, max_new_tokens=N, sampling_params=GREEDY)
        eng.call("zn_debug_tune", _lib.ZN_TUNE_GRAPH_RUNS, 1)
        c = model.generate(cond, audio_prefix_codes=pre, max_new_tokens=N, sampling_params=GREEDY)
        with pytest.raises(_lib.ZonosHipError, match="RoPE"):
            model.generate(cond, audio_prefix_codes=pre, max_new_tokens=N + 8, sampling_params=GREEDY)
    finally:
        eng.call("zn_debug_tune", _lib.ZN_TUNE_GRAPH_RUNS, 2)
        eng.call("zn_debug_eos_bias", 0.0)
    assert tuple(a.shape) == (1, 9, P + N) and torch.equal(a[..., :P], pre.to(torch.int64))
    assert torch.equal(a, b) and torch.equal(a, c)


def test_rope_table_limit_tiny_vs_oracle(tiny):
    """The same limit case on the tiny configuration, where the CPU oracle can follow: context 16384 (prefill of 16351
    positions, then 24 new tokens across the last 512-key block), oracle token stream fed through the override hook:
    output codes bit-equal, prefill logits and every 4th step's logits within 0.06, decisive argmax equal."""
    model, w, cond = tiny
    cfg = synth.TINY_CFG
    N, L_c = 24, 6
    P = 16384 - L_c - 9 - N
    pre = torch.from_numpy(synth.randint(8, "limit.tiny", (1, 9, P), 1024))
    otr = zo.GenTrace()
    noeos = lambda s_, l: l.index_fill(2, torch.tensor([1024]), -float("inf"))
    ref_out = zo.generate(w, cfg, cond, audio_prefix_codes=pre, max_new_tokens=N, sampling_params=GREEDY, trace=otr, logits_hook=noeos)
    toks = torch.stack(otr.tokens).numpy()
    out, logits = _override_generate(model, cond, toks, N, 1, prefix=pre.to("cuda:0"))
    assert torch.equal(out, ref_out)
    worst = 0.0
    for k in list(range(0, len(otr.logits), 4)) + [len(otr.logits) - 1]:
        a, b = logits[k], otr.logits[k].numpy()
        fin = np.isfinite(b)
        worst = max(worst, float(np.abs(np.where(fin, a - b, 0.0)).max()))
        t2 = np.sort(np.where(fin, b, -1e30), -1)[..., -2:]
        dec = (t2[..., 1] - t2[..., 0]) > 0.15
        assert (np.where(fin, a, -1e30).argmax(-1) == np.where(fin, b, -1e30).argmax(-1))[dec].all(), k
    print(f"\n[RoPE limit, tiny] context 16384: worst |dlogit| {worst:.4g}")
    assert worst <= 0.06


def test_sampler_transforms_vs_oracle(tiny):
    """Deterministic part of sample_from_logits (repetition penalty, softmax/T, unified, top-p, top-k, min-p) vs the
    oracle on seeded logits; tolerance 2e-6 absolute on probabilities (fp32, different exp/log implementations)."""
    import ctypes as C
    model, _, _ = tiny
    eng = model.engine(1)
    st = _lib.stream_ptr()
    lg = torch.from_numpy(synth.normal(99, "logits", (2, 9, 1025), 3.0))
    gen = torch.from_numpy(synth.randint(99, "gen", (2, 9, 7), 1025))
    gen[0, 0, -1] = gen[0, 0, -2]
    gen[1, 3, -1] = 1025
    lgd, gend = lg.to("cuda:0"), gen.to(torch.int32).to("cuda:0")
    cases = [dict(temperature=1.0, min_p=0.1), dict(temperature=0.7, linear=0.5, conf=0.4, quad=0.0),
             dict(temperature=1.0, top_p=0.8), dict(temperature=1.0, top_k=50), dict(temperature=1.3, top_p=0.9, top_k=100, min_p=0.05, linear=0.7, conf=-0.1, quad=0.2)]
    for c in cases:
        p = dict(temperature=1.0, top_p=0.0, top_k=0, min_p=0.0, linear=0.0, conf=0.0, quad=0.0)
        p.update(c)
        sp = _lib.zn_sampling(repetition_penalty=3.0, repetition_penalty_window=2, seed=5, **p)
        probs = torch.empty(2, 9, 1025, dtype=torch.float32, device="cuda:0")
        toks = torch.empty(2, 9, dtype=torch.int32, device="cuda:0")
        eng.call("zn_op_sample", lgd.data_ptr(), gend.data_ptr(), 7, C.byref(sp), 0, toks.data_ptr(), probs.data_ptr(), 2, st)
        torch.cuda.synchronize()
        ref = zo.filtered_probs(zo.repetition_penalty(lg, gen, 3.0, 2), p["temperature"], p["top_p"], p["top_k"], p["min_p"], p["linear"], p["conf"], p["quad"])
        err = (probs.cpu() - ref).abs().max().item()
        support_equal = bool(((probs.cpu() > 0) == (ref > 0)).all())
        print(f"\n[sampler {c}] max|dp| {err:.3g} support equal {support_equal}")
        assert err < 2e-6 and support_equal
        t = toks.cpu().long()
        assert bool((ref.gather(-1, t.unsqueeze(-1)) > 0).all())     # sampled tokens lie in the support
    # greedy with penalty: exact
    sp = _lib.zn_sampling(temperature=0.0, repetition_penalty=3.0, repetition_penalty_window=2, seed=1)
    toks = torch.empty(2, 9, dtype=torch.int32, device="cuda:0")
    eng.call("zn_op_sample", lgd.data_ptr(), gend.data_ptr(), 7, C.byref(sp), 0, toks.data_ptr(), None, 2, st)
    torch.cuda.synchronize()
    ref = zo.sample_from_logits(lg, temperature=0.0, generated_tokens=gen).squeeze(-1)
    assert torch.equal(toks.cpu().long(), ref)


def test_gumbel_draw_is_distributional(tiny):
    """Gumbel-max draw: empirical frequencies over 4000 draws vs the filtered probabilities (chi-square-like bound)."""
    import ctypes as C
    model, _, _ = tiny
    eng = model.engine(1)
    st = _lib.stream_ptr()
    lg = torch.zeros(1, 9, 1025)
    lg[..., :4] = torch.tensor([2.0, 1.0, 0.0, -1.0])
    lg[..., 4:] = -30.0
    sp = _lib.zn_sampling(temperature=1.0, repetition_penalty=1.0, repetition_penalty_window=2, seed=1234)
    d = lg.to("cuda:0")
    toks = torch.empty(1, 9, dtype=torch.int32, device="cuda:0")
    counts = torch.zeros(4)
    n = 450
    for i in range(n):
        eng.call("zn_op_sample", d.data_ptr(), None, 0, C.byref(sp), i, toks.data_ptr(), None, 1, st)
        counts += torch.bincount(toks.cpu().long().view(-1), minlength=1025)[:4].float()
    p = torch.softmax(lg[0, 0, :4], -1)
    freq = counts / counts.sum()
    print(f"\n[gumbel] expected {p.numpy().round(4)} observed {freq.numpy().round(4)} (n={int(counts.sum())})")
    assert (freq - p).abs().max() < 0.03


@pytest.mark.parametrize("B", [2, 3, 5, 8])
def test_batched_utterances_match_single_utterance_runs(B):
    """Batch semantics (the reference crashes for B >= 2, so the oracle is B independent batch-1
    runs): rows [cond_0..cond_{B-1}, uncond_0..uncond_{B-1}]; every utterance of a batched generate() must equal
    the same utterance generated alone (same kernels, same rounding), including ragged audio prefixes content."""
    model, _ = build_model(synth.TINY_CFG, 77, "cuda:0", peaky=True)
    d = synth.TINY_CFG["d_model"]
    conds = [synth.conditioning(100 + i, "cond", 2, 6, d) for i in range(B)]
    pre = torch.from_numpy(synth.randint(5, "bprefix", (B, 9, 4), 1024)).to("cuda:0")
    batched_cond = torch.cat([c[0:1] for c in conds] + [c[1:2] for c in conds], 0).to("cuda:0")
    out_b = model.generate(batched_cond, audio_prefix_codes=pre, max_new_tokens=20, batch_size=B, sampling_params=GREEDY).cpu()
    for i in range(B):
        solo = model.generate(conds[i].to("cuda:0"), audio_prefix_codes=pre[i:i + 1], max_new_tokens=20, batch_size=1, sampling_params=GREEDY).cpu()
        # output lengths can differ only through EOS, which greedy peaky runs of 20 tokens do not hit
        n = min(solo.shape[-1], out_b.shape[-1])
        same = (out_b[i, :, :n] == solo[0, :, :n]).float().mean().item()
        # B <= 2 shares the GEMV kernels with the solo run (bit-identical); B >= 3 runs the MFMA small-M path whose fp32
        # summation order differs, so near-ties may flip: require the first frames and most tokens to agree
        if B <= 2:
            assert same == 1.0, (i, same)
        else:
            assert torch.equal(out_b[i, :, :4], solo[0, :, :4]) and same > 0.6, (i, same)


def _override_generate(model, cond, toks, max_new, B, prefix=None):
    """generate() with the sampled tokens replaced by `toks` [calls, B, 9] (the oracle's), EOS suppressed; returns
    (codes, per-call logits)."""
    eng = model.engine(B)
    eng.call("zn_debug_eos_bias", float("-inf"))
    tk = torch.from_numpy(toks.astype(np.int32)).to("cuda:0").contiguous()
    eng.call("zn_debug_token_override", tk.data_ptr(), tk.shape[0])
    try:
        tr = {"logits": []}
        out = model.generate(cond.to("cuda:0"), audio_prefix_codes=prefix, max_new_tokens=max_new, batch_size=B, sampling_params=GREEDY, _trace=tr)
    finally:
        eng.call("zn_debug_token_override", None, 0)
        eng.call("zn_debug_eos_bias", 0.0)
    return out.cpu(), [l.cpu().numpy() for l in tr["logits"]]


@pytest.mark.parametrize("B", [2, 3, 8])
def test_batched_generate_vs_batched_oracle(B):
    """generate(batch_size=B) against the ORACLE's generate(batch_size=B) on the same B utterances (ragged-content audio
    prefixes), not against HIP solo runs: B = 2 -> 4 rows (GEMV), B = 3 -> 6 rows and B = 8 -> 16 rows (the small-M
    MFMA kernels gemm16s / gemm16k with their split-K tickets).  The oracle's token stream is fed through the
    override hook, so every call's logits are comparable: within 0.06, argmax equal on decisive margins, and the
    output codes (integer bookkeeping under that stream) bit-equal."""
    cfg = synth.TINY_CFG
    model, w = build_model(cfg, 77, "cuda:0")
    conds = [synth.conditioning(300 + i, "cond", 2, 6, cfg["d_model"]) for i in range(B)]
    cond = torch.cat([c[0:1] for c in conds] + [c[1:2] for c in conds], 0)
    pre = torch.from_numpy(synth.randint(9, "bo.prefix", (B, 9, 5), 1024))
    N = 40
    otr = zo.GenTrace()
    noeos = lambda s_, l: l.index_fill(2, torch.tensor([1024]), -float("inf"))
    ref_out = zo.generate(w, cfg, cond, audio_prefix_codes=pre, max_new_tokens=N, batch_size=B, sampling_params=GREEDY, trace=otr, logits_hook=noeos)
    toks = torch.stack(otr.tokens).numpy()                      # [calls, B, 9]
    out, logits = _override_generate(model, cond, toks, N, B, prefix=pre.to("cuda:0"))
    assert out.shape == ref_out.shape and torch.equal(out, ref_out)
    worst = 0.0
    for k in range(len(otr.logits)):
        a, b = logits[k], otr.logits[k].numpy()
        fin = np.isfinite(b)
        d = np.abs(np.where(fin, a - b, 0.0))
        worst = max(worst, float(d.max()))
        t2 = np.sort(np.where(fin, b, -1e30), -1)[..., -2:]
        dec = (t2[..., 1] - t2[..., 0]) > 0.15
        assert (np.where(fin, a, -1e30).argmax(-1) == np.where(fin, b, -1e30).argmax(-1))[dec].all(), k
    print(f"\n[batched B={B} vs batched oracle] {len(otr.logits)} calls, worst |dlogit| {worst:.4g}")
    assert worst <= 0.06


def test_full_dims_batch8_teacher_forced_vs_solo_runs(full):
    """BASELINE config 3's per-GPU share at the real dimensions: 8 utterances in one generate() (16 rows: the MFMA small-M
    projections, LayerNorm inside in_proj, 16-row attention) against the same utterances generated alone (2 rows: the
    GEMV kernels).  Same rounding points, different fp32 summation order: free-running, a near-tie (several of the 9
    top-2 margins per step lie within two bf16 ulps of a logit even for the decisive-margin heads) redirects a
    trajectory after a few frames, so the batched run is fed each solo run's tokens and the per-step logits are compared:
    within 2^-4.5 of the logit scale (a bf16 ulp is 0.5 at |l| ~ 100 and the heavy-tailed heads multiply a flipped hidden ulp
    by up to 20; the two runs also prefill through different kernels: 50 rows stream through gemm64s_kernel, 400 rows through
    the 128 x 128 GEMM), argmax equal wherever the solo margin exceeds twice that.  The comparison with the ORACLE at this
    size is test_full_dims_batch8_vs_batched_oracle below."""
    model, _ = full
    heads = torch.cat([torch.from_numpy(synth.peaky_heads(1234, f"heads.{i}.weight", 1025, 2048)).to(torch.bfloat16) for i in range(9)], 0)
    keep = model.fused_heads.weight.data.clone()
    B, T = 8, 16
    conds = [synth.conditioning(300 + i, "cond", 2, 24, 2048) for i in range(B)]
    batched = torch.cat([c[0:1] for c in conds] + [c[1:2] for c in conds], 0).to("cuda:0")
    try:
        model.fused_heads.weight.data.copy_(heads.to("cuda:0"))
        solo_logits, fed = [], []
        for i in range(B):
            tr = {"logits": [], "cols": []}
            tr["after_step"] = lambda step_idx, delayed, col, tr=tr: tr["cols"].append(delayed[:, :, col].clone())
            model.generate(conds[i].to("cuda:0"), max_new_tokens=T, batch_size=1, sampling_params=GREEDY, _trace=tr)
            solo_logits.append(torch.stack(tr["logits"]).cpu())          # [steps, 1, 9, V]
            fed.append(torch.stack(tr["cols"]))                           # [steps, 1, 9]: the column each step fed forward
        inp = torch.cat(fed, 1)                                           # [steps, B, 9]
        trb = {"logits": []}

        def hook(step_idx, delayed, col):                                  # first call: step_idx = -1 (after the prefill)
            if step_idx + 1 < inp.shape[0]:
                delayed[:, :, col] = inp[step_idx + 1]
        trb["after_step"] = hook
        model.generate(batched, max_new_tokens=T, batch_size=B, sampling_params=GREEDY, _trace=trb)
        got = torch.stack(trb["logits"]).cpu()                            # [steps, B, 9, V]
    finally:
        model.fused_heads.weight.data.copy_(keep)
    ref = torch.cat(solo_logits, 1)
    n = min(got.shape[0], ref.shape[0])
    got, ref = got[:n].numpy(), ref[:n].numpy()
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin)
    diff = np.abs(np.where(fin, got - ref, 0.0))
    scale = np.abs(ref[fin]).max()
    top2 = np.sort(np.where(fin, ref, -np.inf), -1)[..., -2:]
    margin = top2[..., 1] - top2[..., 0]
    same = np.where(fin, got, -np.inf).argmax(-1) == np.where(fin, ref, -np.inf).argmax(-1)
    tol = 2.0 ** -4.5 * scale
    print(f"\n[batch 8 vs solo, full dims, teacher-forced] {n} steps: exact logits {float((diff == 0).mean()):.4f}, max|diff| {diff.max():.3g}, "
          f"mean|diff| {diff.mean():.3g} (max|logit| {scale:.1f}, tol {tol:.2f}); argmax equal {same.mean():.4f}; "
          f"decisive pairs {float((margin > 2 * tol).mean()):.3f}")
    assert diff.max() <= tol, diff.max()
    assert same[margin > 2 * tol].all()


def test_full_dims_batch8_vs_batched_oracle(full):
    """BASELINE config 3's per-GPU share against the ORACLE at the real dimensions: generate(batch_size=8) (16 rows: gemm16s /
    gemm16k with their split-K tickets, LayerNorm inside in_proj, 16-row attention; prefill of 400 rows) vs the oracle's
    generate(batch_size=8) on the same 8 utterances, 6 new tokens (prefill + 13 decode steps), the oracle's token stream fed
    through the override hook: output codes bit-equal, every call's logits within 0.1 (the full-dims bar), greedy index
    equal wherever the oracle's margin is decisive."""
    model, w = full
    B, N = 8, 6
    conds = [synth.conditioning(500 + i, "cond", 2, 24, 2048) for i in range(B)]
    cond = torch.cat([c[0:1] for c in conds] + [c[1:2] for c in conds], 0)
    otr = zo.GenTrace()
    torch.set_num_threads(16)
    noeos = lambda s_, l: l.index_fill(2, torch.tensor([1024]), -float("inf"))
    ref_out = zo.generate(w, synth.FULL_CFG, cond, max_new_tokens=N, batch_size=B, sampling_params=GREEDY, trace=otr, logits_hook=noeos)
    toks = torch.stack(otr.tokens).numpy()
    out, logits = _override_generate(model, cond, toks, N, B)
    assert torch.equal(out, ref_out)
    worst, exact, tot = 0.0, 0, 0
    for k in range(len(otr.logits)):
        a, b = logits[k], otr.logits[k].numpy()
        fin = np.isfinite(b)
        d = np.abs(np.where(fin, a - b, 0.0))
        worst = max(worst, float(d.max()))
        exact += int((d == 0).sum())
        tot += d.size
        t2 = np.sort(np.where(fin, b, -1e30), -1)[..., -2:]
        dec = (t2[..., 1] - t2[..., 0]) > 0.2
        assert (np.where(fin, a, -1e30).argmax(-1) == np.where(fin, b, -1e30).argmax(-1))[dec].all(), k
    print(f"\n[batch 8 vs batched oracle, full dims] {len(otr.logits)} calls: exact logits {exact / tot:.4f}, worst |dlogit| {worst:.4g}")
    assert worst <= 0.1


@pytest.mark.parametrize("P", [3, 70, 250, 800])
def test_prefill_batched_and_positionwise_vs_oracle(tiny, P):
    """zn_prefill over S = L_c + P + 1 positions (S = 10, 77, 257, 807: below/above the CPU flash kernel's query splits
    of 32/64/256 and across a 512-key block) in both modes — batched (MFMA GEMMs + tiled causal attention) and position by
    position through the decode kernels — against the oracle: prefill logits within 0.06, the KV cache of the last
    layer bit-equal on > 97 % of entries, first greedy frame identical where the margin is decisive."""
    model, w, cond = tiny
    cfg = synth.TINY_CFG
    pre = torch.from_numpy(synth.randint(3, f"pf.prefix.{P}", (1, 9, P), 1024))
    # oracle prefill
    otr = zo.GenTrace()
    zo.generate(w, cfg, cond, audio_prefix_codes=pre, max_new_tokens=1, sampling_params=GREEDY, trace=otr)
    ref = otr.logits[0].numpy()
    eng = model.engine(1)
    got = {}
    for mode in (1, 0):
        eng.call("zn_debug_prefill_mode", mode)
        try:
            tr = {"logits": []}
            model.generate(cond.to("cuda:0"), audio_prefix_codes=pre.to("cuda:0"), max_new_tokens=1, sampling_params=GREEDY, _trace=tr)
            got[mode] = tr["logits"][0].cpu().numpy()
        finally:
            eng.call("zn_debug_prefill_mode", 1)
    for mode, name in ((1, "batched"), (0, "positionwise")):
        d = np.abs(got[mode] - ref)
        top2 = np.sort(ref, -1)[..., -2:]
        decisive = (top2[..., 1] - top2[..., 0]) > 0.15
        same = got[mode].argmax(-1) == ref.argmax(-1)
        print(f"\n[prefill P={P} {name}] max|dlogit| {d.max():.4g}, exact {np.mean(d == 0):.4f}, argmax equal {same.mean():.3f}")
        assert d.max() <= 0.06, (mode, P, d.max())
        assert same[decisive].all()


def test_embed_codes_bit_exact_vs_oracle(tiny):
    """K1 (codec_utils.py:37): sequential bf16 adds over the 9 codebooks, incl. EOS (1024) and MASK (1025) rows."""
    model, w, _ = tiny
    codes = torch.from_numpy(synth.randint(21, "embed.codes", (3, 9, 11), 1026))
    codes[0, :, 0] = 1025
    codes[1, 0, 3] = 1024
    got = model.embed_codes(codes.to("cuda:0")).cpu()
    ref = zo.embed_codes(w, codes)
    assert got.shape == ref.shape and torch.equal(got.view(torch.int16), ref.view(torch.int16))


def test_long_context_teacher_forced_vs_oracle(tiny):
    """Decode across the 512- and 1024-key block boundaries of the attention (context grows from 7 to ~1150): HIP logits
    vs the oracle under teacher forcing, every 64th step compared; tolerance 0.06, decisive argmax equal."""
    model, w, cond = tiny
    N = 1140
    otr = zo.GenTrace()
    ref_out = zo.generate(w, synth.TINY_CFG, cond, max_new_tokens=N, sampling_params=GREEDY, trace=otr,
                          logits_hook=lambda s, l: l.index_fill(2, torch.tensor([1024]), -float("inf")) if s >= 0 else l)
    # the oracle's per-step inputs = delayed codes; rebuild them from its raw tokens through the override hook
    toks = torch.stack(otr.tokens).numpy()            # [calls, 1, 9]
    eng = model.engine(1)
    eng.call("zn_debug_eos_bias", float("-inf"))
    tk = torch.from_numpy(toks.astype(np.int32)).to("cuda:0").contiguous()
    eng.call("zn_debug_token_override", tk.data_ptr(), tk.shape[0])
    try:
        tr = {"logits": []}
        out = model.generate(cond.to("cuda:0"), max_new_tokens=N, sampling_params=GREEDY, _trace=tr)
    finally:
        eng.call("zn_debug_token_override", None, 0)
        eng.call("zn_debug_eos_bias", 0.0)
    assert torch.equal(out.cpu(), ref_out)
    worst, checked = 0.0, 0
    for k in list(range(0, len(otr.logits), 64)) + [len(otr.logits) - 1, 510, 511, 512, 513, 1023, 1024, 1025]:
        if k >= len(otr.logits):
            continue
        a, b = tr["logits"][k].cpu().numpy(), otr.logits[k].numpy()
        fin = np.isfinite(b)
        d = np.abs(np.where(fin, a - b, 0.0)).max()
        worst = max(worst, float(d))
        t2 = np.sort(np.where(fin, b, -1e30), -1)[..., -2:]
        dec = (t2[..., 1] - t2[..., 0]) > 0.15
        assert (np.where(fin, a, -1e30).argmax(-1) == np.where(fin, b, -1e30).argmax(-1))[dec].all(), k
        checked += 1
    print(f"\n[long context] {checked} steps compared up to context {7 + N + 8}; worst |dlogit| {worst:.4g}")
    assert worst <= 0.06


def test_callback_stop_and_seeded_sampling(tiny):
    model, w, cond = tiny
    calls = []

    def cb(frame, step, max_steps):
        calls.append((step, max_steps))
        return step < 5                      # model.py:508: returning False stops the loop

    out = model.generate(cond.to("cuda:0"), max_new_tokens=40, sampling_params=GREEDY, callback=cb)
    ref = zo.generate(w, synth.TINY_CFG, cond, max_new_tokens=40, sampling_params=GREEDY, callback=lambda f, s, m: s < 5)
    assert calls[0] == (1, 48) and len(calls) == 5 and out.shape == ref.shape
    sp = dict(min_p=0.1)                     # the reference's default sampling_params (model.py:362)
    a = model.generate(cond.to("cuda:0"), max_new_tokens=30, sampling_params=sp, seed=7).cpu()
    b = model.generate(cond.to("cuda:0"), max_new_tokens=30, sampling_params=sp, seed=7).cpu()
    c = model.generate(cond.to("cuda:0"), max_new_tokens=30, sampling_params=sp, seed=8).cpu()
    assert torch.equal(a, b) and a.shape[:2] == (1, 9) and int(a.min()) >= 0 and int(a.max()) <= 1023
    assert a.shape != c.shape or not torch.equal(a, c)
    app = dict(top_p=0.9, top_k=200, min_p=0.02, linear=0.5, conf=0.4, quad=0.0)    # audio_generation_pipeline.py:151-158
    d = model.generate(cond.to("cuda:0"), max_new_tokens=30, sampling_params=app, seed=3).cpu()
    assert d.shape[:2] == (1, 9) and int(d.min()) >= 0 and int(d.max()) <= 1023


def test_errors_are_reported_not_crashes(tiny):
    model, _, cond = tiny
    with pytest.raises(AssertionError):
        model.generate(cond.to("cuda:0"), max_new_tokens=4, cfg_scale=1.0)                # model.py:399
    with pytest.raises(ValueError):
        model.generate(cond[:1].to("cuda:0"), max_new_tokens=4)                          # rows != 2 * batch_size
    with pytest.raises(TypeError):
        model.generate(cond.to("cuda:0"), max_new_tokens=4, sampling_params=dict(bogus=1))
    with pytest.raises(_lib.ZonosHipError):                                              # beyond the 16384-row RoPE table (_torch.py:206)
        model.generate(cond.to("cuda:0"), max_new_tokens=16400, sampling_params=GREEDY)


def test_small_m_projections_match_the_gemv_path(full):
    """16 activation rows through one block (LDS-staged MFMA projections, K split over workgroups, ticketed combine) vs
    the same rows two at a time (weight-streaming GEMV kernels): same rounding points, different fp32 summation order.
    New K/V bit-equal > 0.995, block output bit-equal > 0.9 and within 2^-5 of the output scale (the bar of the
    single-utterance block test)."""
    model, _ = full
    eng = model.engine(8)
    st = _lib.stream_ptr()
    L, max_len, R = 40, 64, 16
    x0 = synth.conditioning(99, "m16.x", R, 1, 2048)[:, 0].contiguous()
    kv0 = torch.from_numpy(synth.normal(99, "m16.kv", (R, max_len, 2, 4, 128))).to(torch.bfloat16)
    lengths = torch.full((R,), L - 1, dtype=torch.int32, device="cuda:0")
    for layer in (0, 7):
        xa, kva = x0.clone().to("cuda:0"), kv0.clone().to("cuda:0")
        eng.call("zn_op_layer_decode", layer, xa.data_ptr(), kva.data_ptr(), max_len, lengths.data_ptr(), None, R, st)
        xb, kvb = x0.clone().to("cuda:0"), kv0.clone().to("cuda:0")
        for r in range(0, R, 2):
            xs, ks = xb[r:r + 2].contiguous(), kvb[r:r + 2].contiguous()
            eng.call("zn_op_layer_decode", layer, xs.data_ptr(), ks.data_ptr(), max_len, lengths[r:r + 2].data_ptr(), None, 2, st)
            xb[r:r + 2], kvb[r:r + 2] = xs, ks
        torch.cuda.synchronize()
        ya, yb = xa.cpu(), xb.cpu()
        eq = float((ya.view(torch.int16) == yb.view(torch.int16)).float().mean())
        keq = float((kva[:, L - 1].cpu().view(torch.int16) == kvb[:, L - 1].cpu().view(torch.int16)).float().mean())
        md = (ya.float() - yb.float()).abs().max().item()
        print(f"\n[16 rows vs 8 x 2 rows, layer {layer}] new K/V bit-equal {keq:.5f}; output bit-equal {eq:.5f}, max|diff| {md:.4g}")
        assert keq > 0.995 and eq > 0.9
        assert md <= 2.0 ** -5 * max(1.0, yb.float().abs().max().item())


@pytest.mark.parametrize("R", [16, 10, 5, 24])
def test_fc1_layernorm_from_handed_over_statistics(full, R):
    """Rows 5..16: fc1's nn.LayerNorm (_torch.py:325, `norm2`) is not a launch - the second out_proj's epilogue leaves {sum, centred second
    moment} per row and 16-column tile, fc1 adds the tiles in a fixed order and normalises its activation chunks while staging them
    (gemm16s_kernel<EPI_SILU, ., true>).  Against the same block with layernorm_kernel in between (zn_debug_tune(ZN_TUNE_FC1_LN_LAUNCH, 2)): the statistics are
    the same numbers summed in another order (tile-wise instead of lane-wise), so the normalised rows may differ by a bf16 ulp here and
    there; block output bit-equal > 0.98 and within 2^-6 of its scale, new K/V (produced before the change) bit-equal; ragged row counts
    (10, 5: clamped rows of the last group; 24: two row groups per launch pair) included.  The batch-8 tests above hold the path against the oracle."""
    model, _ = full
    eng = model.engine(max(8, (R + 1) // 2))
    st = _lib.stream_ptr()
    L, max_len = 40, 64
    x0 = synth.conditioning(98, "lnp.x", R, 1, 2048)[:, 0].contiguous()
    x0 = (x0.float() * torch.linspace(0.5, 3.0, R)[:, None] + torch.linspace(-2.0, 2.0, R)[:, None]).to(torch.bfloat16)   # rows of different mean and scale
    kv0 = torch.from_numpy(synth.normal(98, "lnp.kv", (R, max_len, 2, 4, 128))).to(torch.bfloat16)
    lengths = torch.full((R,), L - 1, dtype=torch.int32, device="cuda:0")
    outs = {}
    try:
        for mode in (1, 2):
            eng.call("zn_debug_tune", _lib.ZN_TUNE_FC1_LN_LAUNCH, mode)
            xa, kva = x0.clone().to("cuda:0"), kv0.clone().to("cuda:0")
            for layer in (0, 11):
                eng.call("zn_op_layer_decode", layer, xa.data_ptr(), kva.data_ptr(), max_len, lengths.data_ptr(), None, R, st)
            torch.cuda.synchronize()
            outs[mode] = (xa.cpu(), kva[:, L - 1].cpu())
    finally:
        eng.call("zn_debug_tune", _lib.ZN_TUNE_FC1_LN_LAUNCH, 1)
    ya, yb = outs[1][0], outs[2][0]
    assert torch.isfinite(ya.float()).all()
    eq = float((ya.view(torch.int16) == yb.view(torch.int16)).float().mean())
    md = (ya.float() - yb.float()).abs().max().item()
    print(f"\n[fc1 LayerNorm from handed-over statistics vs the launch, {R} rows, two blocks] output bit-equal {eq:.5f}, max|diff| {md:.4g} (scale {yb.float().abs().max().item():.3g})")
    assert eq > 0.98 and md <= 2.0 ** -6 * max(1.0, yb.float().abs().max().item())


@pytest.mark.parametrize("rows", [5, 8, 13, 16])
def test_small_m_linear_shapes_vs_fp32_reference(tiny, rows):
    """zn_op_linear at 5..16 activation rows (the LDS-staged MFMA kernel: 32/64-row workgroups, K split over workgroups
    with the ticketed combine, clamped edge tiles; short slices fall back to the direct-fragment kernel) against an fp32
    matmul rounded once to bf16, over the projection shapes of both backbones plus ragged N: bit-equal > 0.98 (fp32
    summation order), never more than one bf16 ulp of the row scale apart."""
    model, _, _ = tiny
    eng = HipEngine(model.backbone, max_rows=16)
    st = _lib.stream_ptr()
    for N, K in ((2048, 2048), (3072, 2048), (8512, 2048), (9225, 2048), (16384, 2048), (2048, 4096), (2048, 8192), (1000, 512), (72, 256)):
        x = torch.from_numpy(synth.normal(5, f"lin.x.{N}.{K}.{rows}", (rows, K))).to(torch.bfloat16)
        W = torch.from_numpy(synth.uniform(5, f"lin.w.{N}.{K}", (N, K), 1.0 / np.sqrt(K))).to(torch.bfloat16)
        ref = (x.float() @ W.float().T).to(torch.bfloat16)
        xd, Wd = x.cuda(), W.cuda()
        out = torch.empty(rows, N, dtype=torch.bfloat16, device="cuda:0")
        eng.call("zn_op_linear", xd.data_ptr(), None, None, Wd.data_ptr(), out.data_ptr(), rows, N, K, st)
        torch.cuda.synchronize()
        got = out.cpu()
        eq = float((got.view(torch.int16) == ref.view(torch.int16)).float().mean())
        md = (got.float() - ref.float()).abs().max().item()
        print(f"\n[linear rows={rows} N={N} K={K}] bit-equal {eq:.5f} max|d| {md:.3g}")
        assert eq > 0.98 and md <= 2.0 ** -7 * max(1.0, ref.float().abs().max().item()), (N, K, eq, md)
