"""Generation without guidance (cfg_scale == 1): one row per utterance, no CFG mix.

The oracle asserts cfg_scale != 1 like the reference (model.py:399), but a guided run whose unconditional rows equal its conditional
rows gives exactly the conditional logits (tests/test_cfg1_cpu.py), so the unguided path on [c] is held to the unchanged oracle on
[c ‖ c] at cfg_scale=2 - and, at the real dimensions, bit for bit to the guided HIP run on [c ‖ c] and to the launches path."""
import threading

import numpy as np
import pytest
import torch

from oracle import zonos_oracle as zo
from zonos_amd import _lib, synth
from zonos_amd import conditioning as zc
from zonos_amd.testing import build_model

pytestmark = pytest.mark.gpu
GREEDY = {"temperature": 0.0}


def _noeos(s_, l):
    return l.index_fill(2, torch.tensor([1024]), -float("inf"))


def _override_generate(model, cond, toks, max_new, B, cfg_scale, prefix=None):
    """generate() with the sampled tokens replaced by `toks` [calls, B, 9] (the oracle's), EOS suppressed; returns (codes, per-call
    logits).  The engine is the one generate() picks for this many rows (engine(b) holds 2 b rows)."""
    eng = model.engine((cond.shape[0] + 1) // 2)
    eng.call("zn_debug_eos_bias", float("-inf"))
    tk = torch.from_numpy(toks.astype(np.int32)).to("cuda:0").contiguous()
    eng.call("zn_debug_token_override", tk.data_ptr(), tk.shape[0])
    try:
        tr = {"logits": []}
        out = model.generate(cond.to("cuda:0"), audio_prefix_codes=prefix, max_new_tokens=max_new, batch_size=B, cfg_scale=cfg_scale,
                             sampling_params=GREEDY, _trace=tr)
    finally:
        eng.call("zn_debug_token_override", None, 0)
        eng.call("zn_debug_eos_bias", 0.0)
    return out.cpu(), [l.cpu().numpy() for l in tr["logits"]]


def _vs_oracle(logits, otr, tol, dec):
    worst = 0.0
    for k in range(len(otr.logits)):
        a, b = logits[k], otr.logits[k].numpy()
        fin = np.isfinite(b)
        d = np.abs(np.where(fin, a - np.where(fin, b, 0.0), 0.0))
        worst = max(worst, float(d.max()))
        t2 = np.sort(np.where(fin, b, -1e30), -1)[..., -2:]
        decisive = (t2[..., 1] - t2[..., 0]) > dec
        assert (np.where(fin, a, -1e30).argmax(-1) == np.where(fin, b, -1e30).argmax(-1))[decisive].all(), k
    return worst


# ------------------------------------------------------------------------------------------------ (a) tiny, against the oracle
@pytest.mark.parametrize("B", [1, 3, 5])
def test_tiny_unguided_vs_oracle_on_doubled_rows(B):
    """B unguided utterances = B rows (1: the GEMV kernels; 3, 5: odd row counts on the small-M MFMA path) against the oracle's guided
    run on [c_0..c_{B-1} ‖ c_0..c_{B-1}], the oracle's tokens fed back: codes equal, logits within 0.06, decisive argmax equal."""
    cfg = synth.TINY_CFG
    model, w = build_model(cfg, 77, "cuda:0")
    c = torch.cat([synth.conditioning(700 + i, "cond", 1, 6, cfg["d_model"]) for i in range(B)], 0)
    pre = torch.from_numpy(synth.randint(9, "cfg1.prefix", (B, 9, 5), 1024))
    N = 40
    otr = zo.GenTrace()
    ref_out = zo.generate(w, cfg, torch.cat([c, c], 0), audio_prefix_codes=pre, max_new_tokens=N, cfg_scale=2.0, batch_size=B,
                          sampling_params=GREEDY, trace=otr, logits_hook=_noeos)
    toks = torch.stack(otr.tokens).numpy()
    out, logits = _override_generate(model, c, toks, N, B, 1.0, prefix=pre.to("cuda:0"))
    assert out.shape == ref_out.shape and torch.equal(out, ref_out)
    worst = _vs_oracle(logits, otr, 0.06, 0.15)
    print(f"\n[tiny unguided B={B} vs oracle on [c ‖ c]] {len(otr.logits)} calls, worst |dlogit| {worst:.4g}")
    assert worst <= 0.06


# ------------------------------------------------------------------------------------------------ (b) full dims, one row
@pytest.fixture(scope="module")
def full():
    model, w = build_model(synth.FULL_CFG, 1234, "cuda:0")
    return model, w


def _traced(model, cond, pre, new, cfg_scale, B=1):
    tr = {"logits": []}
    o = model.generate(cond, audio_prefix_codes=pre, max_new_tokens=new, cfg_scale=cfg_scale, batch_size=B, sampling_params=GREEDY, _trace=tr)
    return o.cpu(), torch.stack(tr["logits"]).cpu()


@pytest.mark.parametrize("prefix,new", [(0, 40), (480, 48), (3040, 48), (4060, 48), (6100, 40)])
def test_full_dims_one_row_kernel_is_bit_identical(full, prefix, new):
    """One unguided utterance at the Zonos-v0.1 dimensions runs the one-row whole-step kernel (zn_decode_path_detail == 2) up to 6144
    keys and the launches path beyond.  Codes and every traced step's logits are bit-identical to (i) the launches path at one row
    (zn_debug_tune(ZN_TUNE_PERSISTENT, 2)) and (ii) the guided run on [c ‖ c] at cfg_scale=2 (the two-row kernel); contexts from 26 keys, across
    512 keys, the 3072- and 4096-key changes of instantiation and 6144 keys; 8-step graphs; no hand-off timeout; a second run equal."""
    model, _ = full
    eng = model.engine(1)
    c = synth.conditioning(1234, "cond", 1, 24, 2048).to("cuda:0")
    pre = torch.from_numpy(synth.randint(1234, f"cfg1.prefix{prefix}", (1, 9, prefix), 1024)).to("cuda:0") if prefix else None
    try:
        eng.call("zn_debug_eos_bias", float("-inf"))
        t0 = eng.counters()["handoff_timeouts"]
        o1, l1 = _traced(model, c, pre, new, 1.0)
        end_ctx = 24 + prefix + 1 + new + 9
        assert eng.lib.zn_decode_path_detail(eng.h) == (2 if end_ctx + 8 <= 6144 else 0), eng.lib.zn_decode_path_detail(eng.h)
        o1b, l1b = _traced(model, c, pre, new, 1.0)
        o2, l2 = _traced(model, torch.cat([c, c], 0), pre, new, 2.0)
        eng.call("zn_debug_tune", _lib.ZN_TUNE_PERSISTENT, 2)
        o3, l3 = _traced(model, c, pre, new, 1.0)
        assert eng.lib.zn_decode_path_detail(eng.h) == 0
        eng.call("zn_debug_tune", _lib.ZN_TUNE_PERSISTENT, 1)
        assert o1.shape[-1] == prefix + new
        for o, l in ((o1b, l1b), (o2, l2), (o3, l3)):
            assert torch.equal(o, o1)
            assert l.shape == l1.shape and torch.equal(l.view(torch.int32), l1.view(torch.int32))
        # untraced runs replay 8-step graphs
        plain = [model.generate(cc, audio_prefix_codes=pre, max_new_tokens=new, cfg_scale=s, sampling_params=GREEDY).cpu()
                 for cc, s in ((c, 1.0), (torch.cat([c, c], 0), 2.0))]
        assert torch.equal(plain[0], o1) and torch.equal(plain[1], o1)
        assert eng.counters()["handoff_timeouts"] == t0
    finally:
        eng.call("zn_debug_tune", _lib.ZN_TUNE_PERSISTENT, 1)
        eng.call("zn_debug_eos_bias", 0.0)


# ------------------------------------------------------------------------------------------------ (c) two unguided utterances
def test_full_dims_two_unguided_rows_match_one_row_runs(full):
    """B = 2 without guidance fills the two rows of the two-row whole-step kernel; each row's codes and logits are bit-identical to
    a one-row run of its conditioning."""
    model, _ = full
    cs = [synth.conditioning(1300 + i, "cond", 1, 24, 2048).to("cuda:0") for i in range(2)]
    eng = model.engine(1)
    T = 24
    o2, l2 = _traced(model, torch.cat(cs, 0), None, T, 1.0, B=2)
    assert eng.lib.zn_decode_path_detail(eng.h) == 2
    for i in range(2):
        o1, l1 = _traced(model, cs[i], None, T, 1.0)
        n = min(o1.shape[-1], o2.shape[-1])
        assert torch.equal(o2[i:i + 1, :, :n], o1[:, :, :n]), i
        k = min(l1.shape[0], l2.shape[0])
        assert torch.equal(l2[:k, i:i + 1].contiguous().view(torch.int32), l1[:k].contiguous().view(torch.int32)), i


# ------------------------------------------------------------------------------------------------ (d) batches at full dims
def test_full_dims_batch8_unguided_vs_batched_oracle_and_batch16(full):
    """8 unguided utterances (8 rows) against the batched oracle on [c_0..c_7 ‖ c_0..c_7] (test_full_dims_batch8_vs_batched_oracle's
    protocol and 0.1 bar); then 16 unguided utterances on [c_0..c_7, c_0..c_7] against the guided batch of 8 on [c_0..c_7 ‖ c_0..c_7]:
    the 16-row kernels see identical inputs in both runs, so rows b and b + 8 equal each other and the guided run bit for bit."""
    model, w = full
    B, N = 8, 6
    c = torch.cat([synth.conditioning(500 + i, "cond", 1, 24, 2048) for i in range(B)], 0)
    otr = zo.GenTrace()
    torch.set_num_threads(16)
    ref_out = zo.generate(w, synth.FULL_CFG, torch.cat([c, c], 0), max_new_tokens=N, cfg_scale=2.0, batch_size=B, sampling_params=GREEDY,
                          trace=otr, logits_hook=_noeos)
    toks = torch.stack(otr.tokens).numpy()
    out, logits = _override_generate(model, c, toks, N, B, 1.0)
    assert torch.equal(out, ref_out)
    worst = _vs_oracle(logits, otr, 0.1, 0.2)
    print(f"\n[batch 8 unguided vs batched oracle on [c ‖ c], full dims] {len(otr.logits)} calls, worst |dlogit| {worst:.4g}")
    assert worst <= 0.1
    cd = c.to("cuda:0")
    T = 16
    o16, l16 = _traced(model, torch.cat([cd, cd], 0), None, T, 1.0, B=16)
    og, lg = _traced(model, torch.cat([cd, cd], 0), None, T, 2.0, B=8)
    n = min(o16.shape[-1], og.shape[-1])
    k = min(l16.shape[0], lg.shape[0])
    for half in (0, 8):
        assert torch.equal(o16[half:half + 8, :, :n], og[:, :, :n]), half
        assert torch.equal(l16[:k, half:half + 8].contiguous().view(torch.int32), lg[:k].contiguous().view(torch.int32)), half


# ------------------------------------------------------------------------------------------------ (e) hybrid
@pytest.mark.parametrize("B", [1, 3])
def test_hybrid_tiny_unguided_vs_oracle_on_doubled_rows(B):
    """The hybrid stack (Mamba2 state and KV caches of R = B rows, odd included) without guidance against the oracle's guided run on
    [c ‖ c]: codes equal under the oracle's token stream, logits within 0.06, decisive argmax equal."""
    cfg = synth.HYBRID_TINY_CFG
    model, sd = build_model(cfg, 21, "cuda:0")
    c = torch.cat([synth.conditioning(900 + i, "cond", 1, 7, cfg["d_model"]) for i in range(B)], 0)
    N = 24
    otr = zo.GenTrace()
    ref_out = zo.generate(sd, dict(cfg), torch.cat([c, c], 0), max_new_tokens=N, cfg_scale=2.0, batch_size=B, sampling_params=GREEDY,
                          trace=otr, logits_hook=_noeos)
    toks = torch.stack(otr.tokens).numpy()
    out, logits = _override_generate(model, c, toks, N, B, 1.0)
    assert torch.equal(out, ref_out)
    worst = _vs_oracle(logits, otr, 0.06, 0.12)
    print(f"\n[hybrid tiny unguided B={B} vs oracle on [c ‖ c]] {len(otr.logits)} calls, worst |dlogit| {worst:.4g}")
    assert worst <= 0.06


# ------------------------------------------------------------------------------------------------ (f) the public surface
def test_public_surface_without_guidance(golden_dir):
    """prepare_conditioning at its default cfg_scale=1.0 feeds generate(cfg_scale=1.0); seeded min_p sampling is deterministic; a callback
    stops the run; the row checks keep their error types; an unguided and a guided request on two threads equal their solo runs."""
    g = np.load(f"{golden_dir}/conditioner.npz")
    cfg = synth.TINY_CFG
    model, _ = build_model(cfg, int(g["d128_none_seed"]), "cuda:0", conditioners=synth.TRANSFORMER_CONDITIONERS, projection="none")
    spk = torch.from_numpy(synth.normal(77, "cond.speaker", (1, 1, 128))).to(torch.bfloat16)
    cd = zc.make_cond_dict(device="cuda:0", text="ignored", language="en-us", speaker=spk, emotion=[0.5, 0.05, 0.05, 0.05, 0.05, 0.05, 0.1, 0.15],
                           fmax=22050.0, pitch_std=45.0, speaking_rate=13.0)
    cd["espeak"] = ("ids", torch.from_numpy(g["d128_none_ids"]))
    cond = model.prepare_conditioning(cd)
    assert cond.shape[0] == 1
    out = model.generate(cond, max_new_tokens=30, cfg_scale=1.0, sampling_params=GREEDY)
    assert out.shape[:2] == (1, 9) and out.shape[2] > 0 and int(out.min()) >= 0 and int(out.max()) <= 1023
    a = model.generate(cond, max_new_tokens=30, cfg_scale=1.0, sampling_params=dict(min_p=0.1), seed=5).cpu()
    b = model.generate(cond, max_new_tokens=30, cfg_scale=1.0, sampling_params=dict(min_p=0.1), seed=5).cpu()
    assert torch.equal(a, b) and a.shape[:2] == (1, 9) and int(a.min()) >= 0 and int(a.max()) <= 1023
    seen = []

    def stop_at_5(frame, step, max_steps):
        seen.append(step)
        return step < 5
    short = model.generate(cond, max_new_tokens=30, cfg_scale=1.0, sampling_params=GREEDY, callback=stop_at_5)
    assert seen[-1] == 5 and short.shape[:2] == (1, 9)
    c2 = torch.cat([cond, cond], 0)
    with pytest.raises(AssertionError):
        model.generate(c2, max_new_tokens=4, cfg_scale=1.0)
    with pytest.raises(ValueError):
        model.generate(cond, max_new_tokens=4, cfg_scale=2.0)
    guided_cond = model.prepare_conditioning(cd, cfg_scale=2.0)
    solo_u = model.generate(cond, max_new_tokens=24, cfg_scale=1.0, sampling_params=GREEDY).cpu()
    solo_g = model.generate(guided_cond, max_new_tokens=24, cfg_scale=2.0, sampling_params=GREEDY).cpu()
    res, errs = {}, []
    start = threading.Barrier(2)

    def run(name, cnd, s):
        try:
            start.wait()
            res[name] = model.generate(cnd, max_new_tokens=24, cfg_scale=s, sampling_params=GREEDY).cpu()
        except Exception as e:          # noqa: BLE001 - reported below
            errs.append(e)
    th = [threading.Thread(target=run, args=("u", cond, 1.0)), threading.Thread(target=run, args=("g", guided_cond, 2.0))]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not errs, errs
    assert torch.equal(res["u"], solo_u) and torch.equal(res["g"], solo_g)
