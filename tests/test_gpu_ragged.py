"""Utterances of different prompt lengths in one generate() call (`conditioning_lengths`, zn_prefill_rows).

Rows are right-padded; the padding is never visible to a result, and every utterance gets what it would get in a batch of utterances
of its own length.  Bit-identity is asserted wherever the two sides run the same kernels; the oracle comparison carries the bound of
tests/test_gpu_decode.py::test_batched_generate_vs_batched_oracle (0.06 on the tiny configuration)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import zonos_oracle as zo
from zonos_amd import _lib, synth
from zonos_amd.conditioning import pad_conditionings
from zonos_amd.model import _sampling_struct
from zonos_amd.testing import build_model

pytestmark = pytest.mark.gpu
GREEDY = {"temperature": 0.0}
DEV = "cuda:0"
CFGS = {"transformer": synth.TINY_CFG, "hybrid": synth.HYBRID_TINY_CFG}


@pytest.fixture(scope="module")
def models():
    built = {}

    def get(name):
        if name not in built:
            built[name] = build_model(CFGS[name], 77 if name == "transformer" else 23, DEV, peaky=True)
        return built[name]
    return get


@pytest.fixture(scope="module")
def full():
    model, w = build_model(synth.FULL_CFG, 1234, DEV)
    return model, w


def _utterances(lengths, d, seed0, halves=2):
    return [synth.conditioning(seed0 + i, "ragged.cond", halves, L, d) for i, L in enumerate(lengths)]


def _rows(conds):
    """generate()'s batch layout for conditionings of one length."""
    halves = conds[0].shape[0]
    return torch.cat([c[h:h + 1] for h in range(halves) for c in conds], 0)


def _run(model, cond, B, max_new, lengths=None, prefix=None, cfg_scale=2.0):
    """Greedy generate() with EOS suppressed (every run keeps all max_new frames); returns (codes, per-call logits [calls, B, 9, 1025])."""
    eng = model.engine(B)
    eng.call("zn_debug_eos_bias", float("-inf"))
    try:
        tr = {"logits": []}
        kw = {} if lengths is None else {"conditioning_lengths": lengths}
        out = model.generate(cond.to(DEV), audio_prefix_codes=prefix, max_new_tokens=max_new, batch_size=B, cfg_scale=cfg_scale,
                             sampling_params=GREEDY, _trace=tr, **kw)
    finally:
        eng.call("zn_debug_eos_bias", 0.0)
    assert eng.counters()["handoff_timeouts"] == 0
    return out.cpu(), torch.stack([l.cpu() for l in tr["logits"]])


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _gemm_class(M):
    """The prefill projections' kernel is chosen by M = R * S (zn_linear_plan.h: plan_linear's gemm16k / gemm64s kernels up to 64 rows, launch_gemm's
    plain kernel up to 255, its LDS-staged one from 256)."""
    return 0 if M <= 64 else 1 if M <= 255 else 2


# ------------------------------------------------------------------------------------------------ 1. equal lengths are the old call
@pytest.mark.parametrize("arch", ["transformer", "hybrid"])
@pytest.mark.parametrize("B,cfg_scale", [(1, 2.0), (2, 1.0), (3, 2.0), (8, 2.0)], ids=["B1-guided", "B2-unguided", "B3", "B8"])
def test_equal_lengths_are_the_call_without_lengths(models, arch, B, cfg_scale):
    model, _ = models(arch)
    d, L = CFGS[arch]["d_model"], 7
    cond = _rows(_utterances([L] * B, d, 500, halves=1 if cfg_scale == 1 else 2))
    pre = torch.from_numpy(synth.randint(3, "ragged.prefix", (B, 9, 3), 1024)).to(DEV)
    base = _run(model, cond, B, 12, prefix=pre, cfg_scale=cfg_scale)
    same = _run(model, cond, B, 12, lengths=[L] * B, prefix=pre, cfg_scale=cfg_scale)
    assert torch.equal(base[0], same[0]) and _same_bits(base[1], same[1])


# ------------------------------------------------------------------------------------------------ 2. padding is never read
@pytest.mark.parametrize("arch", ["transformer", "hybrid"])
@pytest.mark.parametrize("cfg_scale", [2.0, 1.0], ids=["guided", "unguided"])
def test_padding_is_never_read(models, arch, cfg_scale):
    """The same ragged call with zeros and with +-1e4 in the pad region of prefix_conditioning: bit-identical codes and logits.  (NaN
    padding is not asserted: the pad positions' activations pass through the row-wise kernels and land in cache slots that are overwritten
    before they are read, so nothing known reads them, but that has not been measured.)"""
    model, _ = models(arch)
    d, lengths = CFGS[arch]["d_model"], [9, 4, 12, 6]
    B = len(lengths)
    cond, lens = pad_conditionings(_utterances(lengths, d, 520, halves=1 if cfg_scale == 1 else 2), cfg_scale)
    loud = cond.clone()
    sign = torch.from_numpy(synth.randint(7, "ragged.sign", tuple(cond.shape), 2)).to(cond.dtype) * 2 - 1
    for r in range(cond.shape[0]):
        loud[r, lens[r % B]:] = 1e4 * sign[r, lens[r % B]:]
    assert not torch.equal(loud, cond)
    pre = torch.from_numpy(synth.randint(3, "ragged.prefix", (B, 9, 2), 1024)).to(DEV)
    quiet = _run(model, cond, B, 12, lengths=lens, prefix=pre, cfg_scale=cfg_scale)
    noisy = _run(model, loud, B, 12, lengths=lens, prefix=pre, cfg_scale=cfg_scale)
    assert torch.equal(quiet[0], noisy[0]) and _same_bits(quiet[1], noisy[1])


# ------------------------------------------------------------------------------------------------ 3. a row does not depend on its batch-mates' lengths
def _check_rows_against_uniform_batches(model, d, lengths, P, max_new, cfg_scale=2.0, seed0=540, same_class=True):
    """Row i of the ragged batch == row i of the uniform call on B utterances of length L_i with utterance i in slot i (the other slots hold
    other utterances of that length)."""
    B, halves = len(lengths), 1 if cfg_scale == 1 else 2
    R = halves * B
    utts = _utterances(lengths, d, seed0, halves)
    cond, lens = pad_conditionings(utts, cfg_scale)
    pre = torch.from_numpy(synth.randint(3, "ragged.prefix", (B, 9, P), 1024)).to(DEV) if P else None
    if same_class:
        classes = {_gemm_class(R * (L + P + 1)) for L in lengths}
        assert len(classes) == 1, f"the ragged call (M = {R * (max(lengths) + P + 1)}) and the uniform calls must run one projection kernel class: {classes}"
    codes, logits = _run(model, cond, B, max_new, lengths=lens, prefix=pre, cfg_scale=cfg_scale)
    for i, L in enumerate(lengths):
        mates = _utterances([L] * B, d, seed0 + 100 * (i + 1), halves)
        mates[i] = utts[i]
        ucodes, ulogits = _run(model, _rows(mates), B, max_new, prefix=pre, cfg_scale=cfg_scale)
        assert _same_bits(logits[:, i], ulogits[:, i]), f"utterance {i} (length {L}): logits differ from the uniform batch's"
        assert torch.equal(codes[i], ucodes[i]), f"utterance {i} (length {L}): codes differ"


@pytest.mark.parametrize("arch", ["transformer", "hybrid"])
@pytest.mark.parametrize("lengths,P", [([4, 6, 8], 0), ([27, 12, 21, 17], 3), ([100, 200], 0), ([150, 800, 420], 0)],
                         ids=["B3-short", "B4-prefix", "qsplit-32-64", "qsplit-32-256-64"])
def test_rows_do_not_depend_on_batch_mates_lengths(models, arch, lengths, P):
    """Guided batches.  [4, 6, 8] without a prefix: M = 6 S <= 54 rows (the short-prompt kernels).  [27, 12, 21, 17] with a 3-frame
    prefix: M = 8 S in 128 .. 248 (the plain MFMA GEMM).  [100, 200]: S = 101 < 192 <= 201, query split 32 against 64, both M >= 256 - this
    case fails if the split is taken from the longest row.  [150, 800, 420]: splits 32 / 256 / 64.  The transformer cases assert that the
    ragged call and every uniform call fall in one projection-kernel class; the hybrid backbone prefills in mode 2 (projections row by
    row through the step's GEMV: independent of M), with two lengths in the last case to keep its launch count moderate."""
    model, _ = models(arch)
    if arch == "hybrid" and len(lengths) == 3 and max(lengths) > 300:
        lengths = [150, 420]
    eng = model.engine(len(lengths))
    if arch == "hybrid":
        eng.call("zn_debug_prefill_mode", 2)
    try:
        _check_rows_against_uniform_batches(model, CFGS[arch]["d_model"], lengths, P, 8, same_class=arch == "transformer")
    finally:
        eng.call("zn_debug_prefill_mode", 1)


def test_full_dims_batch8_rows_do_not_depend_on_batch_mates_lengths(full):
    """Zonos-v0.1 dimensions (head size 128: the matrix-core prefill attention), B = 8 guided, lengths over 18 .. 40: M = 16 S >= 304."""
    model, _ = full
    _check_rows_against_uniform_batches(model, synth.FULL_CFG["d_model"], [40, 18, 33, 25, 21, 37, 29, 19], 0, 6, seed0=560)


# ------------------------------------------------------------------------------------------------ 4. against the oracle
@pytest.mark.parametrize("B", [3, 8])
def test_ragged_batch_vs_solo_oracle_runs(models, B):
    """The oracle generates every utterance alone; its B token streams, stacked, drive the ragged batched call through the override hook.
    Every call's logits of row i within 0.06 of solo run i, argmax equal where the oracle's top-2 margin exceeds 0.15, codes bit-equal."""
    cfg = synth.TINY_CFG
    model, w = build_model(cfg, 77, DEV)
    lengths = [6, 11, 4, 9, 14, 5, 8, 12][:B]
    utts = _utterances(lengths, cfg["d_model"], 600)
    pre = torch.from_numpy(synth.randint(9, "ragged.oprefix", (B, 9, 5), 1024))
    N = 40
    noeos = lambda s_, l: l.index_fill(2, torch.tensor([1024]), -float("inf"))
    refs, traces = [], []
    for i in range(B):
        tr = zo.GenTrace()
        refs.append(zo.generate(w, cfg, utts[i], audio_prefix_codes=pre[i:i + 1], max_new_tokens=N, batch_size=1, sampling_params=GREEDY, trace=tr,
                                logits_hook=noeos))
        traces.append(tr)
    calls = len(traces[0].tokens)
    assert all(len(t.tokens) == calls for t in traces)
    toks = torch.stack([torch.cat([t.tokens[k] for t in traces], 0) for k in range(calls)]).numpy()          # [calls, B, 9]
    cond, lens = pad_conditionings(utts, 2.0)
    eng = model.engine(B)
    eng.call("zn_debug_eos_bias", float("-inf"))
    tk = torch.from_numpy(toks.astype(np.int32)).to(DEV).contiguous()
    eng.call("zn_debug_token_override", tk.data_ptr(), tk.shape[0])
    try:
        tr = {"logits": []}
        out = model.generate(cond.to(DEV), audio_prefix_codes=pre.to(DEV), max_new_tokens=N, batch_size=B, sampling_params=GREEDY, _trace=tr,
                             conditioning_lengths=lens).cpu()
    finally:
        eng.call("zn_debug_token_override", None, 0)
        eng.call("zn_debug_eos_bias", 0.0)
    assert eng.counters()["handoff_timeouts"] == 0
    logits = [l.cpu().numpy() for l in tr["logits"]]
    worst = 0.0
    for i in range(B):
        assert out[i:i + 1].shape == refs[i].shape and torch.equal(out[i:i + 1], refs[i]), i
        for k in range(len(traces[i].logits)):
            a, b = logits[k][i], traces[i].logits[k].numpy()[0]
            fin = np.isfinite(b)
            worst = max(worst, float(np.abs(np.where(fin, a, 0.0) - np.where(fin, b, 0.0)).max()))
            t2 = np.sort(np.where(fin, b, -1e30), -1)[..., -2:]
            dec = (t2[..., 1] - t2[..., 0]) > 0.15
            assert (np.where(fin, a, -1e30).argmax(-1) == np.where(fin, b, -1e30).argmax(-1))[dec].all(), (i, k)
    print(f"\n[ragged B={B} vs solo oracle runs] {calls} calls, worst |dlogit| {worst:.4g}")
    assert worst <= 0.06


# ------------------------------------------------------------------------------------------------ 5. two unguided rows of unequal length
@pytest.mark.parametrize("which", ["chain", "full"])
def test_two_unguided_rows_of_unequal_length(full, which):
    """cfg_scale=1, B = 2 on models the two-row persistent kernels serve (d_model 512: the per-block chain; Zonos-v0.1 dimensions: the
    whole-step kernel).  Equal lengths keep them; unequal lengths run the launches path (zn_decode_path_detail == 0, include/zonos_hip.h)
    and give each utterance the bits of the uniform batches, which ran the persistent kernels."""
    if which == "chain":
        cfg = synth.CHAIN_CFG
        model, _ = build_model(cfg, 91, DEV)
    else:
        cfg, model = synth.FULL_CFG, full[0]
    d, lengths = cfg["d_model"], [9, 15]
    eng = model.engine(2)
    utts = _utterances(lengths, d, 700, halves=1)
    _run(model, _rows(_utterances([9, 9], d, 710, halves=1)), 2, 10, cfg_scale=1.0)
    persistent = eng.lib.zn_decode_path_detail(eng.h)
    assert persistent == (1 if which == "chain" else 2), persistent
    cond, lens = pad_conditionings(utts, 1.0)
    codes, logits = _run(model, cond, 2, 10, lengths=lens, cfg_scale=1.0)
    assert eng.lib.zn_decode_path_detail(eng.h) == 0 and eng.lib.zn_decode_path(eng.h) == 0
    for i, L in enumerate(lengths):
        mates = _utterances([L, L], d, 720 + 10 * i, halves=1)
        mates[i] = utts[i]
        ucodes, ulogits = _run(model, _rows(mates), 2, 10, cfg_scale=1.0)
        assert eng.lib.zn_decode_path_detail(eng.h) == persistent
        assert _same_bits(logits[:, i], ulogits[:, i]) and torch.equal(codes[i], ucodes[i]), i
    c = eng.counters()
    assert c["handoff_timeouts"] == 0 and c["demoted"] == 0, c


# ------------------------------------------------------------------------------------------------ 6. errors
def _raw_prefill_rows(model, B, rows, S, row_len, cfg_scale):
    """zn_gen_begin + zn_prefill_rows on a random right-padded input; returns (status, message)."""
    eng = model.engine(max(B, (rows + 1) // 2))
    nq, d = model.config.codebook_dimension, model.config.backbone.d_model
    ip = model.setup_cache(batch_size=rows, max_seqlen=S + 16)
    delayed = torch.full((B, nq, 12), model.masked_token_id, dtype=torch.int32, device=DEV)
    sp = _sampling_struct(GREEDY, 0)
    n_layer = model.config.backbone.n_layer
    kv = (C.c_void_p * n_layer)(*[ip.key_value_memory_dict[i][0].data_ptr() for i in range(n_layer)])
    st = eng.stream()
    eng.call("zn_gen_begin", B, kv, ip.max_seqlen, ip.lengths_per_sample.data_ptr(), delayed.data_ptr(), 12, 1, 4, float(cfg_scale), C.byref(sp), st)
    hidden = synth.conditioning(5, "ragged.err", rows, S, d).to(DEV)
    try:
        rc = eng.lib.zn_prefill_rows(eng.h, hidden.data_ptr(), S, (C.c_int32 * rows)(*row_len), st)
        msg = eng.lib.zn_last_error(eng.h).decode()
    finally:
        torch.cuda.synchronize()
        eng.call("zn_gen_end")
    return rc, msg


@pytest.mark.parametrize("arch", ["transformer", "hybrid"])
def test_errors_are_statuses_and_leave_the_handle_usable(models, arch):
    model, _ = models(arch)
    d = CFGS[arch]["d_model"]
    good = _run(model, _rows(_utterances([6, 6], d, 800)), 2, 6)
    rc, msg = _raw_prefill_rows(model, 2, 4, 9, [9, 5, 9, 6], 2.0)                # utterance 1: 5 conditional, 6 unconditional positions
    assert rc == -1 and "utterance 1" in msg and "lockstep" in msg, (rc, msg)
    for bad in ([9, 0, 9, 0], [9, 10, 9, 10], [8, 5, 8, 5]):                       # out of range; beyond S; no row of S positions
        rc, msg = _raw_prefill_rows(model, 2, 4, 9, bad, 2.0)
        assert rc == -1 and "zn_prefill_rows" in msg, (bad, rc, msg)
    eng = model.engine(2)
    eng.call("zn_debug_prefill_mode", 0)
    try:
        rc, msg = _raw_prefill_rows(model, 2, 4, 9, [9, 5, 9, 5], 2.0)
        assert rc == -4 and "position by position" in msg, (rc, msg)
        cond, lens = pad_conditionings(_utterances([6, 3], d, 810), 2.0)
        with pytest.raises(_lib.ZonosHipError, match=r"status -4"):
            model.generate(cond.to(DEV), max_new_tokens=4, batch_size=2, sampling_params=GREEDY, conditioning_lengths=lens)
        rc, _ = _raw_prefill_rows(model, 2, 4, 9, [9, 9, 9, 9], 2.0)              # equal lengths are zn_prefill: served position by position too
        assert rc == 0
    finally:
        eng.call("zn_debug_prefill_mode", 1)
    again = _run(model, _rows(_utterances([6, 6], d, 800)), 2, 6)
    assert torch.equal(good[0], again[0]) and _same_bits(good[1], again[1])
    cond, lens = pad_conditionings(_utterances([6, 3], d, 810), 2.0)
    out, _ = _run(model, cond, 2, 6, lengths=lens)
    assert out.shape[0] == 2
