"""Per-utterance sampling parameters, seed, cfg_scale and length in one batch (Zonos.generate_batch, zn_gen_set_rows, zn_op_sample_rows;
DESIGN.md 4.1c).  Everything is asserted bit for bit, on seeded synthetic weights: a request gets what it would get from a call that
gives its settings to the whole batch, its random stream is that of a one-utterance call with its seed, and it is cut where its own
loop would have ended."""
import ctypes as C

import pytest
import torch

from zonos_amd import _lib, synth
from zonos_amd.codebook_pattern import apply_delay_pattern, revert_delay_pattern
from zonos_amd.conditioning import pad_conditionings
from zonos_amd.model import GenRequest, _sampling_struct, finalise_codes, row_end_offset, stop_check_at
from zonos_amd.testing import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NQ, V, EOS, MASK = 9, 1025, 1024, 1025
CFGS = {"transformer": synth.TINY_CFG, "hybrid": synth.HYBRID_TINY_CFG}


@pytest.fixture(scope="module")
def models():
    built = {}

    def get(name):
        if name not in built:
            built[name] = build_model(CFGS[name], 77 if name == "transformer" else 23, DEV, peaky=True)[0]
        return built[name]
    return get


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _utt(seed, L, d, halves=2):
    return synth.conditioning(seed, "requests.cond", halves, L, d)


def _table(rows):
    """zn_row_params array [(sampling dict, seed, cfg_scale, max_new_tokens)] and its copy on the device."""
    t = (_lib.zn_row_params * len(rows))()
    for i, (sp, seed, cfg_scale, max_new) in enumerate(rows):
        t[i].sp, t[i].cfg_scale, t[i].max_new_tokens = _sampling_struct(sp, seed), cfg_scale, max_new
    return t, torch.frombuffer(bytearray(bytes(t)), dtype=torch.uint8).to(DEV)


class _hooks:
    """EOS suppressed (and, optionally, forced at one loop step, which overrides the suppression) on the engine that serves B utterances."""
    def __init__(self, model, B, force=-1):
        self.eng, self.force = model.engine(B), force

    def __enter__(self):
        self.eng.call("zn_debug_eos_bias", float("-inf"))
        self.eng.call("zn_debug_force_eos", self.force)
        return self.eng

    def __exit__(self, *exc):
        self.eng.call("zn_debug_eos_bias", 0.0)
        self.eng.call("zn_debug_force_eos", -1)
        if exc[0] is None:
            assert self.eng.counters()["handoff_timeouts"] == 0


def _batch(model, reqs, trace=True, keep_delayed=False):
    """generate_batch -> (results on the host, per-call logits [calls, B, 9, 1025] or None, the call's delayed codes or None)."""
    tr, kept = ({"logits": []} if trace else None), []
    if keep_delayed:
        tr["after_step"] = lambda i, delayed, offset: kept.append(delayed)
    outs = [o.cpu() for o in model.generate_batch(reqs, _trace=tr)]
    return outs, (torch.stack([l.cpu() for l in tr["logits"]]) if trace else None), (kept[-1].cpu() if kept else None)


# ------------------------------------------------------------------------------------------------ 1. the kernel, row by row
SETS = [dict(temperature=0.0, repetition_penalty=3.0, repetition_penalty_window=2),
        dict(temperature=0.9, top_k=40, top_p=0.8),
        dict(temperature=1.2, min_p=0.1, linear=0.7, conf=0.3, quad=0.1)]


def test_sample_rows_is_sample_per_row_in_any_slot(models):
    """zn_op_sample_rows on three rows with three parameter sets and seeds: tokens and filtered probabilities of row b are those of
    zn_op_sample(batch = 1) on row b alone with row b's parameters, and follow the row when the rows are permuted."""
    eng = models("transformer").engine(2)
    st = eng.stream()
    B, W, draw = 3, 7, 5
    logits = torch.from_numpy(synth.normal(11, "requests.logits", (B, NQ, V))).float().mul(3.0).to(DEV).contiguous()
    recent = torch.from_numpy(synth.randint(11, "requests.recent", (B, NQ, W), V)).to(torch.int32).to(DEV)
    for b in range(B):                                    # the window's last two tokens rank high: the penalty decides the greedy row
        top = logits[b].topk(2, dim=-1).indices
        recent[b, :, W - 2:] = top.to(torch.int32)
    recent = recent.contiguous()
    rows = [(SETS[b], 1000 + 17 * b, 2.0, 10) for b in range(B)]

    def solo(b):
        sp = _sampling_struct(rows[b][0], rows[b][1])
        tok = torch.full((1, NQ), -7, dtype=torch.int32, device=DEV)
        pr = torch.full((1, NQ, V), -1.0, dtype=torch.float32, device=DEV)
        eng.call("zn_op_sample", logits[b:b + 1].contiguous().data_ptr(), recent[b:b + 1].contiguous().data_ptr(), W, C.byref(sp), draw,
                 tok.data_ptr(), pr.data_ptr(), 1, st)
        torch.cuda.synchronize()
        return tok.cpu()[0], pr.cpu()[0]

    def batched(order):
        _, tab = _table([rows[i] for i in order])
        lg, rc = logits[order].contiguous(), recent[order].contiguous()
        tok = torch.full((B, NQ), -7, dtype=torch.int32, device=DEV)
        pr = torch.full((B, NQ, V), -1.0, dtype=torch.float32, device=DEV)
        eng.call("zn_op_sample_rows", lg.data_ptr(), rc.data_ptr(), W, tab.data_ptr(), draw, tok.data_ptr(), pr.data_ptr(), B, st)
        torch.cuda.synchronize()
        return tok.cpu(), pr.cpu()

    alone = [solo(b) for b in range(B)]
    assert not torch.equal(alone[0][0], logits[0].argmax(-1).cpu().to(torch.int32)), "the penalty must move the greedy row's choice"
    assert bool((alone[0][1] == -1.0).all()) and bool((alone[1][1] >= 0).all())        # greedy writes no probabilities; sampling rows do
    assert 1 <= int((alone[1][1][0] > 0).sum()) <= 40                                    # top_k
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        tok, pr = batched(order)
        for slot, b in enumerate(order):
            assert torch.equal(tok[slot], alone[b][0]), (order, slot)
            assert _same_bits(pr[slot], alone[b][1]), (order, slot)
    # the same seed in every row: rows with equal logits and parameters draw equal tokens in every slot
    same = [(SETS[2], 5, 2.0, 10)] * B
    _, tab = _table(same)
    lg = logits[:1].repeat(B, 1, 1).contiguous()
    tok = torch.empty(B, NQ, dtype=torch.int32, device=DEV)
    eng.call("zn_op_sample_rows", lg.data_ptr(), None, 0, tab.data_ptr(), 3, tok.data_ptr(), None, B, st)
    torch.cuda.synchronize()
    assert torch.equal(tok[0], tok[1]) and torch.equal(tok[0], tok[2])
    assert eng.counters()["handoff_timeouts"] == 0


# ------------------------------------------------------------------------------------------------ 2. one request is the old call
@pytest.mark.parametrize("arch", ["transformer", "hybrid"])
@pytest.mark.parametrize("cfg_scale", [2.0, 1.0], ids=["guided", "cfg1"])
def test_one_request_is_generate(models, arch, cfg_scale):
    model = models(arch)
    cond = _utt(300, 7, CFGS[arch]["d_model"], 1 if cfg_scale == 1 else 2).to(DEV)
    with _hooks(model, 1):
        for sp, seed in ((dict(temperature=0.0), None), (dict(temperature=1.0), 9)):
            want = model.generate(cond, max_new_tokens=10, cfg_scale=cfg_scale, sampling_params=sp, seed=seed)
            got = model.generate_batch([GenRequest(cond, sampling_params=sp, seed=seed, cfg_scale=cfg_scale, max_new_tokens=10)])
            assert len(got) == 1 and got[0].dtype == torch.int64 and torch.equal(got[0], want), (sp, seed)


# ------------------------------------------------------------------------------------------------ 3. deterministic settings per row
PENALTY = [1.0, 3.0, 5.0, 2.0, 1.5, 4.0, 1.0, 2.5]
SCALE = [1.5, 2.0, 3.0, 2.5, 1.25, 4.0, 1.75, 2.25]
LENGTH = [5, 11, 8, 6, 10, 7, 9, 8]
BUDGET = [6, 14, 9, 11, 7, 13, 8, 10]


@pytest.mark.parametrize("arch", ["transformer", "hybrid"])
@pytest.mark.parametrize("B", [3, 8])
def test_greedy_rows_with_their_own_penalty_scale_and_length(models, arch, B):
    """Request b == row b of generate(batch_size=B) on the same padded conditionings with request b's penalty, cfg_scale and
    max_new_tokens given to the whole batch: codes, and the logits of every call of row b's generation, bit for bit.  The same
    requests without a trace (deferred stop checks, steps replayed as captured graphs) give the same codes."""
    model = models(arch)
    d = CFGS[arch]["d_model"]
    utts = [_utt(310 + b, LENGTH[b], d).to(DEV) for b in range(B)]
    sps = [dict(temperature=0.0, repetition_penalty=PENALTY[b]) for b in range(B)]
    reqs = [GenRequest(utts[b], sampling_params=sps[b], cfg_scale=SCALE[b], max_new_tokens=BUDGET[b]) for b in range(B)]
    cond, lens = pad_conditionings(utts, 2.0)
    with _hooks(model, B):
        outs, logits, _ = _batch(model, reqs)
        assert len(outs) == B and logits.shape[0] == max(BUDGET[:B]) + NQ - 1           # first frame + max_new + 9 - 2 loop steps
        again, _, _ = _batch(model, reqs, trace=False)
        for b in range(B):
            tr = {"logits": []}
            ref = model.generate(cond, max_new_tokens=BUDGET[b], cfg_scale=SCALE[b], batch_size=B, sampling_params=sps[b], _trace=tr,
                                 conditioning_lengths=lens).cpu()
            rl = torch.stack([l.cpu() for l in tr["logits"]])
            assert tuple(outs[b].shape) == (1, NQ, BUDGET[b]) and torch.equal(outs[b], ref[b:b + 1]), b
            assert rl.shape[0] == BUDGET[b] + NQ - 1 and _same_bits(logits[:rl.shape[0], b], rl[:, b]), b
            assert torch.equal(again[b], outs[b]), b
    distinct = {tuple(o[0, :, :6].flatten().tolist()) for o in outs}
    assert len(distinct) == B


# ------------------------------------------------------------------------------------------------ 4. stochastic rows, replayed
@pytest.mark.parametrize("arch", ["transformer", "hybrid"])
def test_stochastic_rows_replay_as_one_utterance_calls(models, arch):
    """Three temperatures and seeds in one call.  Every token the generation wrote is the token zn_op_sample(batch = 1) draws from that
    call's traced logits of the row with the row's parameters and seed, draw index 1 + step and the penalty window of the row's own
    codes (the first frame: draw 0, no penalty) - the stream of a one-utterance generation, whatever the slot."""
    model = models(arch)
    d = CFGS[arch]["d_model"]
    B, temps, seeds, budgets = 3, [0.8, 1.0, 1.3], [41, 42, 43], [10, 7, 12]
    utts = [_utt(330 + b, [6, 9, 5][b], d).to(DEV) for b in range(B)]
    sps = [dict(temperature=temps[b], min_p=0.05) for b in range(B)]                    # repetition penalty 3.0 over 2 tokens (the defaults)
    reqs = [GenRequest(utts[b], sampling_params=sps[b], seed=seeds[b], cfg_scale=2.0, max_new_tokens=budgets[b]) for b in range(B)]
    with _hooks(model, B) as eng:
        outs, logits, _ = _batch(model, reqs)
        st = eng.stream()
        tok = torch.empty(1, NQ, dtype=torch.int32, device=DEV)
        checked = 0
        for b in range(B):
            assert tuple(outs[b].shape) == (1, NQ, budgets[b])
            delayed = apply_delay_pattern(outs[b], MASK)[0]                             # EOS is suppressed: the codes are the raw tokens
            sp = _sampling_struct(sps[b], seeds[b])
            for call in range(budgets[b] + NQ - 1):                                     # call 0 = the first frame, call k = loop step k - 1
                lg = logits[call, b:b + 1].to(DEV).contiguous()
                col = call + 1                                                          # the column the call writes (no audio prefix)
                if call == 0:
                    eng.call("zn_op_sample", lg.data_ptr(), None, 0, C.byref(sp), 0, tok.data_ptr(), None, 1, st)
                else:
                    recent = delayed[:, col - 2:col].to(torch.int32).unsqueeze(0).contiguous().to(DEV)
                    eng.call("zn_op_sample", lg.data_ptr(), recent.data_ptr(), 2, C.byref(sp), call, tok.data_ptr(), None, 1, st)
                torch.cuda.synchronize()
                got = tok.cpu()[0]
                for k in range(NQ):
                    if k + 1 <= col < k + 1 + budgets[b]:                               # the cells of the delay pattern that hold codes
                        assert int(got[k]) == int(delayed[k, col]), (b, call, k)
                        checked += 1
        assert checked == NQ * sum(budgets)
        # identical requests in different slots, with a different one between them
        twin = GenRequest(utts[0], sampling_params=dict(temperature=1.0), seed=77, cfg_scale=2.5, max_new_tokens=9)
        other = GenRequest(utts[1], sampling_params=dict(temperature=1.1), seed=78, cfg_scale=2.0, max_new_tokens=12)
        o3, _, _ = _batch(model, [twin, other, twin], trace=False)
        assert torch.equal(o3[0], o3[2]) and not torch.equal(o3[0][..., :7], o3[1][..., :7])
        o3b, _, _ = _batch(model, [other, twin, twin], trace=False)
        assert torch.equal(o3b[1], o3[0]) and torch.equal(o3b[2], o3[0]) and torch.equal(o3b[0], o3[1])


# ------------------------------------------------------------------------------------------------ 5. per-row length and stop
@pytest.mark.parametrize("arch", ["transformer", "hybrid"])
def test_rows_end_on_their_own_budget_or_stop(models, arch):
    """Codebook-0 EOS forced at loop step 7 in a call with budgets 6, 20 and 40: row 0's budget has ended by then (8 of its 14 remaining
    steps are left, fewer than the 9 an EOS asks for) and it returns its 6 frames; the others are finalised at row_end_offset.  All rows
    are done after step 15 (7 + 9 - 1), which is a stop check of a three-utterance call: 16 loop steps run."""
    model = models(arch)
    d = CFGS[arch]["d_model"]
    budgets, force = [6, 20, 40], 7
    reqs = [GenRequest(_utt(350 + b, 5 + b, d).to(DEV), sampling_params=dict(temperature=0.0), cfg_scale=2.0, max_new_tokens=budgets[b])
            for b in range(3)]
    with _hooks(model, 3, force=force):
        outs, logits, delayed = _batch(model, reqs, keep_delayed=True)
        fast, _, _ = _batch(model, reqs, trace=False)
    done_after = max(min(force + NQ - 1, b + NQ - 2) for b in budgets)
    last = next(s for s in range(done_after, 200) if stop_check_at(s, 3))
    assert (done_after, last) == (15, 15) and logits.shape[0] == 1 + last + 1
    assert tuple(outs[0].shape) == (1, NQ, budgets[0])
    for b in range(3):
        t_b = budgets[b] + NQ
        row = delayed[b:b + 1, :, :t_b].to(torch.int64)
        assert int(row[0, 0, force + 2]) == (EOS if b else MASK)                        # the EOS column: beyond row 0's own cells
        hit = (row[0, 0, 2:] == EOS).nonzero()
        end = row_end_offset(1, t_b, 3, NQ, 2 + int(hit[0, 0]) if len(hit) else None)
        assert end == (t_b if b == 0 else last + 2)
        want = finalise_codes(revert_delay_pattern(row), end, NQ, EOS)
        assert torch.equal(outs[b], want), b
        assert torch.equal(fast[b], outs[b]), b                                         # deferred stop checks, captured graphs
    assert outs[1].shape[2] == outs[2].shape[2] == force + 1                            # frames 0 .. 7: the EOS frame (8) is where they stop


# ------------------------------------------------------------------------------------------------ 6. state errors
@pytest.mark.parametrize("arch", ["transformer", "hybrid"])
def test_set_rows_errors_are_statuses_and_leave_the_generation_usable(models, arch):
    model = models(arch)
    d = CFGS[arch]["d_model"]
    reqs = [GenRequest(_utt(370 + b, 6, d).to(DEV), sampling_params=dict(temperature=0.0, repetition_penalty=2.0 + b), cfg_scale=2.0 + b,
                       max_new_tokens=6 + b) for b in range(2)]
    with _hooks(model, 2) as eng:
        good, _, _ = _batch(model, reqs)
        n_layer, B, S, max_new = model.config.backbone.n_layer, 2, 7, 8
        ip = model.setup_cache(batch_size=2 * B, max_seqlen=S + max_new + NQ)
        delayed = apply_delay_pattern(torch.full((B, NQ, max_new), -1, dtype=torch.int32, device=DEV), MASK).contiguous()
        kv = (C.c_void_p * n_layer)(*[ip.key_value_memory_dict[i][0].data_ptr() for i in range(n_layer)])
        st = eng.stream()
        sp = _sampling_struct(dict(temperature=0.0), 0)
        row = lambda cfg_scale=2.0, max_new_tokens=5, window=2: (dict(temperature=0.0, repetition_penalty_window=window), 1, cfg_scale, max_new_tokens)

        def set_rows(rows):
            t, _ = _table(rows)
            rc = eng.lib.zn_gen_set_rows(eng.h, t, len(rows))
            return rc, eng.lib.zn_last_error(eng.h).decode()
        eng.call("zn_gen_end")
        assert set_rows([row(), row()])[0] == -3                                        # no generation begun
        eng.call("zn_gen_begin", B, kv, ip.max_seqlen, ip.lengths_per_sample.data_ptr(), delayed.data_ptr(), delayed.shape[2], 1, max_new, 2.0,
                 C.byref(sp), st)
        try:
            rc, msg = set_rows([row(), row(), row()])
            assert rc == -1 and "3 entries" in msg, (rc, msg)
            rc, msg = set_rows([row(), row(cfg_scale=1.0)])
            assert rc == -1 and "utterance 1" in msg and "cfg_scale" in msg, (rc, msg)
            assert set_rows([row(cfg_scale=1.0), row(cfg_scale=1.0)])[0] == -1          # the row layout was fixed with guidance
            assert set_rows([row(max_new_tokens=0), row()])[0] == -1 and set_rows([row(), row(max_new_tokens=max_new + 1)])[0] == -1
            assert set_rows([row(window=65), row()])[0] == -1
            assert set_rows([row(max_new_tokens=max_new), row(max_new_tokens=1)])[0] == 0
            hidden = synth.conditioning(5, "requests.err", 2 * B, S, d).to(DEV)
            eng.call("zn_prefill", hidden.data_ptr(), S, st)
            rc, msg = set_rows([row(), row()])
            assert rc == -3 and "after zn_prefill" in msg, (rc, msg)
            eng.call("zn_sample_first", st)                                             # the generation goes on after the refused calls
            eng.call("zn_decode_steps", 3, st)
            done = C.c_int32(-1)
            eng.call("zn_all_stopped", C.byref(done), st)
            assert done.value == 0
            assert bool((delayed[:, 0, 1:5] >= 0).all()) and bool((delayed[:, 0, 1:5] <= EOS).all())    # first frame + three steps were written
        finally:
            torch.cuda.synchronize()
            eng.call("zn_gen_end")
        again, _, _ = _batch(model, reqs)
        assert all(torch.equal(a, g) for a, g in zip(again, good))
