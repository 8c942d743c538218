"""Guided and unguided requests in one generate_batch() call and one serving session (the row pair of zn_row_params).
Everything is asserted bit for bit, codes and per-step logits, on seeded synthetic weights.

The bit contract.  In a mixed call or session of R rows, a guided request's logits and codes are those of its row in a guided
generate_batch(ragged_prefix=True) call of R / 2 requests, an unguided request's those of its row in an unguided call of R requests: both
references run R rows, hence the same kernels.  The reference call holds the request beside mates of its own conditioning length, budget
and prefix length, as tests/test_gpu_serve.py builds it.  Codes are compared where `row_end_offset` agrees for the two batch sizes, which
every case asserts on the CPU (EOS is suppressed, or forced at a step at which both cadences check at loop step 15).

Comparability.  The transformer's prefill projections pick their kernel by M = rows x positions; every prefill here - the mixed call's, an
admission's, a reference call's - keeps M <= 64 and the cases assert it.  At R = 16 that leaves 3 conditioning positions and no prefix; at
R = 18 it leaves 2 conditioning positions (one fewer than everywhere else: 18 x 4 = 72 would leave the class)."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest
import torch

from zonos_amd import _lib, synth
from zonos_amd.autoencoder import DACAutoencoder
from zonos_amd.codebook_pattern import apply_delay_pattern
from zonos_amd.model import GenRequest, ServeResult, _drain, _sampling_struct
from zonos_amd.rows import GenCall, Hooks
from zonos_amd.serving import ServeChunk, row_end_offset
from zonos_amd.testing import build_model

from test_gpu_serve import CFGS, EOS, MASK, NQ, SEEDS, V, _gemm_class, _hooks, _plen, _prefix, _row_len, _same_bits, _Session, _utt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mixed_defaults.npz")
PENALTY, SCALE = [1.0, 3.0, 5.0, 2.0, 1.5], [1.5, 2.0, 3.0, 2.5, 1.25]


@pytest.fixture(scope="module")
def dac():
    return DACAutoencoder(synth.dac_state_dict(4321, encoder=False), device=DEV)


@pytest.fixture(scope="module")
def models(dac):
    built = {}

    def get(name):
        if name not in built:
            built[name] = build_model(CFGS[name], SEEDS[name], DEV, dac=dac, peaky=True)[0]
        return built[name]
    return get


def _mk(arch, kind, tag, L, n, P=0, sp=None, seed=None):
    """One request: kind "G" (guided, [2, L, d]) or "U" (cfg_scale == 1, [1, L, d]); `tag` names it (its conditioning, its reference)."""
    d, halves = CFGS[arch]["d_model"], 2 if kind == "G" else 1
    sp = dict(temperature=0.0, repetition_penalty=PENALTY[tag % 5]) if sp is None else sp
    r = GenRequest(_utt(2000 + tag, L, d, halves).to(DEV), sampling_params=sp, seed=seed, cfg_scale=SCALE[tag % 5] if kind == "G" else 1.0,
                   max_new_tokens=n, audio_prefix_codes=_prefix(2400 + tag, P))
    r._tag = tag
    return r


def _mix(arch, kinds, Ls, budgets, prefixes=None, base=0, stochastic=()):
    prefixes = [0] * len(kinds) if prefixes is None else prefixes
    out = []
    for i, (k, L, n, P) in enumerate(zip(kinds, Ls, budgets, prefixes)):
        sp, seed = (dict(temperature=1.0, top_k=40), 4242 + i) if i in stochastic else (None, None)
        out.append(_mk(arch, k, base + i, L, n, P, sp, seed))
    return out


def _guided(r):
    return float(r.cfg_scale) != 1.0


def _rows(reqs):
    return sum(2 if _guided(r) else 1 for r in reqs)


def _first_rows(reqs):
    first, u = [], 0
    for r in reqs:
        first.append(u)
        u += 2 if _guided(r) else 1
    return first


_REFS = {}


def _reference(model, arch, r, rows, force=-1):
    """The request's row in a call of its own kind that runs `rows` rows (guided: rows / 2 requests) -> (codes, logits [calls, 9, 1025]).
    Computed once per (request, rows, hook) and shared by the tests."""
    key = (arch, rows, force, r._tag)
    if key not in _REFS:
        d, halves = CFGS[arch]["d_model"], 2 if _guided(r) else 1
        assert rows % halves == 0
        B = rows // halves
        if arch == "transformer":
            assert _gemm_class(rows * _row_len(r)) == 0
        pos = r._tag % B
        mates = [GenRequest(_utt(7000 + 10 * r._tag + k, int(r.conditioning.shape[1]), d, halves).to(DEV), sampling_params=r.sampling_params, seed=r.seed,
                            cfg_scale=r.cfg_scale, max_new_tokens=r.max_new_tokens, audio_prefix_codes=_prefix(7500 + 10 * r._tag + k, _plen(r))) for k in range(B - 1)]
        tr = {"logits": []}
        outs = model.generate_batch(mates[:pos] + [r] + mates[pos:], ragged_prefix=True, _trace=tr)
        _REFS[key] = (outs[pos].cpu(), torch.stack([lg[pos].cpu() for lg in tr["logits"]]))
    return _REFS[key]


def _ends_agree(r, n_requests, rows, force):
    """row_end_offset of the request for the mixed call's cadence and for its reference call's; they must agree for codes to be compared."""
    P, n = _plen(r), int(r.max_new_tokens)
    t_b = P + n + NQ
    eos = P + force + 2 if 0 <= force and force + 1 < n else None                   # loop step `force` writes frame force + 1, if the row still has it
    end = row_end_offset(P + 1, t_b, n_requests, NQ, eos)
    ref_B = rows // 2 if _guided(r) else rows
    assert end == row_end_offset(P + 1, t_b, ref_B, NQ, eos), (r._tag, end, n_requests, ref_B)
    return end


def _run_mixed(model, reqs, ragged):
    kept = []
    tr = {"logits": [], "after_step": lambda i, delayed, offset: kept.append(delayed)}
    outs = model.generate_batch(reqs, ragged_prefix=ragged, mixed_guidance=True, _trace=tr)
    return [o.cpu() for o in outs], torch.stack([lg.cpu() for lg in tr["logits"]]), kept[-1].cpu()


def _check_call(model, arch, reqs, ragged, force=-1):
    """generate_batch(mixed_guidance=True) against every request's reference call; returns the call's results."""
    R, first = _rows(reqs), _first_rows(reqs)
    if arch == "transformer":
        assert _gemm_class(R * max(_row_len(r) for r in reqs)) == 0
    with _hooks(model, (R + 1) // 2, arch, force=force):
        outs, logits, delayed = _run_mixed(model, reqs, ragged)
        assert logits.shape[1:] == (R, NQ, V) and delayed.shape[0] == R
        fast = [o.cpu() for o in model.generate_batch(reqs, ragged_prefix=ragged, mixed_guidance=True)]     # deferred stop checks, captured graphs
        for i, r in enumerate(reqs):
            end = _ends_agree(r, len(reqs), R, force)
            ref, rl = _reference(model, arch, r, R, force)
            assert torch.equal(outs[i], ref), f"request {i}: codes differ from its reference call's"
            assert torch.equal(fast[i], outs[i]), f"request {i}: the call without a trace differs"
            u, k = first[i], min(logits.shape[0], rl.shape[0])
            assert k >= end - _plen(r) - 1, (i, k, end)
            assert _same_bits(logits[:k, u], rl[:k]), f"request {i}: logits differ from its reference call's"
            if _guided(r):
                t_b = _plen(r) + int(r.max_new_tokens) + NQ
                assert _same_bits(logits[:, u + 1], logits[:, u]), f"request {i}: its two rows saw different logits"
                assert torch.equal(delayed[u, :, :t_b], delayed[u + 1, :, :t_b]), f"request {i}: its two rows hold different cells"
    return outs, logits


# ------------------------------------------------------------------------------------------------ 1. R = 4: the GEMV kernels; 7. sampling
def test_four_rows_guided_beside_unguided(models):
    """[G, U, U] in one call of four rows, the guided request and one unguided request sampling (temperature 1, top_k 40, their own
    seeds).  Besides the references: every token of the two sampling requests is the token zn_op_sample(batch = 1) draws from the call's
    traced logits of the request's row with the request's parameters and seed - the stream of a one-utterance generate(seed=s), as
    tests/test_gpu_requests.py replays it."""
    arch = "transformer"
    model = models(arch)
    reqs = _mix(arch, "GUU", [5, 3, 7], [6, 12, 4], base=10, stochastic=(0, 1))
    with pytest.raises(ValueError, match="row layout"):
        model.generate_batch(reqs)
    outs, logits = _check_call(model, arch, reqs, ragged=False)
    assert [tuple(o.shape) for o in outs] == [(1, NQ, 6), (1, NQ, 12), (1, NQ, 4)]
    first = _first_rows(reqs)
    with _hooks(model, 2, arch) as eng:
        st = eng.stream()
        tok = torch.empty(1, NQ, dtype=torch.int32, device=DEV)
        checked = 0
        for i in (0, 1):
            r, n = reqs[i], int(reqs[i].max_new_tokens)
            delayed = apply_delay_pattern(outs[i], MASK)[0]                         # EOS is suppressed: the codes are the raw tokens
            sp = _sampling_struct(r.sampling_params, r.seed)
            for call in range(n + NQ - 1):
                lg, col = logits[call, first[i]:first[i] + 1].to(DEV).contiguous(), call + 1
                if call == 0:
                    eng.call("zn_op_sample", lg.data_ptr(), None, 0, C.byref(sp), 0, tok.data_ptr(), None, 1, st)
                else:
                    recent = delayed[:, col - 2:col].to(torch.int32).unsqueeze(0).contiguous().to(DEV)
                    eng.call("zn_op_sample", lg.data_ptr(), recent.data_ptr(), 2, C.byref(sp), call, tok.data_ptr(), None, 1, st)
                torch.cuda.synchronize()
                got = tok.cpu()[0]
                for k in range(NQ):
                    if k + 1 <= col < k + 1 + n:
                        assert int(got[k]) == int(delayed[k, col]), (i, call, k)
                        checked += 1
        assert checked == NQ * (6 + 12)
    greedy = [GenRequest(r.conditioning, sampling_params=dict(temperature=0.0), cfg_scale=r.cfg_scale, max_new_tokens=r.max_new_tokens) for r in reqs]
    with _hooks(model, 2, arch):
        g = model.generate_batch(greedy, mixed_guidance=True)
    assert not torch.equal(g[0].cpu(), outs[0]) and not torch.equal(g[1].cpu(), outs[1]), "the temperature must decide tokens"


# ------------------------------------------------------------------------------------------------ 2. R = 6 and 16: the small-M tile; 8. hybrid
ORDERS6 = {"interleaved": "UGUG", "grouped": "GGUU"}
ORDERS16 = {"interleaved": "UGUGUGUGUGU", "grouped": "GGGGGUUUUUU"}


def _six(arch):
    # tags follow the kind, so both orders share their requests' references
    g = [_mk(arch, "G", 30, 5, 9, 1), _mk(arch, "G", 31, 7, 14, 0)]
    u = [_mk(arch, "U", 32, 3, 20, 3), _mk(arch, "U", 33, 6, 5, 2)]
    return g, u


@pytest.mark.parametrize("arch", ["transformer", "hybrid"])
@pytest.mark.parametrize("order", sorted(ORDERS6))
def test_six_rows_in_two_orders(models, arch, order):
    g, u = _six(arch)
    gi, ui = iter(g), iter(u)
    reqs = [next(gi) if k == "G" else next(ui) for k in ORDERS6[order]]
    assert _rows(reqs) == 6
    outs, _ = _check_call(models(arch), arch, reqs, ragged=True)
    assert [o.shape[2] for o in outs] == [_plen(r) + int(r.max_new_tokens) for r in reqs]


def test_six_rows_with_a_forced_eos(models):
    """EOS forced in codebook 0 at loop step 3: every row still has frame 4 and stops there.  The rows with more than 8 frames leave at
    the check after loop step 15, which calls of 4, 3 and 6 utterances all make (column P + 17: 8 frames, the EOS frame outside the
    boundary search's window of 2); the row with 5 frames ends on its budget, where the search finds the EOS frame."""
    arch = "transformer"
    g, u = _six(arch)
    reqs = [u[0], g[0], u[1], g[1]]
    outs, _ = _check_call(models(arch), arch, reqs, ragged=True, force=3)
    assert [o.shape[2] - _plen(r) for o, r in zip(outs, reqs)] == [8, 8, 4, 8]


@pytest.mark.parametrize("order", sorted(ORDERS16))
def test_sixteen_rows_in_two_orders(models, order):
    arch = "transformer"
    budgets = [4, 9, 13, 6, 20, 8, 5, 11, 7, 16, 10]
    g = [_mk(arch, "G", 50 + j, 3, budgets[j]) for j in range(5)]
    u = [_mk(arch, "U", 60 + j, 3, budgets[5 + j]) for j in range(6)]
    gi, ui = iter(g), iter(u)
    reqs = [next(gi) if k == "G" else next(ui) for k in ORDERS16[order]]
    assert _rows(reqs) == 16
    _check_call(models(arch), arch, reqs, ragged=False)


# ------------------------------------------------------------------------------------------------ 4. ragged prefixes in a mixed call
def test_ragged_prefixes_in_a_mixed_call(models):
    arch = "transformer"
    reqs = _mix(arch, "GUUG", [4, 7, 5, 3], [7, 10, 4, 12], [3, 0, 1, 0], base=80)
    outs, _ = _check_call(models(arch), arch, reqs, ragged=True)
    assert [tuple(o.shape) for o in outs] == [(1, NQ, 10), (1, NQ, 10), (1, NQ, 5), (1, NQ, 12)]
    with pytest.raises(ValueError, match="different lengths"):
        models(arch).generate_batch(reqs, mixed_guidance=True)


# ------------------------------------------------------------------------------------------------ sessions
def _sizes(source):
    reqs = [r for r in source if isinstance(r, GenRequest)]
    return max(_row_len(r) - 1 for r in reqs), max(int(r.max_new_tokens) for r in reqs)


def _serve(model, source, slots, sched_every, trace=True, guided=None):
    max_prompt, max_new = _sizes(source)
    tr = {} if trace else None
    out, order = {}, []
    for res in model.serve(iter(source), slots=slots, max_prompt=max_prompt, max_new_tokens=max_new, guided=guided, sched_every=sched_every, _trace=tr):
        assert isinstance(res, ServeResult) and res.index not in out and res.error is None, res
        out[res.index] = res
        order.append(res.index)
    return out, tr, order


def _slots_of(tr, index):
    kind, _, held = next(rec for rec in tr["slots"] if rec[0] == "admit" and index in rec[2])
    return [b for b, who in enumerate(held) if who == index]


def _session_logits(tr, index, which=0):
    """The logits of request `index` in its first (or second) slot: its admission's, then those of every step it held the slot."""
    b = _slots_of(tr, index)[which]
    return torch.stack([lg[b].cpu() for lg, (_, _, held) in zip(tr["logits"], tr["slots"]) if held[b] == index])


def _check_served(model, arch, reqs, slots, out, tr, indices=None):
    for i in (range(len(reqs)) if indices is None else indices):
        r = reqs[i]
        _ends_agree(r, slots, slots, -1)
        ref, rl = _reference(model, arch, r, slots)
        assert torch.equal(out[i].codes.cpu(), ref), f"request {i}: codes differ from its reference call's"
        got = _session_logits(tr, i)
        assert got.shape[0] >= rl.shape[0], (i, got.shape, rl.shape)
        assert _same_bits(got[:rl.shape[0]], rl), f"request {i}: logits differ from its reference call's"
        held = _slots_of(tr, i)
        assert len(held) == (2 if _guided(r) else 1)
        if _guided(r):
            assert _same_bits(_session_logits(tr, i, 1), got), f"request {i}: its two rows saw different logits"


def _admissions(tr, reqs):
    """[(session step, [request indices])] and the check that every admission prefilled M = rows x positions in projection class 0."""
    out = []
    for kind, step, held in tr["slots"]:
        if kind == "admit":
            rows = [h for h in held if h is not None]
            assert _gemm_class(len(rows) * max(_row_len(reqs[h]) for h in rows)) == 0
            out.append((step, sorted(set(rows))))
    return out


SESSION_KINDS = "GGUUGUGUUG"
SESSION_L = [5, 7, 3, 6, 4, 7, 3, 5, 6, 4]
SESSION_BUDGET = [9, 14, 20, 4, 12, 6, 17, 5, 10, 8]
SESSION_PREFIX = [1, 0, 3, 2, 0, 1, 3, 0, 2, 1]


def _session_requests(arch):
    return _mix(arch, SESSION_KINDS, SESSION_L, SESSION_BUDGET, SESSION_PREFIX, base=100, stochastic=(1, 5))


# ------------------------------------------------------------------------------------------------ 5. a mixed session of six rows
def test_ten_requests_through_a_six_row_session(models):
    """G G U U fill the six rows; U3 (4 frames) leaves first and its row stays idle while G4, at the head of the queue, waits for a second
    one - nothing behind it overtakes.  Every result is its reference call's; the two rows of a guided request hold the same cells when
    it retires."""
    arch = "transformer"
    model = models(arch)
    reqs = _session_requests(arch)
    with _hooks(model, 3, arch):
        out, tr, order = _serve(model, reqs, 6, 4)
        _check_served(model, arch, reqs, 6, out, tr)
        fast, _, order2 = _serve(model, reqs, 6, 4, trace=False)                   # four steps per enqueue, as captured graphs
    assert sorted(out) == list(range(10)) and order2 == order
    assert all(torch.equal(fast[i].codes, out[i].codes) for i in range(10))
    admits = _admissions(tr, reqs)
    assert admits[0] == (0, [0, 1, 2, 3]) and [i for _, who in admits for i in who] == list(range(10)), "FIFO, nothing overtakes"
    step4 = next(step for step, who in admits if 4 in who)
    waited = [held for kind, step, held in tr["slots"] if kind == "step" and step <= step4 and held.count(None) == 1]
    assert waited and all(held[5] is None for held in waited), "the guided request waited on the single idle row 5"
    assert _slots_of(tr, 4) == [0, 1] and _slots_of(tr, 5) == [5], "the two lowest idle rows; the request behind takes the third"
    pairs = {index: (held, rows) for index, held, rows in tr["retired"]}
    assert sorted(pairs) == list(range(10))
    for i, r in enumerate(reqs):
        held, rows = pairs[i]
        assert held == _slots_of(tr, i)
        if _guided(r):
            assert len(held) == 2 and torch.equal(rows[0], rows[1]), f"request {i}: its two rows differ at retirement"
            assert int((rows[0] == -1).sum()) == 0


# ------------------------------------------------------------------------------------------------ 6. serve_stream(guided=None)
def test_mixed_stream_concatenates_to_serve_and_decode(models):
    arch = "transformer"
    model = models(arch)
    reqs = _session_requests(arch)
    max_prompt, max_new = _sizes(reqs)
    with _hooks(model, 3, arch):
        served, _, _ = _serve(model, reqs, 6, 4, trace=False)
        chunks = {}
        for ch in model.serve_stream(iter(reqs), slots=6, max_prompt=max_prompt, max_new_tokens=max_new, guided=None, sched_every=4, chunk_frames=4):
            assert isinstance(ch, ServeChunk) and ch.error is None
            got = chunks.setdefault(ch.index, [])
            assert not (got and got[-1].done), f"request {ch.index}: a chunk after its done chunk"
            got.append(ch)
    assert sorted(chunks) == list(range(10)) and all(chs[-1].done for chs in chunks.values())
    early = 0
    for i, chs in chunks.items():
        codes = torch.cat([c.codes for c in chs], dim=2)
        assert torch.equal(codes, served[i].codes), f"request {i}: codes differ from serve(guided=None)'s"
        wav = torch.cat([c.wav for c in chs], dim=2)
        ref = model.autoencoder.decode(served[i].codes)
        assert wav.shape == ref.shape and torch.equal(wav, ref), f"request {i}: wav differs from decode() of its codes"
        early += any(c.wav.shape[2] > 0 for c in chs[:-1])
    assert early >= 2, "requests of both kinds must hear audio before they retire"


# ------------------------------------------------------------------------------------------------ 3. R = 18: a pair across the 16-row group
def test_a_pair_straddles_the_sixteen_row_group(models):
    """Eighteen unguided requests fill eighteen rows; those in rows 3 and 17 have 4 frames and leave at session step 12, and the guided
    request behind them takes rows 3 and 17: its conditional row in the first 16-row group of the small-M kernels, its unconditional one
    in the second."""
    arch = "transformer"
    model = models(arch)
    reqs = [_mk(arch, "U", 200 + j, 2, 4 if j in (3, 17) else 20) for j in range(18)] + [_mk(arch, "G", 220, 2, 8)]
    with _hooks(model, 9, arch):
        out, tr, _ = _serve(model, reqs, 18, 4)
        assert _slots_of(tr, 18) == [3, 17]
        assert _admissions(tr, reqs) == [(0, list(range(18))), (12, [18])]
        _check_served(model, arch, reqs, 18, out, tr, indices=(18, 0, 3, 16))
    index, held, rows = next(rec for rec in tr["retired"] if rec[0] == 18)
    assert held == [3, 17] and torch.equal(rows[0], rows[1])


def test_a_pair_with_its_unconditional_row_below(models):
    """Through zn_gen_set_rows with a table of our own: eighteen rows, the guided request's unconditional row is row 3 and its conditional
    row is row 17, both entries naming the pair (17, 3); an unguided request in every other row."""
    arch = "transformer"
    model = models(arch)
    g = _mk(arch, "G", 240, 2, 8)
    u = [_mk(arch, "U", 241 + j, 2, 6 + j % 5) for j in range(16)]
    ui = iter(u)
    layout = [("f", g) if b == 3 else ("o", g) if b == 17 else ("u", next(ui)) for b in range(18)]
    cond = torch.stack([(r.conditioning[1] if role == "f" else r.conditioning[0]) for role, r in layout]).contiguous()
    table = (_lib.zn_row_params * 18)()
    for b, (role, r) in enumerate(layout):
        table[b].sp = _sampling_struct(r.sampling_params, 0)
        table[b].cfg_scale, table[b].max_new_tokens = float(r.cfg_scale), int(r.max_new_tokens)
        if role != "u":
            table[b].reserved[0], table[b].reserved[1] = 17 + 1, 3 + 1
    owners = [17] + [b for b, (role, _) in enumerate(layout) if role == "u"]
    assert _gemm_class(18 * 3) == 0
    with _hooks(model, 9, arch):
        call = GenCall(cond, [2] * 18, [None] * 18, [0] * 18, [int(r.max_new_tokens) for _, r in layout], 10, 1.0, _sampling_struct({}, 0),
                       table=table, request_rows=owners)
        with model._engine_held(9) as eng:
            tr = {"logits": []}
            outs = _drain(model._generation(eng, call, torch.cuda.current_stream(), Hooks(trace=tr)))
            assert eng.lib.zn_decode_path_detail(eng.h) == 0
        logits = torch.stack([lg.cpu() for lg in tr["logits"]])
        assert _same_bits(logits[:, 3], logits[:, 17])
        for out, b, r in [(outs[0], 17, g), (outs[1], 0, u[0]), (outs[16], 16, u[15])]:
            _ends_agree(r, 17, 18, -1)
            ref, rl = _reference(model, arch, r, 18)
            k = min(logits.shape[0], rl.shape[0])
            assert k >= int(r.max_new_tokens) + NQ - 1
            assert torch.equal(out.cpu(), ref) and _same_bits(logits[:k, b], rl[:k]), b


# ------------------------------------------------------------------------------------------------ 10. refusals through the C ABI
def test_pair_refusals_are_statuses_and_leave_the_generation_usable(models):
    arch = "transformer"
    model = models(arch)
    d, n_layer, B, S, max_new = CFGS[arch]["d_model"], model.config.backbone.n_layer, 4, 5, 8
    with _hooks(model, 2, arch) as eng:
        st = eng.stream()
        sp = _sampling_struct(dict(temperature=0.0), 0)

        def begin(cfg_scale):
            rows = B if cfg_scale == 1.0 else 2 * B
            ip = model.setup_cache(batch_size=rows, max_seqlen=S + max_new + NQ)
            delayed = apply_delay_pattern(torch.full((B, NQ, max_new), -1, dtype=torch.int32, device=DEV), MASK).contiguous()
            kv = (C.c_void_p * n_layer)(*[ip.key_value_memory_dict[i][0].data_ptr() for i in range(n_layer)])
            eng.call("zn_gen_begin", B, kv, ip.max_seqlen, ip.lengths_per_sample.data_ptr(), delayed.data_ptr(), delayed.shape[2], 1, max_new, cfg_scale,
                     C.byref(sp), st)
            return ip, delayed

        def set_rows(entries):
            """entries: [(cfg_scale, max_new_tokens, penalty, (word 0, word 1))]"""
            t = (_lib.zn_row_params * len(entries))()
            for i, (cfg_scale, n, penalty, words) in enumerate(entries):
                t[i].sp = _sampling_struct(dict(temperature=0.0, repetition_penalty=penalty), 1)
                t[i].cfg_scale, t[i].max_new_tokens, t[i].reserved[0], t[i].reserved[1] = cfg_scale, n, words[0], words[1]
            rc = eng.lib.zn_gen_set_rows(eng.h, t, len(entries))
            return rc, eng.lib.zn_last_error(eng.h).decode()
        U, pair = (1.0, 5, 2.0, (0, 0)), lambda o, f, n=6, penalty=3.0: (2.0, n, penalty, (o + 1, f + 1))
        keep = begin(2.0)                                                           # a pair in a generation begun with guidance
        try:
            rc, msg = set_rows([pair(0, 1), pair(0, 1), (2.0, 5, 2.0, (0, 0)), (2.0, 5, 2.0, (0, 0))])
            assert rc == -1 and "utterance 0" in msg and "begun with guidance" in msg, (rc, msg)
            assert set_rows([(2.0, 5, 2.0, (0, 0))] * 4)[0] == 0
        finally:
            torch.cuda.synchronize()
            eng.call("zn_gen_end")
        ip, delayed = begin(1.0)
        try:
            rc, msg = set_rows([U, (2.0, 6, 3.0, (0, 0)), U, U])
            assert rc == -1 and "utterance 1" in msg and "cfg_scale" in msg, (rc, msg)                   # guided, and no pair named
            rc, msg = set_rows([U, pair(1, 3), U, U])
            assert rc == -1 and "utterance 1" in msg and "differ" in msg, (rc, msg)                       # the partner's entry is another request's
            rc, msg = set_rows([pair(0, 1), U, U, U])
            assert rc == -1 and "utterance 0" in msg, (rc, msg)                                           # the partner does not name the pair
            rc, msg = set_rows([U, pair(1, 3), U, pair(1, 3, penalty=4.0)])
            assert rc == -1 and "utterance 1" in msg and "differ" in msg, (rc, msg)                       # the partner's parameters differ
            rc, msg = set_rows([U, pair(1, 3), U, pair(1, 3, n=7)])
            assert rc == -1 and "differ" in msg, (rc, msg)
            rc, msg = set_rows([U, pair(1, 4), U, U])
            assert rc == -1 and "utterance 1" in msg and "out of range" in msg, (rc, msg)                 # a row out of range
            rc, msg = set_rows([U, (2.0, 6, 3.0, (2, -1)), U, U])
            assert rc == -1 and "out of range" in msg, (rc, msg)
            rc, msg = set_rows([U, pair(1, 1), U, U])
            assert rc == -1 and "utterance 1" in msg and "same row twice" in msg, (rc, msg)               # the same row twice
            rc, msg = set_rows([U, pair(2, 3), pair(2, 3), pair(2, 3)])
            assert rc == -1 and "utterance 1" in msg and "own row" in msg, (rc, msg)                      # a pair that is not the entry's
            rc, msg = set_rows([(1.0, 5, 2.0, (1, 2)), (1.0, 5, 2.0, (1, 2)), U, U])
            assert rc == -1 and "utterance 0" in msg and "cfg_scale == 1" in msg, (rc, msg)               # a pair on an unguided entry
            assert eng.lib.zn_decode_path_detail(eng.h) == 0
            # the generation goes on after the refused calls: the unconditional row below the conditional one
            assert set_rows([U, pair(3, 1), U, pair(3, 1)])[0] == 0
            hidden = synth.conditioning(5, "mixed.err", B, S, d).to(DEV)
            eng.call("zn_prefill", hidden.data_ptr(), S, st)
            eng.call("zn_sample_first", st)
            eng.call("zn_decode_steps", 3, st)
            done = C.c_int32(-1)
            eng.call("zn_all_stopped", C.byref(done), st)
            assert done.value == 0
            cells = delayed.cpu()
            assert bool((cells[:, 0, 1:5] >= 0).all()) and bool((cells[:, 0, 1:5] <= EOS).all())          # first frame + three steps were written
            assert torch.equal(cells[1], cells[3]) and not torch.equal(cells[0], cells[2])
        finally:
            torch.cuda.synchronize()
            eng.call("zn_gen_end")
        del keep, ip


class _RowSession(_Session):
    """tests/test_gpu_serve.py's session through the C ABI, admitting row by row: items are (slot, request, which half of its conditioning,
    the pair its entry names or None, a change to its row_len)."""
    def admit_rows(self, items):
        n, d = len(items), self.model.config.backbone.d_model
        Ls, Ps = [int(r.conditioning.shape[1]) for _, r, _, _, _ in items], [_plen(r) for _, r, _, _, _ in items]
        S = max(L + P + 1 for L, P in zip(Ls, Ps))
        cond = torch.zeros(self.halves * n, max(Ls), d, dtype=torch.bfloat16, device=DEV)
        codes = torch.full((n, NQ, self.width - NQ), MASK, dtype=torch.int32, device=DEV)
        adm = (_lib.zn_admit * n)()
        for j, (slot, r, half, pair, delta) in enumerate(items):
            for hf in range(self.halves):
                cond[hf * n + j, :Ls[j]] = r.conditioning[half if self.halves == 1 else hf].to(torch.bfloat16)
            if Ps[j]:
                codes[j, :, :Ps[j]] = r.audio_prefix_codes[0].to(device=DEV, dtype=torch.int32)
            codes[j, :, Ps[j]:Ps[j] + int(r.max_new_tokens)] = -1
            adm[j].slot, adm[j].row_len, adm[j].prefix_len = slot, Ls[j] + Ps[j] + 1 + delta, Ps[j]
            adm[j].params.sp = _sampling_struct(r.sampling_params, 0 if r.seed is None else r.seed)
            adm[j].params.cfg_scale, adm[j].params.max_new_tokens = float(r.cfg_scale), int(r.max_new_tokens)
            if pair is not None:
                adm[j].params.reserved[0], adm[j].params.reserved[1] = pair[0] + 1, pair[1] + 1
        rows = apply_delay_pattern(codes, MASK).contiguous()
        for j, (slot, _, _, _, _) in enumerate(items):
            self.delayed[slot].copy_(rows[j])
        meta = torch.tensor([Ls, Ps], dtype=torch.int32).to(DEV)
        hidden = torch.zeros(self.halves * n, S, d, dtype=torch.bfloat16, device=DEV)
        row_len = torch.empty(self.halves * n, dtype=torch.int32, device=DEV)
        self.eng.call("zn_op_assemble_prefill", cond.data_ptr(), cond.shape[1], meta[0].data_ptr(), rows.data_ptr(), self.width, meta[1].data_ptr(), n,
                      self.halves * n, hidden.data_ptr(), S, row_len.data_ptr(), self.st)
        self.keep = [cond, rows, hidden, row_len, meta]
        return self.lib.zn_gen_admit(self.h, adm, n, hidden.data_ptr(), S, self.st)


def test_admission_refuses_a_broken_pair_and_the_session_goes_on(models):
    arch = "transformer"
    model = models(arch)
    g, u = _mk(arch, "G", 260, 5, 6, 1), _mk(arch, "U", 261, 4, 5)
    other = _mk(arch, "G", 262, 5, 6, 1)
    with _hooks(model, 4, arch):
        s = _RowSession(model, 2, True, 48, 42, 8)                                  # a guided session knows no pairs
        try:
            assert s.open() == 0
            rc = s.admit_rows([(0, g, 0, (0, 1), 0), (1, g, 1, (0, 1), 0)])
            assert rc == -1 and "slot 0 names a row pair" in s.err() and "begun with guidance" in s.err(), (rc, s.err())
        finally:
            torch.cuda.synchronize()
            s.eng.call("zn_gen_end")
        s = _RowSession(model, 4, False, 48, 42, 8)
        try:
            assert s.open() == 0
            rc = s.admit_rows([(2, g, 0, None, 0), (0, g, 1, None, 0)])
            assert rc == -1 and "slot 2" in s.err() and "names no row pair" in s.err(), (rc, s.err())
            rc = s.admit_rows([(2, g, 0, (2, 0), 0), (1, u, 0, None, 0)])
            assert rc == -1 and "slot 2" in s.err() and "not part of this call" in s.err(), (rc, s.err())      # the partner is missing
            rc = s.admit_rows([(2, g, 0, (2, 0), 0), (0, other, 1, (2, 0), 0)])
            assert rc == -1 and "slot 2" in s.err() and "differ" in s.err(), (rc, s.err())                     # the partner's entry is another request's
            rc = s.admit_rows([(2, g, 0, (2, 0), 0), (0, g, 1, (2, 0), -1)])
            assert rc == -1 and "slot 2" in s.err() and "row_len" in s.err(), (rc, s.err())
            rc = s.admit_rows([(2, g, 0, (2, 4), 0), (0, g, 1, (2, 4), 0)])
            assert rc == -1 and "out of range" in s.err(), (rc, s.err())
            rc = s.admit_rows([(2, g, 0, (2, 2), 0), (0, g, 1, (2, 2), 0)])
            assert rc == -1 and "same row twice" in s.err(), (rc, s.err())
            rc = s.admit_rows([(2, g, 0, (1, 0), 0), (0, g, 1, (1, 0), 0)])
            assert rc == -1 and "slot 2" in s.err() and "own" in s.err(), (rc, s.err())
            assert s.state()[1] == [-1, -1, -1, -1], "a refused admission leaves every slot idle"
            # the session goes on: the pair (conditional row 2, unconditional row 0) beside an unguided request in row 1
            assert s.admit_rows([(2, g, 0, (2, 0), 0), (0, g, 1, (2, 0), 0), (1, u, 0, None, 0)]) == 0, s.err()
            s.steps(8)
            rem, own = s.state()
            assert own == [8, 8, 8, -1]
            cells = s.delayed.cpu()
            assert torch.equal(cells[0], cells[2]) and not torch.equal(cells[0], cells[1]) and int((cells[0, 0, 2:8] == -1).sum()) == 0
            assert s.retire(0) == 0 and s.retire(2) == 0 and s.retire(1) == 0
        finally:
            torch.cuda.synchronize()
            s.eng.call("zn_gen_end")


# ------------------------------------------------------------------------------------------------ 9. unchanged defaults
def _digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def default_runs(get_model):
    """The calls that must not change: generate_batch() without the keyword and sessions with guided=True / guided=False, on both tiny
    models.  Returns {name: array}: every request's codes, a digest of its per-step logits, and what zn_decode_path_detail reported while
    the call ran.  tests/golden/mixed_defaults.npz holds what the commit before mixed generations returned."""
    out = {}
    for arch in ("transformer", "hybrid"):
        model = get_model(arch)
        for guided in (True, False):
            kinds = "GGG" if guided else "UUU"
            name = f"{arch}.{'guided' if guided else 'cfg1'}"
            reqs = _mix(arch, kinds, [5, 7, 3], [9, 14, 6], [1, 0, 2], base=300 if guided else 310, stochastic=(1,))
            with _hooks(model, 3, arch) as eng:
                detail = []
                tr = {"logits": [], "after_step": lambda i, delayed, offset: detail.append(eng.lib.zn_decode_path_detail(eng.h))}
                outs = model.generate_batch(reqs, ragged_prefix=True, _trace=tr)
                for i, o in enumerate(outs):
                    out[f"{name}.batch.codes.{i}"] = o.cpu().numpy().astype(np.int16)
                out[f"{name}.batch.logits"] = np.array(_digest(torch.stack(tr["logits"])))
                out[f"{name}.batch.detail"] = np.array(sorted(set(detail)), dtype=np.int32)
                fast = model.generate_batch(reqs, ragged_prefix=True)
                out[f"{name}.batch.fast"] = np.array(_digest(torch.cat([o.flatten() for o in fast])))
                four = reqs + [_mk(arch, kinds[0], (300 if guided else 310) + 3, 6, 11, 1)]
                max_prompt, max_new = _sizes(four)
                tr, detail = {}, []
                for res in model.serve(iter(four), slots=2, max_prompt=max_prompt, max_new_tokens=max_new, guided=guided, sched_every=4, _trace=tr):
                    assert res.error is None
                    detail.append(eng.lib.zn_decode_path_detail(eng.h))
                    out[f"{name}.serve.codes.{res.index}"] = res.codes.cpu().numpy().astype(np.int16)
                out[f"{name}.serve.logits"] = np.array(_digest(torch.stack(tr["logits"])))
                out[f"{name}.serve.slots"] = np.array(repr(tr["slots"]))
                out[f"{name}.serve.detail"] = np.array(sorted(set(detail)), dtype=np.int32)
    return out


def test_the_defaults_return_what_they_returned_before(models):
    want = np.load(GOLDEN)
    got = default_runs(models)
    assert sorted(got) == sorted(want.files)
    for name in sorted(got):
        assert got[name].shape == want[name].shape and bool((got[name] == want[name]).all()), name
