"""An audio prefix of its own length per request of one generate_batch() call (`ragged_prefix=True`, zn_gen_set_prefix_rows,
zn_op_assemble_prefill).  Everything is asserted bit for bit, on seeded synthetic weights: request b of a mixed-prefix
call gets the codes and the per-call logits of its row in a default-path generate_batch() call of the same B in which every request
brings a prefix of b's length P_b.

Conditioning lengths.  The transformer's prefill projections pick their kernel by M = rows x positions (tests/test_gpu_ragged.py
`_gemm_class`), and only calls within one class are bit-comparable.  Each case therefore takes conditioning lengths for which the
mixed-prefix call (positions up to max_b (L_b + P_b + 1)) and every shared-prefix call (max_b L_b + P + 1 for P in the case's prefix
lengths) fall in one class, and asserts that.  The hybrid backbone prefills in mode 2 (projections row by row: independent of M)."""
import ctypes as C

import pytest
import torch

from zonos_amd import _lib, synth
from zonos_amd.codebook_pattern import apply_delay_pattern
from zonos_amd.model import GenRequest, _sampling_struct
from zonos_amd.testing import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NQ, V, EOS, MASK = 9, 1025, 1024, 1025
CFGS = {"transformer": synth.TINY_CFG, "hybrid": synth.HYBRID_TINY_CFG, "chain": synth.CHAIN_CFG}
SEEDS = {"transformer": 77, "hybrid": 23, "chain": 91}


@pytest.fixture(scope="module")
def models():
    built = {}

    def get(name):
        if name not in built:
            built[name] = build_model(CFGS[name], SEEDS[name], DEV, peaky=name != "chain")[0]
        return built[name]
    return get


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _utt(seed, L, d, halves=2):
    return synth.conditioning(seed, "prefix_rows.cond", halves, L, d)


def _prefix(seed, P):
    return None if P == 0 else torch.from_numpy(synth.randint(seed, "prefix_rows.prefix", (1, NQ, P), 1024))


def _gemm_class(M):
    return 0 if M <= 64 else 1 if M <= 255 else 2


def _one_class(R, lengths, prefixes):
    Ms = [R * (max(lengths) + P + 1) for P in set(prefixes)] + [R * max(L + P + 1 for L, P in zip(lengths, prefixes))]
    classes = {_gemm_class(M) for M in Ms}
    assert len(classes) == 1, f"the mixed-prefix call and the shared-prefix calls must run one projection kernel class: M = {Ms}"


class _hooks:
    """EOS suppressed (and, optionally, forced at one loop step) on the engine that serves B utterances; the hybrid backbone prefills
    row by row; no hand-off timeout may have been counted at the end."""
    def __init__(self, model, B, arch, force=-1, suppress=True):
        self.eng, self.arch, self.force, self.suppress = model.engine(B), arch, force, suppress

    def __enter__(self):
        self.eng.call("zn_debug_eos_bias", float("-inf") if self.suppress else 0.0)
        self.eng.call("zn_debug_force_eos", self.force)
        if self.arch == "hybrid":
            self.eng.call("zn_debug_prefill_mode", 2)
        return self.eng

    def __exit__(self, *exc):
        self.eng.call("zn_debug_eos_bias", 0.0)
        self.eng.call("zn_debug_force_eos", -1)
        self.eng.call("zn_debug_prefill_mode", 1)
        if exc[0] is None:
            assert self.eng.counters()["handoff_timeouts"] == 0


def _batch(model, reqs, ragged):
    """generate_batch with a trace -> (results on the host, per-call logits [calls, B, 9, 1025])."""
    tr = {"logits": []}
    outs = [o.cpu() for o in (model.generate_batch(reqs, ragged_prefix=True, _trace=tr) if ragged else model.generate_batch(reqs, _trace=tr))]
    return outs, torch.stack([l.cpu() for l in tr["logits"]])


def _with_prefix_length(reqs, b):
    """The default-path call request b is compared with: every request brings a prefix of b's length - b its own, the others arbitrary
    codes of that length."""
    P = 0 if reqs[b].audio_prefix_codes is None else reqs[b].audio_prefix_codes.shape[2]
    return [r if i == b else GenRequest(r.conditioning, sampling_params=r.sampling_params, seed=r.seed, cfg_scale=r.cfg_scale,
                                        max_new_tokens=r.max_new_tokens, audio_prefix_codes=_prefix(900 + 10 * b + i, P)) for i, r in enumerate(reqs)]


def _check_against_shared_prefix_calls(model, reqs, untraced=True):
    """Mixed prefixes == shared prefixes, request by request: codes and the logits of every call, bit for bit; the same requests without
    a trace (deferred stop checks, steps replayed as captured graphs) give the same codes.  Returns the mixed call's results."""
    outs, logits = _batch(model, reqs, ragged=True)
    if untraced:
        again = [o.cpu() for o in model.generate_batch(reqs, ragged_prefix=True)]
    for b in range(len(reqs)):
        ref, rl = _batch(model, _with_prefix_length(reqs, b), ragged=False)
        assert torch.equal(outs[b], ref[b]), f"request {b}: codes differ from the shared-prefix call's"
        assert _same_bits(logits[:, b], rl[:, b]), f"request {b}: logits differ from the shared-prefix call's"
        if untraced:
            assert torch.equal(again[b], outs[b]), b
    return outs


# ------------------------------------------------------------------------------------------------ 1. the assembly kernel
@pytest.mark.parametrize("halves", [2, 1], ids=["R6-guided", "R3-unguided"])
def test_assembled_rows_are_the_concatenation(models, halves):
    """zn_op_assemble_prefill for B = 3 with L_b = 1, 5, 8 of L_c = 8 and P_b = 12, 0, 1: valid positions carry the bits of
    cat(cond_r[:L_b], embed_codes(delayed_b[..., :P_b + 1])), pad positions are zero, row_len[r] = L_b + P_b + 1.  The code buffer holds
    unknown cells (-1), the mask token and an id beyond the table, which the embedding clamps as zn_op_embed does."""
    model = models("transformer")
    eng, d = model.engine(3), CFGS["transformer"]["d_model"]
    B, L_c, Ls, Ps, t_total = 3, 8, [1, 5, 8], [12, 0, 1], 30
    R = halves * B
    cond = synth.conditioning(5, "prefix_rows.assemble", R, L_c, d).to(DEV).contiguous()
    delayed = torch.from_numpy(synth.randint(6, "prefix_rows.codes", (B, NQ, t_total), 1026)).to(torch.int32)
    delayed[0, 3, 2], delayed[1, 0, 0], delayed[2, 8, 1], delayed[0, 1, 12] = -1, MASK, 5000, -1
    delayed = delayed.to(DEV).contiguous()
    S = max(L + P + 1 for L, P in zip(Ls, Ps))
    for S_call in (S, S + 3):                                  # the call's S may exceed the longest row: more padding
        hidden = torch.full((R, S_call, d), float("nan"), dtype=torch.bfloat16, device=DEV)
        row_len = torch.full((R,), -7, dtype=torch.int32, device=DEV)
        meta = torch.tensor([Ls, Ps], dtype=torch.int32).to(DEV)
        eng.call("zn_op_assemble_prefill", cond.data_ptr(), L_c, meta[0].data_ptr(), delayed.data_ptr(), t_total, meta[1].data_ptr(), B, R,
                 hidden.data_ptr(), S_call, row_len.data_ptr(), eng.stream())
        torch.cuda.synchronize()
        assert row_len.cpu().tolist() == [Ls[r % B] + Ps[r % B] + 1 for r in range(R)]
        for r in range(R):
            b = r % B
            emb = model.embed_codes(delayed[b:b + 1, :, :Ps[b] + 1])[0]
            want = torch.cat([cond[r, :Ls[b]], emb])
            n = want.shape[0]
            assert n == Ls[b] + Ps[b] + 1
            assert torch.equal(hidden[r, :n].view(torch.int16), want.view(torch.int16)), (r, S_call)
            assert bool((hidden[r, n:].view(torch.int16) == 0).all()), (r, S_call)


# ------------------------------------------------------------------------------------------------ 2. mixed prefixes equal shared prefixes
PENALTY = [1.0, 3.0, 5.0, 2.0, 1.5, 4.0, 1.0, 2.5]
SCALE = [1.5, 2.0, 3.0, 2.5, 1.25, 4.0, 1.75, 2.25]
BUDGET = [6, 14, 9, 11, 7, 13, 8, 10]
PREFIX = {3: [5, 0, 12], 8: [1, 12, 0, 5, 12, 0, 1, 5]}
# conditioning lengths per (B, guided): see the module docstring
LENGTH = {(3, True): [10, 14, 11], (3, False): [21, 30, 25], (8, True): [9, 16, 12, 7, 15, 10, 13, 8], (8, False): [5, 11, 8, 6, 10, 7, 9, 8]}


def _requests(arch, B, guided):
    d, halves = CFGS[arch]["d_model"], 2 if guided else 1
    reqs = []
    for b in range(B):
        sp = dict(temperature=0.0, repetition_penalty=PENALTY[b])
        seed = None
        if b == 1:                                             # one stochastic row, seeded: its stream must not depend on the prefix layout
            sp, seed = dict(temperature=0.9, min_p=0.05, repetition_penalty=PENALTY[b]), 4242
        reqs.append(GenRequest(_utt(400 + b, LENGTH[(B, guided)][b], d, halves).to(DEV), sampling_params=sp, seed=seed,
                               cfg_scale=SCALE[b] if guided else 1.0, max_new_tokens=BUDGET[b], audio_prefix_codes=_prefix(800 + b, PREFIX[B][b])))
    return reqs


@pytest.mark.parametrize("arch", ["transformer", "hybrid"])
@pytest.mark.parametrize("guided", [True, False], ids=["guided", "cfg1"])
@pytest.mark.parametrize("B", [3, 8])
def test_mixed_prefixes_equal_shared_prefixes(models, arch, guided, B):
    model = models(arch)
    reqs = _requests(arch, B, guided)
    assert {0, 12} <= set(PREFIX[B]) <= {0, 1, 5, 12}
    if arch == "transformer":
        _one_class((2 if guided else 1) * B, LENGTH[(B, guided)], PREFIX[B])
    with _hooks(model, B, arch):
        outs = _check_against_shared_prefix_calls(model, reqs)
        for b in range(B):
            assert tuple(outs[b].shape) == (1, NQ, PREFIX[B][b] + BUDGET[b])
            if PREFIX[B][b]:
                assert torch.equal(outs[b][..., :PREFIX[B][b]], reqs[b].audio_prefix_codes)       # a result begins with its own prefix


@pytest.mark.parametrize("arch", ["transformer", "hybrid"])
@pytest.mark.parametrize("guided", [True, False], ids=["guided", "cfg1"])
def test_mixed_prefixes_equal_shared_prefixes_with_a_forced_eos(models, arch, guided):
    """Codebook-0 EOS forced at loop step 3 in every row (budgets 6, 14, 9): every row stops before its budget, at columns of its own."""
    model = models(arch)
    reqs = _requests(arch, 3, guided)
    with _hooks(model, 3, arch, force=3):
        outs = _check_against_shared_prefix_calls(model, reqs, untraced=False)
    assert all(o.shape[2] - p < n for o, p, n in zip(outs, PREFIX[3], BUDGET))                     # (where exactly: finalise_codes' boundary search)


# ------------------------------------------------------------------------------------------------ 3. the penalty history at the left edge
@pytest.mark.parametrize("arch", ["transformer", "hybrid"])
def test_penalty_history_clamps_at_the_rows_own_first_column(models, arch):
    """Greedy, repetition penalty 3 over a window of 8, P = 0 and 12 in one call of 12 frames each.  During its first steps the short
    row has fewer than 8 columns: its history clamps at its own column 0 (a history taken at the call's column would reach 12 columns
    to the right of it), while the long row's reaches into its prefix from the first step on.  Both rows equal their shared-prefix calls."""
    model = models(arch)
    d, Ls, Ps = CFGS[arch]["d_model"], [16, 18], [0, 12]
    if arch == "transformer":
        _one_class(4, Ls, Ps)
    sp = dict(temperature=0.0, repetition_penalty=3.0, repetition_penalty_window=8)
    reqs = [GenRequest(_utt(430 + b, Ls[b], d).to(DEV), sampling_params=sp, cfg_scale=2.0, max_new_tokens=12, audio_prefix_codes=_prefix(830 + b, Ps[b]))
            for b in range(2)]
    with _hooks(model, 2, arch):
        outs = _check_against_shared_prefix_calls(model, reqs)
        plain = [GenRequest(r.conditioning, sampling_params=dict(temperature=0.0, repetition_penalty=1.0), cfg_scale=2.0, max_new_tokens=12,
                            audio_prefix_codes=r.audio_prefix_codes) for r in reqs]
        free = [o.cpu() for o in model.generate_batch(plain, ragged_prefix=True)]
    assert [tuple(o.shape) for o in outs] == [(1, NQ, 12), (1, NQ, 24)]
    assert not torch.equal(free[0], outs[0]) and not torch.equal(free[1], outs[1]), "the penalty must decide tokens in both rows"


# ------------------------------------------------------------------------------------------------ 4. lockstep lengths, different prefixes
def test_two_unguided_rows_in_lockstep_with_different_prefixes_leave_the_persistent_kernels(models):
    """cfg_scale = 1, (L, P) = (8, 2) and (4, 6) on the model the two-row chain kernel serves: both rows hold 11 positions after the
    prefill and advance in lockstep, which is all the routing used to ask - but their columns differ, and the chain path's fused tail does
    not read the shift.  The call runs the launches path (zn_decode_path_detail == 0) and equals the shared-prefix calls; the same keyword
    with equal prefixes has no shift and keeps the chain kernel."""
    model = models("chain")
    d, eng = CFGS["chain"]["d_model"], model.engine(2)
    mk = lambda b, L, P: GenRequest(_utt(450 + b, L, d, 1).to(DEV), sampling_params=dict(temperature=0.0, repetition_penalty=2.0), cfg_scale=1.0,
                                    max_new_tokens=10, audio_prefix_codes=_prefix(850 + b, P))
    with _hooks(model, 2, "chain"):
        model.generate_batch([mk(0, 8, 2), mk(1, 8, 2)], ragged_prefix=True)
        assert eng.lib.zn_decode_path_detail(eng.h) == 1                                           # every shift 0: nothing changed
        reqs = [mk(0, 8, 2), mk(1, 4, 6)]
        outs, logits = _batch(model, reqs, ragged=True)
        assert eng.lib.zn_decode_path_detail(eng.h) == 0 and eng.lib.zn_decode_path(eng.h) == 0
        fast = [o.cpu() for o in model.generate_batch(reqs, ragged_prefix=True)]
        assert eng.lib.zn_decode_path_detail(eng.h) == 0
        for b in range(2):
            ref, rl = _batch(model, _with_prefix_length(reqs, b), ragged=False)
            assert torch.equal(outs[b], ref[b]) and _same_bits(logits[:, b], rl[:, b]), b
            assert torch.equal(fast[b], outs[b]), b


# ------------------------------------------------------------------------------------------------ 5. budgets and stops per row
@pytest.mark.parametrize("arch", ["transformer", "hybrid"])
def test_rows_with_prefixes_end_on_their_own_budget_or_stop(models, arch):
    """Budgets 3, 9, 20 with prefixes 12, 0, 5 and a codebook-0 EOS forced at loop step 5: row 0's budget is spent before it, rows 1 and 2
    stop at it.  Each T_b is what generate_batch returns for the request in a call of that B with a shared prefix of P_b frames."""
    model = models(arch)
    d, Ls, budgets, Ps = CFGS[arch]["d_model"], [10, 14, 11], [3, 9, 20], [12, 0, 5]
    if arch == "transformer":
        _one_class(6, Ls, Ps)
    reqs = [GenRequest(_utt(470 + b, Ls[b], d).to(DEV), sampling_params=dict(temperature=0.0), cfg_scale=2.0, max_new_tokens=budgets[b],
                       audio_prefix_codes=_prefix(870 + b, Ps[b])) for b in range(3)]
    with _hooks(model, 3, arch, force=5):
        outs = [o.cpu() for o in model.generate_batch(reqs, ragged_prefix=True)]
        for b in range(3):
            ref = model.generate_batch(_with_prefix_length(reqs, b))[b].cpu()
            assert outs[b].shape == ref.shape and torch.equal(outs[b], ref), (b, tuple(outs[b].shape), tuple(ref.shape))
    assert outs[0].shape[2] == 12 + 3 and outs[1].shape[2] < 0 + 9 and outs[2].shape[2] < 5 + 20


# ------------------------------------------------------------------------------------------------ 6. errors are statuses
@pytest.mark.parametrize("arch", ["transformer", "hybrid"])
def test_set_prefix_rows_errors_are_statuses_and_leave_the_generation_usable(models, arch):
    model = models(arch)
    d = CFGS[arch]["d_model"]
    reqs = [GenRequest(_utt(490 + b, 6, d).to(DEV), sampling_params=dict(temperature=0.0, repetition_penalty=2.0 + b), cfg_scale=2.0 + b,
                       max_new_tokens=6 + b, audio_prefix_codes=_prefix(890 + b, (5, 2)[b])) for b in range(2)]
    with _hooks(model, 2, arch) as eng:
        good, _ = _batch(model, reqs, ragged=True)
        n_layer, B, S, max_new, P_call = model.config.backbone.n_layer, 2, 7, 8, 5
        ip = model.setup_cache(batch_size=2 * B, max_seqlen=S + max_new + NQ)
        codes = torch.full((B, NQ, P_call + max_new), -1, dtype=torch.int32, device=DEV)
        codes[0, :, :5], codes[1, :, :2] = 7, 9
        delayed = apply_delay_pattern(codes, MASK).contiguous()
        kv = (C.c_void_p * n_layer)(*[ip.key_value_memory_dict[i][0].data_ptr() for i in range(n_layer)])
        st = eng.stream()
        sp = _sampling_struct(dict(temperature=0.0), 0)

        def set_prefix(lens):
            rc = eng.lib.zn_gen_set_prefix_rows(eng.h, (C.c_int32 * len(lens))(*lens), len(lens))
            return rc, eng.lib.zn_last_error(eng.h).decode()
        eng.call("zn_gen_end")
        assert set_prefix([5, 2])[0] == -3                                              # no generation begun
        eng.call("zn_gen_begin", B, kv, ip.max_seqlen, ip.lengths_per_sample.data_ptr(), delayed.data_ptr(), delayed.shape[2], P_call + 1, max_new, 2.0,
                 C.byref(sp), st)
        try:
            rc, msg = set_prefix([5, 2, 0])
            assert rc == -1 and "3 entries" in msg, (rc, msg)
            rc, msg = set_prefix([5, -1])
            assert rc == -1 and "utterance 1" in msg, (rc, msg)
            rc, msg = set_prefix([6, 5])
            assert rc == -1 and "utterance 0" in msg, (rc, msg)
            rc, msg = set_prefix([4, 2])
            assert rc == -1 and "no utterance has the 5 prefix frames" in msg, (rc, msg)
            assert set_prefix([5, 2])[0] == 0
            hidden = synth.conditioning(5, "prefix_rows.err", 2 * B, S, d).to(DEV)
            eng.call("zn_prefill", hidden.data_ptr(), S, st)
            rc, msg = set_prefix([5, 2])
            assert rc == -3 and "after zn_prefill" in msg, (rc, msg)
            eng.call("zn_sample_first", st)                                             # the generation goes on after the refused calls
            eng.call("zn_decode_steps", 3, st)
            done = C.c_int32(-1)
            eng.call("zn_all_stopped", C.byref(done), st)
            assert done.value == 0
            torch.cuda.synchronize()
            # first frame + three steps: row 0 wrote columns 6 .. 9, row 1 (shift -3) columns 3 .. 6 and nothing to the right of them
            assert bool((delayed[0, 0, 6:10] >= 0).all()) and bool((delayed[0, 0, 6:10] <= EOS).all())
            assert bool((delayed[1, 0, 3:7] >= 0).all()) and bool((delayed[1, 0, 3:7] <= EOS).all()) and bool((delayed[1, 0, 7:10] == -1).all())
            assert bool((delayed[0, 0, 10:13] == -1).all())
        finally:
            torch.cuda.synchronize()
            eng.call("zn_gen_end")
        again, _ = _batch(model, reqs, ragged=True)
        assert all(torch.equal(a, g) for a, g in zip(again, good))


# ------------------------------------------------------------------------------------------------ 7. the default is unchanged
@pytest.mark.parametrize("arch", ["transformer", "hybrid"])
def test_equal_prefixes_give_the_default_paths_bits(models, arch):
    """Equal prefixes: generate_batch(reqs) and generate_batch(reqs, ragged_prefix=True) return the same codes and logits - every shift is
    0, the kernels get no shift array, and the assembled prefill rows carry the bits of the rows the host used to build."""
    model = models(arch)
    d = CFGS[arch]["d_model"]
    for P in (3, 0):
        reqs = [GenRequest(_utt(510 + b, [10, 14, 11][b], d).to(DEV), sampling_params=dict(temperature=0.0, repetition_penalty=PENALTY[b]),
                           cfg_scale=SCALE[b], max_new_tokens=BUDGET[b], audio_prefix_codes=_prefix(810 + b, P)) for b in range(3)]
        with _hooks(model, 3, arch):
            base, bl = _batch(model, reqs, ragged=False)
            same, sl = _batch(model, reqs, ragged=True)
        assert all(torch.equal(a, b) for a, b in zip(base, same)) and _same_bits(bl, sl), P
