"""Zonos.serve(): requests join a running batch as slots free up (zn_gen_open_slots, zn_gen_admit, zn_gen_retire, zn_gen_row_state;
DESIGN.md 4.1e).  Everything is asserted bit for bit, codes and per-step logits, on seeded synthetic weights.  The reference for a request
r is always existing code: a generate_batch(..., ragged_prefix=True) call of `slots` requests that holds r in some slot, beside mates of
r's own conditioning length, budget and prefix length (arbitrary codes).  A session's logits for r are those of the admission that brought
it and of the steps during which it held its slot, in order: r's own step index.

Comparability.  The transformer's prefill projections pick their kernel by M = rows x positions (tests/test_gpu_ragged.py `_gemm_class`);
an admission prefills n * halves rows of S positions, the reference call slots * halves rows.  Every case keeps every such M <= 64 and
asserts it.  The hybrid backbone prefills in mode 2 (projections row by row: independent of M)."""
import ctypes as C

import pytest
import torch

from zonos_amd import _lib, synth
from zonos_amd.codebook_pattern import apply_delay_pattern
from zonos_amd.conditioning import pad_conditionings
from zonos_amd.model import GenRequest, ServeResult, _sampling_struct
from zonos_amd.serving import serve_slack
from zonos_amd.testing import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NQ, V, EOS, MASK = 9, 1025, 1024, 1025
CFGS = {"transformer": synth.TINY_CFG, "hybrid": synth.HYBRID_TINY_CFG, "chain": synth.CHAIN_CFG}
SEEDS = {"transformer": 77, "hybrid": 23, "chain": 91}
ARCHS = ["transformer", "hybrid"]


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
    return synth.conditioning(seed, "serve.cond", halves, L, d)


def _prefix(seed, P):
    return None if P == 0 else torch.from_numpy(synth.randint(seed, "serve.prefix", (1, NQ, P), 1024))


def _gemm_class(M):
    return 0 if M <= 64 else 1 if M <= 255 else 2


def _plen(r):
    return 0 if r.audio_prefix_codes is None else int(r.audio_prefix_codes.shape[2])


def _row_len(r):
    return int(r.conditioning.shape[1]) + _plen(r) + 1


class _hooks:
    """EOS suppressed (and, optionally, forced at one loop step) on the engine that serves `slots` utterances; the hybrid backbone
    prefills row by row; no hand-off timeout may have been counted at the end."""
    def __init__(self, model, slots, arch, force=-1, suppress=True):
        self.eng, self.arch, self.force, self.suppress = model.engine(slots), arch, force, suppress

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


def _requests(arch, guided, Ls, budgets, prefixes, base=400, stochastic=()):
    d, halves = CFGS[arch]["d_model"], 2 if guided else 1
    reqs = []
    for i, (L, n, P) in enumerate(zip(Ls, budgets, prefixes)):
        sp, seed = dict(temperature=0.0, repetition_penalty=[1.0, 3.0, 5.0, 2.0, 1.5][i % 5]), None
        if i in stochastic:
            sp, seed = dict(temperature=0.9, min_p=0.05, repetition_penalty=2.0), 4242 + i
        reqs.append(GenRequest(_utt(base + i, L, d, halves).to(DEV), sampling_params=sp, seed=seed, cfg_scale=[1.5, 2.0, 3.0, 2.5, 1.25][i % 5] if guided else 1.0,
                               max_new_tokens=n, audio_prefix_codes=_prefix(base + 400 + i, P)))
    return reqs


def _serve(model, source, slots, guided, sched_every=8, trace=True, max_prompt=None, max_new=None):
    """serve() to its end -> ({index: ServeResult}, trace, order of completion)."""
    reqs = [r for r in source if r is not None]
    max_prompt = max(_row_len(r) - 1 for r in reqs) if max_prompt is None else max_prompt
    max_new = max(int(r.max_new_tokens) for r in reqs) if max_new is None else max_new
    tr = {} if trace else None
    out, order = {}, []
    for res in model.serve(iter(source), slots=slots, max_prompt=max_prompt, max_new_tokens=max_new, guided=guided, sched_every=sched_every, _trace=tr):
        assert isinstance(res, ServeResult) and res.index not in out
        out[res.index] = res
        order.append(res.index)
    return out, tr, order


def _request_logits(tr, index):
    """The logits of request `index`: its admission's, then those of every step it held its slot."""
    rows = [lg[b].cpu() for lg, (_, _, held) in zip(tr["logits"], tr["slots"]) for b, who in enumerate(held) if who == index]
    return torch.stack(rows)


def _step0(tr, index):
    return next(step for kind, step, held in tr["slots"] if kind == "admit" and index in held)


def _reference(model, arch, r, i, slots, guided):
    """generate_batch(ragged_prefix=True) of `slots` requests holding r at position i % slots -> (codes, logits [calls, 9, 1025])."""
    d, halves, pos = CFGS[arch]["d_model"], 2 if guided else 1, i % slots
    if arch == "transformer":
        assert _gemm_class(slots * halves * _row_len(r)) == 0
    mates = [GenRequest(_utt(7000 + 10 * i + k, int(r.conditioning.shape[1]), d, halves).to(DEV), sampling_params=r.sampling_params, seed=r.seed, cfg_scale=r.cfg_scale,
                        max_new_tokens=r.max_new_tokens, audio_prefix_codes=_prefix(7500 + 10 * i + k, _plen(r))) for k in range(slots - 1)]
    call = mates[:pos] + [r] + mates[pos:]
    tr = {"logits": []}
    outs = model.generate_batch(call, ragged_prefix=True, _trace=tr)
    return outs[pos].cpu(), torch.stack([lg[pos].cpu() for lg in tr["logits"]])


def _check_request(model, arch, r, i, slots, guided, res, tr, force_at=None):
    if force_at is None:
        ref, rl = _reference(model, arch, r, i, slots, guided)
    else:
        eng = model.engine(slots)
        eng.call("zn_debug_force_eos", force_at)
        ref, rl = _reference(model, arch, r, i, slots, guided)
    assert res.error is None and torch.equal(res.codes.cpu(), ref), f"request {i}: codes differ from its generate_batch call's"
    got = _request_logits(tr, i)
    assert got.shape[0] >= rl.shape[0], f"request {i}: retired after {got.shape[0] - 1} own steps, its call ran {rl.shape[0] - 1}"
    assert _same_bits(got[:rl.shape[0]], rl), f"request {i}: logits differ from its generate_batch call's"
    return ref


def _admission_classes(tr, reqs, halves):
    """Every admission of the session prefilled M = n * halves * S rows in projection class 0."""
    for kind, _, held in tr["slots"]:
        if kind == "admit":
            who = [h for h in held if h is not None]
            assert _gemm_class(len(who) * halves * max(_row_len(reqs[h]) for h in who)) == 0


# ------------------------------------------------------------------------------------------------ 1. all admitted at the start
@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("guided", [True, False], ids=["guided", "cfg1"])
def test_three_requests_in_three_slots_equal_generate_batch(models, arch, guided):
    model = models(arch)
    reqs = _requests(arch, guided, [6, 9, 4], [6, 14, 9], [1, 0, 5], stochastic=(1,))
    halves = 2 if guided else 1
    assert _gemm_class(3 * halves * max(_row_len(r) for r in reqs)) == 0
    with _hooks(model, 3, arch):
        out, tr, _ = _serve(model, reqs, 3, guided)
        btr = {"logits": []}
        ref = [o.cpu() for o in model.generate_batch(reqs, ragged_prefix=True, _trace=btr)]
    assert tr["slots"][0] == ("admit", 0, [0, 1, 2])
    for i in range(3):
        assert torch.equal(out[i].codes.cpu(), ref[i]), i
        got, rl = _request_logits(tr, i), torch.stack([lg[i].cpu() for lg in btr["logits"]])
        n = min(got.shape[0], rl.shape[0])
        assert n >= int(reqs[i].max_new_tokens) + NQ - 1 and _same_bits(got[:n], rl[:n]), i
        assert tuple(out[i].codes.shape) == (1, NQ, _plen(reqs[i]) + int(reqs[i].max_new_tokens))


# ------------------------------------------------------------------------------------------------ 2. refill
REFILL_L, REFILL_BUDGET, REFILL_PREFIX = [6, 10, 3, 9, 12], [6, 14, 9, 11, 7], [5, 0, 12, 1, 0]


@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("slots,guided", [(2, True), (3, False)], ids=["2slots-guided", "3slots-cfg1"])
def test_refilled_slots_equal_their_generate_batch_calls(models, arch, slots, guided):
    """Five requests through two or three slots, EOS suppressed: every request - admitted at the start, admitted into a freed slot, or
    running on beside an admission - equals its reference call in codes and logits."""
    model = models(arch)
    reqs = _requests(arch, guided, REFILL_L, REFILL_BUDGET, REFILL_PREFIX, stochastic=(1, 3))
    with _hooks(model, slots, arch):
        out, tr, order = _serve(model, reqs, slots, guided)
        if arch == "transformer":
            _admission_classes(tr, reqs, 2 if guided else 1)
        for i, r in enumerate(reqs):
            ref = _check_request(model, arch, r, i, slots, guided, out[i], tr)
            assert tuple(ref.shape) == (1, NQ, REFILL_PREFIX[i] + REFILL_BUDGET[i])
        fast, _, order2 = _serve(model, reqs, slots, guided, trace=False)           # eight steps per enqueue, as captured graphs
        assert order2 == order and all(torch.equal(fast[i].codes, out[i].codes) for i in range(5))
    assert sorted(out) == [0, 1, 2, 3, 4]
    admits = [(step, [h for h in held if h is not None]) for kind, step, held in tr["slots"] if kind == "admit"]
    assert any(len(who) >= 2 for _, who in admits), "one admission must bring two requests at once"
    mid = False
    for k, (kind, step, held) in enumerate(tr["slots"]):
        if kind == "admit" and step > 0:
            before, after = tr["slots"][k - 1][2], tr["slots"][k + 1][2]
            mid = mid or any(b is not None and b == a and b not in held for b, a in zip(before, after))
    assert mid, "one request must be admitted while another row is mid-utterance"


# ------------------------------------------------------------------------------------------------ 3. the random stream knows neither slot nor time
@pytest.mark.parametrize("arch", ARCHS)
def test_a_seeded_request_draws_the_same_stream_first_and_last(models, arch):
    model = models(arch)
    d = CFGS[arch]["d_model"]
    star = GenRequest(_utt(610, 8, d).to(DEV), sampling_params=dict(temperature=0.9, min_p=0.05), seed=1234, cfg_scale=2.0, max_new_tokens=12,
                      audio_prefix_codes=_prefix(611, 1))
    others = _requests(arch, True, [6, 10, 9], [6, 14, 9], [5, 0, 1], base=620)
    with _hooks(model, 2, arch):
        first, tr1, _ = _serve(model, [star] + others, 2, True)
        last, tr2, _ = _serve(model, others + [star], 2, True)
        assert _step0(tr1, 0) == 0 and _step0(tr2, 3) > 0
        ref = _check_request(model, arch, star, 0, 2, True, first[0], tr1)
        _check_request(model, arch, star, 3, 2, True, last[3], tr2)
    assert torch.equal(first[0].codes, last[3].codes) and torch.equal(first[0].codes.cpu(), ref)
    greedy = GenRequest(star.conditioning, sampling_params=dict(temperature=0.0), cfg_scale=2.0, max_new_tokens=12, audio_prefix_codes=star.audio_prefix_codes)
    with _hooks(model, 2, arch):
        g, _, _ = _serve(model, [greedy], 2, True, trace=False)
    assert not torch.equal(g[0].codes, first[0].codes), "the temperature must decide tokens"


# ------------------------------------------------------------------------------------------------ 4. stops per row
@pytest.mark.parametrize("arch", ARCHS)
def test_a_forced_eos_stops_each_row_at_its_own_step(models, arch):
    """zn_debug_force_eos at session step 12 of a two-slot session scheduled every 4 steps: request 0 (3 frames) has left at step 12 and
    request 2 takes its slot there, so the hook meets request 1 at its own step 12 and request 2 at its own step 0.  Each equals its
    reference call run with the hook at its own step 12 - step0; requests admitted later run to their budgets."""
    model = models(arch)
    K = 12
    budgets = [3, 14, 9, 11, 7]
    reqs = _requests(arch, True, REFILL_L, budgets, REFILL_PREFIX)
    with _hooks(model, 2, arch, force=K):
        out, tr, _ = _serve(model, reqs, 2, True, sched_every=4)
        ages = {}
        for i, r in enumerate(reqs):
            own = K - _step0(tr, i)
            ages[i] = own
            ref = _check_request(model, arch, r, i, 2, True, out[i], tr, force_at=own if own >= 0 else -1)
            assert ref.shape[2] <= REFILL_PREFIX[i] + budgets[i]
            if own < 0:
                assert ref.shape[2] == REFILL_PREFIX[i] + budgets[i], "a request admitted after the hook runs to its budget"
    alive = [i for i, own in ages.items() if 0 <= own <= budgets[i] - 2]          # the step samples a frame inside the request's budget
    assert len({ages[i] for i in alive}) >= 2, f"rows of different ages must be alive at the hook: {ages}"
    assert all(out[i].codes.shape[2] < REFILL_PREFIX[i] + budgets[i] for i in alive)
    assert any(own < 0 for own in ages.values())


# ------------------------------------------------------------------------------------------------ the ABI, driven directly
class _Session:
    """A slotted session through the C ABI, as Zonos.serve() drives it."""
    def __init__(self, model, slots, guided, max_len, width, slack, caches=None, lengths=None):
        self.model, self.slots, self.guided, self.halves = model, slots, guided, 2 if guided else 1
        self.eng = model.engine(slots)
        self.lib, self.h, self.st = self.eng.lib, self.eng.h, self.eng.stream()
        self.R, self.width, self.slack, self.max_len = slots * self.halves, width, slack, max_len
        n_layer = model.config.backbone.n_layer
        if caches is None:
            self.ip = model.setup_cache(batch_size=self.R, max_seqlen=max_len)
            assert self.ip.max_seqlen == max_len
            caches = [self.ip.key_value_memory_dict[i][0] for i in range(n_layer)]
        self.caches = caches
        self.lengths = torch.zeros(self.R, dtype=torch.int32, device=DEV)
        self.delayed = torch.full((slots, NQ, width), MASK, dtype=torch.int32, device=DEV)
        kv = (C.c_void_p * n_layer)(*[c.data_ptr() for c in caches])
        sp = _sampling_struct({}, 0)
        self.eng.call("zn_gen_begin", slots, kv, max_len, self.lengths.data_ptr(), self.delayed.data_ptr(), width, 1, width - NQ, 2.0 if guided else 1.0,
                      C.byref(sp), self.st)
        self.keep = []

    def err(self):
        return self.lib.zn_last_error(self.h).decode()

    def open(self):
        return self.lib.zn_gen_open_slots(self.h, self.slack)

    def admit(self, items, write_rows=True, row_len_delta=0):
        """items: [(slot, request)] -> status of zn_gen_admit."""
        n, d = len(items), self.model.config.backbone.d_model
        reqs = [r for _, r in items]
        Ls, Ps = [int(r.conditioning.shape[1]) for r in reqs], [_plen(r) for r in reqs]
        cond, _ = pad_conditionings([r.conditioning.to(DEV) for r in reqs], 2.0 if self.guided else 1.0)
        cond = cond.to(torch.bfloat16).contiguous()
        codes = torch.full((n, NQ, self.width - NQ), MASK, dtype=torch.int32, device=DEV)
        for j, r in enumerate(reqs):
            if Ps[j]:
                codes[j, :, :Ps[j]] = r.audio_prefix_codes[0].to(device=DEV, dtype=torch.int32)
            codes[j, :, Ps[j]:Ps[j] + int(r.max_new_tokens)] = -1
        rows = apply_delay_pattern(codes, MASK).contiguous()
        adm = (_lib.zn_admit * n)()
        for j, (slot, r) in enumerate(items):
            if write_rows:
                self.delayed[slot].copy_(rows[j])
            adm[j].slot, adm[j].row_len, adm[j].prefix_len = slot, Ls[j] + Ps[j] + 1 + row_len_delta, Ps[j]
            adm[j].params.sp = _sampling_struct(r.sampling_params, 0 if r.seed is None else r.seed)
            adm[j].params.cfg_scale, adm[j].params.max_new_tokens = float(r.cfg_scale), int(r.max_new_tokens)
        S = max(L + P + 1 for L, P in zip(Ls, Ps)) + row_len_delta
        meta = torch.tensor([Ls, Ps], dtype=torch.int32).to(DEV)
        hidden = torch.zeros(self.halves * n, S, d, dtype=torch.bfloat16, device=DEV)
        row_len = torch.empty(self.halves * n, dtype=torch.int32, device=DEV)
        self.eng.call("zn_op_assemble_prefill", cond.data_ptr(), cond.shape[1], meta[0].data_ptr(), rows.data_ptr(), self.width, meta[1].data_ptr(), n,
                      self.halves * n, hidden.data_ptr(), S, row_len.data_ptr(), self.st)
        self.keep = [cond, rows, hidden, row_len, meta]
        return self.lib.zn_gen_admit(self.h, adm, n, hidden.data_ptr(), S, self.st)

    def steps(self, n):
        self.eng.call("zn_decode_steps", n, self.st)

    def state(self):
        rem, own = (C.c_int32 * self.slots)(), (C.c_int32 * self.slots)()
        self.eng.call("zn_gen_row_state", rem, own, self.st)
        return list(rem), list(own)

    def retire(self, slot):
        return self.lib.zn_gen_retire(self.h, slot)

    def result(self, slot, r):
        return self.model._finalise_row(self.delayed[slot:slot + 1].cpu(), _plen(r), int(r.max_new_tokens), self.slots, NQ)[0]

    def run_to_end(self, slot, r):
        """Steps until request r in `slot` has left its own loop (eight at a time), retires it -> (codes, steps run)."""
        need, ran = int(r.max_new_tokens) + NQ - 1, 0
        while ran < need:                                   # EOS suppressed: the row ends on its budget (row_end_offset == t_b)
            self.steps(8)
            ran += 8
        rem, own = self.state()
        assert rem[slot] <= 0 and own[slot] == ran, (rem, own, ran)
        codes = self.result(slot, r)
        assert self.retire(slot) == 0, self.err()
        return codes, ran

    def end(self):
        torch.cuda.synchronize()
        self.eng.call("zn_gen_end")


# ------------------------------------------------------------------------------------------------ 5. an idle row stays in its cache
@pytest.mark.parametrize("arch", ARCHS)
def test_an_idle_slot_stays_inside_its_own_cache_rows(models, arch):
    """Two guided slots, max_len 48.  Every layer's cache is a view into one tensor with a guard region behind the layer's last row, filled
    with a fixed pattern and longer than every position the session's steps could reach.  Slot 0 runs one request of 3 frames and is
    retired; slot 1 is refilled until the session has run more than 2 * max_len steps.  Every slot-1 request equals its reference, every
    guard byte is unchanged, and slot 0 reports length 0 (step count -1) throughout."""
    model = models(arch)
    d, n_layer, max_len, slots, R = CFGS[arch]["d_model"], model.config.backbone.n_layer, 48, 2, 4
    slack = serve_slack(8)
    width = 5 + 8 + NQ + slack
    probe = model.setup_cache(batch_size=R, max_seqlen=max_len)
    sizes = []
    for i in range(n_layer):
        a, b = probe.key_value_memory_dict[i]
        sizes.append(a.numel() * 2 + (0 if b is None else b.numel() * 2))
    total_steps = 2 * max_len + 40
    pos_bytes = 2 * CFGS[arch]["num_heads_kv"] * (d // CFGS[arch]["num_heads"]) * 2
    guard = (total_steps + 8) * pos_bytes
    assert guard % 256 == 0 and all(s % 256 == 0 for s in sizes)
    big = torch.full((sum(sizes) + n_layer * guard,), 0x5A, dtype=torch.uint8, device=DEV)
    caches, guards, at = [], [], 0
    for s in sizes:
        caches.append(big[at:at + s])
        caches[-1].zero_()                                  # (Mamba2 state buffers begin at zero, as allocate_inference_cache leaves them)
        guards.append(big[at + s:at + s + guard])
        at += s + guard
    short = _requests(arch, True, [5], [3], [0], base=700)[0]
    fills = _requests(arch, True, [6, 4, 7, 5, 6, 4, 7, 5], [8, 5, 7, 6, 8, 5, 7, 6], [1, 5, 0, 1, 1, 5, 0, 1], base=710)      # L + P + budget <= 15: each fits max_len 48 exactly or with room
    with _hooks(model, slots, arch):
        s = _Session(model, slots, True, max_len, width, slack, caches=caches)
        results, ran = [], 0
        try:
            assert s.open() == 0, s.err()
            assert s.admit([(0, short), (1, fills[0])]) == 0, s.err()
            k = 0
            while True:
                codes, n = s.run_to_end(1, fills[k])
                ran += n
                results.append(codes)
                rem, own = s.state()
                if k == 0:
                    assert own[0] == n and rem[0] <= 0
                    first = s.result(0, short)
                    assert s.retire(0) == 0, s.err()
                else:
                    assert own[0] == -1 and rem[0] <= 0
                assert int(s.lengths[0]) == 0 or k == 0
                if ran > 2 * max_len:
                    break
                k += 1
                assert k < len(fills)
                assert s.admit([(1, fills[k])]) == 0, s.err()
                assert int(s.lengths[0]) == 0 and int(s.lengths[2]) == 0, "an idle slot's rows report length 0"
                assert s.state()[1][0] == -1
            assert ran <= total_steps
            assert int(s.lengths[0]) == 0 and int(s.lengths[2]) == 0
        finally:
            s.end()
        for g in guards:
            assert bool((g == 0x5A).all()), "a write left its layer's cache"
        ref, _ = _reference(model, arch, short, 0, slots, True)
        assert torch.equal(first, ref)
        for k, codes in enumerate(results):
            ref, _ = _reference(model, arch, fills[k], 1, slots, True)
            assert torch.equal(codes, ref), f"slot-1 request {k} differs from its reference"


# ------------------------------------------------------------------------------------------------ 6. errors are statuses
@pytest.mark.parametrize("arch", ARCHS)
def test_session_errors_are_statuses_and_leave_the_session_usable(models, arch):
    model = models(arch)
    slack = serve_slack(8)
    a, b = _requests(arch, True, [6, 5], [6, 8], [1, 0], base=740)
    max_len, width = 48, 1 + 8 + NQ + slack                              # b fits both exactly: 5 + 0 + 8 + 9 + 24 = 46 <= 48; 0 + 8 + 9 + 24 = 41 <= 42
    fit_len = GenRequest(_utt(745, 7, CFGS[arch]["d_model"]).to(DEV), sampling_params=dict(temperature=0.0), cfg_scale=2.0, max_new_tokens=8)      # 7 + 8 + 9 + 24 = 48
    long_len = GenRequest(_utt(745, 8, CFGS[arch]["d_model"]).to(DEV), sampling_params=dict(temperature=0.0), cfg_scale=2.0, max_new_tokens=8)     # 49
    long_w = GenRequest(_utt(746, 3, CFGS[arch]["d_model"]).to(DEV), sampling_params=dict(temperature=0.0), cfg_scale=2.0, max_new_tokens=9)       # width: 0 + 9 + 9 + 24 = 42 fits
    long_w1 = GenRequest(_utt(746, 3, CFGS[arch]["d_model"]).to(DEV), sampling_params=dict(temperature=0.0), cfg_scale=2.0, max_new_tokens=10)     # 43 > 42
    unguided = GenRequest(_utt(747, 5, CFGS[arch]["d_model"]).to(DEV), sampling_params=dict(temperature=0.0), cfg_scale=1.0, max_new_tokens=4)
    with _hooks(model, 2, arch):
        s = _Session(model, 2, True, max_len, width, slack)
        try:
            rc = s.admit([(0, a)], write_rows=False)
            assert rc == -3 and "zn_gen_open_slots" in s.err(), (rc, s.err())              # admit without a session
            assert s.retire(0) == -3
        finally:
            s.end()
        s = _Session(model, 2, True, max_len, width, slack)
        try:
            hidden = synth.conditioning(5, "serve.err", 4, 7, CFGS[arch]["d_model"]).to(DEV)
            s.eng.call("zn_prefill", hidden.data_ptr(), 7, s.st)
            rc = s.open()
            assert rc == -3 and "after zn_prefill" in s.err(), (rc, s.err())               # zn_gen_open_slots after a prefill
        finally:
            s.end()
        s = _Session(model, 2, True, max_len, width, slack)
        try:
            assert s.open() == 0, s.err()
            assert s.retire(1) == -3 and "slot 1 is idle" in s.err()                       # retire an idle slot
            rc = s.admit([(0, a), (0, b)], write_rows=False)
            assert rc == -1 and "slot 0 named twice" in s.err(), (rc, s.err())
            rc = s.admit([(2, a)], write_rows=False)
            assert rc == -1 and "slot 2 out of range" in s.err(), (rc, s.err())
            rc = s.admit([(1, long_len)], write_rows=False)
            assert rc == -1 and "slot 1" in s.err() and "max_len 48" in s.err(), (rc, s.err())
            rc = s.admit([(1, long_w1)], write_rows=False)
            assert rc == -1 and "slot 1" in s.err() and "width 42" in s.err(), (rc, s.err())
            rc = s.admit([(1, unguided)], write_rows=False)
            assert rc == -1 and "slot 1 has cfg_scale 1" in s.err(), (rc, s.err())
            assert s.state() == ([0, 0], [-1, -1])                                        # the refused calls left every slot idle
            assert s.admit([(0, a)]) == 0, s.err()
            rc = s.admit([(0, b)], write_rows=False)
            assert rc == -3 and "slot 0 is busy" in s.err(), (rc, s.err())
            assert s.admit([(1, b)]) == 0, s.err()                                         # the session goes on after the refused calls
            s.steps(16)
            rem, own = s.state()
            assert own == [16, 16] and rem[0] <= 0 and rem[1] <= 0
            got_a, got_b = s.result(0, a), s.result(1, b)
            assert s.retire(0) == 0 and s.retire(1) == 0
            for slot, r in ((0, fit_len), (1, long_w)):                                    # the capacity rule at its boundary: these fit
                assert s.admit([(slot, r)]) == 0, s.err()
            s.steps(24)
            assert s.state()[1] == [24, 24]
            fit = [s.result(0, fit_len), s.result(1, long_w)]
        finally:
            s.end()
        for got, r, i in ((got_a, a, 0), (got_b, b, 1), (fit[0], fit_len, 0), (fit[1], long_w, 1)):
            ref, _ = _reference(model, arch, r, i, 2, True)
            assert torch.equal(got, ref), i


# ------------------------------------------------------------------------------------------------ 7. the serve() surface
def test_serve_refuses_per_request_skips_none_and_releases_on_close(models):
    model = models("transformer")
    d = CFGS["transformer"]["d_model"]
    reqs = _requests("transformer", True, [6, 10, 3], [6, 9, 7], [5, 0, 1], base=760)
    too_long = GenRequest(_utt(765, 6, d).to(DEV), sampling_params=dict(temperature=0.0), cfg_scale=2.0, max_new_tokens=30)
    wrong = GenRequest(_utt(766, 6, d, 1).to(DEV), sampling_params=dict(temperature=0.0), cfg_scale=1.0, max_new_tokens=5)
    cond = _utt(767, 7, d).to(DEV)
    with _hooks(model, 2, "transformer"):
        before = model.generate(cond, max_new_tokens=10, cfg_scale=2.0, sampling_params=dict(temperature=0.0)).cpu()
        source = [reqs[0], too_long, None, reqs[1], None, wrong, None, reqs[2]]
        out, tr, order = _serve(model, source, 2, True, max_prompt=12, max_new=9)
        assert isinstance(out[1].error, ValueError) and out[1].codes is None and "exceed" in str(out[1].error)
        assert isinstance(out[3].error, ValueError) and out[3].codes is None and "cfg_scale" in str(out[3].error)
        assert order.index(1) < order.index(0), "a refusal is reported at once"
        first = tr["slots"][0]
        assert first == ("admit", 0, [0, None]), "a None item ends the scheduling point's admissions"
        for i, r in ((0, reqs[0]), (2, reqs[1]), (4, reqs[2])):
            _check_request(model, "transformer", r, i, 2, True, out[i], tr)
        gen = model.serve(iter(reqs), slots=2, max_prompt=12, max_new_tokens=9, guided=True)
        got = next(gen)
        assert got.error is None and got.index in (0, 1)
        eng = model.engine(2)
        assert eng.generating, "the engine is held while the generator is alive"
        gen.close()
        assert not eng.generating
        after = model.generate(cond, max_new_tokens=10, cfg_scale=2.0, sampling_params=dict(temperature=0.0)).cpu()
    assert torch.equal(before, after)


@pytest.mark.parametrize("slots,guided", [(1, True), (2, False)], ids=["1slot-guided", "2slots-cfg1"])
def test_a_session_never_runs_the_persistent_kernels(models, slots, guided):
    """Two rows on the model the chain kernel serves: a session reports zn_decode_path_detail 0; generate_batch and generate on the same
    engine report the persistent path afterwards."""
    model = models("chain")
    d, halves = CFGS["chain"]["d_model"], 2 if guided else 1
    eng = model.engine(slots)
    reqs = [GenRequest(_utt(780 + i, 8, d, halves).to(DEV), sampling_params=dict(temperature=0.0), cfg_scale=2.0 if guided else 1.0, max_new_tokens=10)
            for i in range(3)]
    with _hooks(model, slots, "chain"):
        seen = []
        for res in model.serve(iter(reqs), slots=slots, max_prompt=8, max_new_tokens=10, guided=guided):
            assert res.error is None and tuple(res.codes.shape) == (1, NQ, 10)
            seen.append((eng.lib.zn_decode_path_detail(eng.h), eng.lib.zn_decode_path(eng.h)))
        assert len(seen) == 3 and all(p == (0, 0) for p in seen), seen
        if guided:
            model.generate(reqs[0].conditioning, max_new_tokens=10, cfg_scale=2.0, sampling_params=dict(temperature=0.0))
        else:
            model.generate_batch(reqs[:2])
        assert eng.lib.zn_decode_path_detail(eng.h) >= 1 and eng.lib.zn_decode_path(eng.h) == 1


# ------------------------------------------------------------------------------------------------ 8. the default is unchanged
@pytest.mark.parametrize("arch", ARCHS)
def test_a_session_leaves_the_default_paths_bits(models, arch):
    model = models(arch)
    d = CFGS[arch]["d_model"]
    reqs = _requests(arch, True, [6, 9, 4], [6, 14, 9], [1, 0, 5], base=800, stochastic=(1,))
    cond = synth.conditioning(9, "serve.default", 6, 7, d).to(DEV)

    def both():
        tr, tg = {"logits": []}, {"logits": []}
        outs = [o.cpu() for o in model.generate_batch(reqs, ragged_prefix=True, _trace=tr)]
        g = model.generate(cond, max_new_tokens=8, cfg_scale=2.0, batch_size=3, sampling_params=dict(temperature=0.0), seed=3, _trace=tg).cpu()
        return outs, torch.stack([l.cpu() for l in tr["logits"]]), g, torch.stack([l.cpu() for l in tg["logits"]])
    with _hooks(model, 3, arch):
        o1, l1, g1, gl1 = both()
        _serve(model, reqs, 3, True)
        _serve(model, reqs, 3, True, trace=False)
        o2, l2, g2, gl2 = both()
    assert all(torch.equal(a, b) for a, b in zip(o1, o2)) and _same_bits(l1, l2)
    assert torch.equal(g1, g2) and _same_bits(gl1, gl2)
