"""Guided and unguided requests in one call and one session, the parts that need no GPU: what `check_requests` and
`check_serve_request` accept, how `SlotScheduler` places requests of one and two slots, the sampler's logits stage for a row-pair table
(a numpy transcription of sample_kernel's first stage), and the struct that carries the pair."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from zonos_amd import _lib
from zonos_amd.conditioning import pad_conditioning_rows
from zonos_amd.model import MAX_BATCH_REQUESTS, GenRequest, check_requests
from zonos_amd.parallel import request_groups
from zonos_amd.serving import SlotScheduler, check_serve_request

NQ, D = 9, 32


def _req(cfg_scale, halves=None, L=5, n=6, P=0):
    halves = (1 if cfg_scale == 1.0 else 2) if halves is None else halves
    return GenRequest(torch.zeros(halves, L, D), cfg_scale=cfg_scale, max_new_tokens=n,
                      audio_prefix_codes=None if P == 0 else torch.zeros(1, NQ, P, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ check_requests
def test_check_requests_accepts_a_mix_only_with_the_keyword():
    mix = [_req(2.0), _req(1.0), _req(1.0), _req(3.0)]
    assert check_requests(mix, NQ, D, mixed_guidance=True) == (None, 0)
    with pytest.raises(ValueError, match="row layout"):
        check_requests(mix, NQ, D)
    with pytest.raises(ValueError, match="row layout"):
        check_requests(mix, NQ, D, ragged_prefix=True)
    # one kind only: the keyword changes nothing
    assert check_requests([_req(2.0), _req(1.5)], NQ, D, mixed_guidance=True) == (True, 0)
    assert check_requests([_req(1.0), _req(1.0)], NQ, D, mixed_guidance=True) == (False, 0)
    # with ragged prefixes the lengths come back per request
    rag = [_req(2.0, P=3), _req(1.0), _req(1.0, P=1)]
    assert check_requests(rag, NQ, D, ragged_prefix=True, mixed_guidance=True) == (None, [3, 0, 1])
    with pytest.raises(ValueError, match="different lengths"):
        check_requests(rag, NQ, D, mixed_guidance=True)


def test_check_requests_holds_each_conditioning_to_its_own_cfg_scale():
    with pytest.raises(ValueError, match=r"request 1: conditioning of shape \(1, 5, 32\), expected \[2"):
        check_requests([_req(1.0), _req(2.0, halves=1)], NQ, D, mixed_guidance=True)
    with pytest.raises(ValueError, match=r"request 0: conditioning of shape \(2, 5, 32\), expected \[1"):
        check_requests([_req(1.0, halves=2), _req(2.0)], NQ, D, mixed_guidance=True)


def test_check_requests_counts_rows_in_a_mixed_call():
    fits = [_req(2.0)] * (MAX_BATCH_REQUESTS // 2 - 1) + [_req(1.0)] * 2
    assert check_requests(fits, NQ, D, mixed_guidance=True)[0] is None
    with pytest.raises(ValueError, match="rows"):
        check_requests(fits + [_req(1.0)], NQ, D, mixed_guidance=True)


def test_pad_conditioning_rows_lays_requests_out_in_order():
    conds = [torch.full((2, 3, D), 1.0), torch.full((1, 5, D), 2.0), torch.full((2, 4, D), 3.0)]
    conds[0][1] = -1.0
    out, lengths, first = pad_conditioning_rows(conds)
    assert tuple(out.shape) == (5, 5, D) and lengths == [3, 3, 5, 4, 4] and first == [0, 2, 3]
    assert bool((out[0, :3] == 1.0).all()) and bool((out[1, :3] == -1.0).all()) and bool((out[0, 3:] == 0).all())
    assert bool((out[2] == 2.0).all()) and bool((out[3, :4] == 3.0).all()) and bool((out[4, 4:] == 0).all())
    with pytest.raises(ValueError):
        pad_conditioning_rows([torch.zeros(3, 4, D)])


def test_request_groups_stop_splitting_by_guidance():
    reqs = [_req(2.0), _req(1.0), _req(2.0), _req(1.0), _req(1.0)]
    share = list(range(5))
    assert request_groups(reqs, share, 8) == [[0, 2], [1, 3, 4]]
    assert request_groups(reqs, share, 8, mixed_guidance=True) == [[0, 1, 2, 3, 4]]
    assert request_groups(reqs, share, 2, mixed_guidance=True) == [[0, 1], [2, 3], [4]]
    many = [_req(2.0)] * 40
    groups = request_groups(many, list(range(40)), 64, mixed_guidance=True)
    assert [len(g) for g in groups] == [32, 8]                                     # 64 rows per call at most


# ------------------------------------------------------------------------------------------------ check_serve_request
def _serve_check(cond_shape, cfg_scale, guided, prefix_shape=None, n=6):
    return check_serve_request(cond_shape, prefix_shape, n, cfg_scale, nq=NQ, d_model=D, guided=guided, max_len=64, width=48, slack=24)


def test_check_serve_request_in_a_mixed_session():
    assert _serve_check((2, 5, D), 2.0, None) == (5, 0)
    assert _serve_check((1, 7, D), 1.0, None, prefix_shape=(1, NQ, 3)) == (7, 3)
    with pytest.raises(ValueError, match=r"expected \[2"):
        _serve_check((1, 5, D), 2.0, None)
    with pytest.raises(ValueError, match=r"expected \[1"):
        _serve_check((2, 5, D), 1.0, None)
    # the two sessions of one kind keep their refusals
    with pytest.raises(ValueError, match="row layout"):
        _serve_check((1, 5, D), 1.0, True)
    with pytest.raises(ValueError, match="row layout"):
        _serve_check((2, 5, D), 2.0, False)
    with pytest.raises(ValueError, match="KV positions"):
        _serve_check((2, 5, D), 2.0, None, n=40)


# ------------------------------------------------------------------------------------------------ SlotScheduler
def _drive(slots, sched_every, needs, budgets, arrivals, rng):
    """A session over requests needing `needs[i]` slots that run budgets[i] + NQ - 1 steps, request i reaching the queue at scheduling
    point arrivals[i] (non-decreasing).  Returns the log [(point, admitted [(slot, index)], holders after admission, retired [(slot, index)])]."""
    s = SlotScheduler(slots, NQ, sched_every)
    point = [0]

    def source():
        for i in range(len(needs)):
            while arrivals[i] > point[0]:
                yield None
            yield i
    src = source()
    log = []
    for _ in range(10000):
        admitted, refused = s.pull(src, lambda i: (0, budgets[i], needs[i]))
        assert not refused
        partners = {slot: s.partner(slot) for slot, _, _ in admitted}
        holders = s.holders()
        for b in range(slots):                                                      # own_steps of the two slots of a request agree
            if s.partner(b) is not None:
                assert s.own_steps(b) == s.own_steps(s.partner(b)) and s.partner(s.partner(b)) == b
                assert s.is_owner(b) != s.is_owner(s.partner(b)) and holders[b] == holders[s.partner(b)]
        if s.finished():
            log.append((point[0], [(slot, i, partners[slot]) for slot, i, _ in admitted], holders, []))
            break
        retired = []
        if not s.all_idle():
            s.advance()
            rem = [0 if s.rows[b] is not None and s.own_steps(b) >= s.rows[b].max_new_tokens + NQ - 1 else 1 for b in range(slots)]
            for b in s.wants_eos(rem):
                assert s.is_owner(b)
                s.set_eos(b, None)
            before = {b: (s.partner(b), s.own_steps(b)) for b in range(slots)}
            for b, index, end in s.due():
                retired.append((b, index, before[b][0]))
                assert s.rows[b] is None and (before[b][0] is None or s.rows[before[b][0]] is None)   # both slots leave together
        log.append((point[0], [(slot, i, partners[slot]) for slot, i, _ in admitted], holders, retired))
        point[0] += 1
    else:
        raise AssertionError("the session did not end")
    return log


@pytest.mark.parametrize("seed", range(12))
def test_scheduler_places_one_and_two_slot_requests_fifo(seed):
    rng = random.Random(seed)
    slots, sched_every, n = rng.choice([2, 3, 6]), rng.choice([4, 8]), 14
    needs = [rng.choice([1, 2]) for _ in range(n)]
    budgets = [rng.randint(1, 20) for _ in range(n)]
    arrivals, t = [], 0
    for _ in range(n):
        t += rng.choice([0, 0, 0, 1, 2])
        arrivals.append(t)
    log = _drive(slots, sched_every, needs, budgets, arrivals, rng)
    order = [i for _, admitted, _, _ in log for _, i, _ in admitted]
    assert order == list(range(n)), "admission is FIFO: nothing overtakes a request that waits for two slots"
    seen_retired = set()
    busy = {}
    for point, admitted, holders, retired in log:
        for slot, i, partner in admitted:
            assert arrivals[i] <= point
            took = [slot] if partner is None else [slot, partner]
            assert len(took) == needs[i], "a guided request is admitted whole, at one scheduling point"
            assert partner is None or slot < partner
            idle_before = [b for b in range(slots) if b not in busy]
            assert took == idle_before[:needs[i]], "the lowest idle slots"
            for b in took:
                assert b not in busy, "a slot is never double-booked"
                busy[b] = i
        assert holders == [busy.get(b) for b in range(slots)]
        for slot, i, partner in retired:
            for b in ([slot] if partner is None else [slot, partner]):
                assert busy.pop(b) == i
            seen_retired.add(i)
    assert seen_retired == set(range(n)) and not busy


def test_a_guided_request_waits_for_a_second_idle_slot():
    """Three slots, two of them busy: the guided request at the head of the queue waits, and the unguided one behind it does not take the
    idle slot."""
    s = SlotScheduler(3, NQ, 8)
    src = iter(["u0", "u1", "g", "u2"])
    need = {"u0": 1, "u1": 1, "g": 2, "u2": 1}
    budget = {"u0": 4, "u1": 20, "g": 5, "u2": 5}
    accept = lambda r: (0, budget[r], need[r])
    admitted, _ = s.pull(src, accept)
    assert [(slot, r) for slot, _, r in admitted] == [(0, "u0"), (1, "u1")] and s.waiting[1] == "g" and s.free_slots() == [2]
    assert s.pull(src, accept) == ([], []) and s.pulled == 3, "nothing behind the waiting request is pulled"
    s.advance(16)
    s.set_eos(0, None)
    assert s.due() == [(0, 0, 4 + NQ)]
    admitted, _ = s.pull(src, accept)
    assert [(slot, r) for slot, _, r in admitted] == [(0, "g")] and s.partner(0) == 2 and s.waiting is None and not s.is_owner(2)
    assert s.holders() == [2, 1, 2] and s.wants_eos([0, 0, 0]) == [0, 1]
    # a request that needs more slots than the session has is refused, not queued for ever
    one = SlotScheduler(1, NQ, 8)
    admitted, refused = one.pull(iter(["g"]), accept)
    assert not admitted and len(refused) == 1 and "slots" in str(refused[0][1]) and one.finished()


# ------------------------------------------------------------------------------------------------ the sampler's logits stage
def _logits_stage(raw, rows, mix, batch, pairs):
    """sample_kernel's first stage for every utterance u of the launch, fp32 with the kernel's operation order: utterance u reads cc from
    raw row u and uu from raw row u + batch (launch-wide `mix`), or from the rows its entry names, and mixes uu + (cc - uu) * cfg_scale."""
    out = np.empty((batch,) + raw.shape[1:], dtype=np.float32)
    for u in range(batch):
        cfg_scale, word0, word1 = rows[u]
        m, rc, ru = mix, u, u + (batch if mix else 0)
        if pairs and word0 > 0:
            m, rc, ru = 1, word0 - 1, word1 - 1
        cc, uu = raw[rc], raw[ru]
        if m:
            diff = (cc - uu).astype(np.float32)                                     # __fsub_rn
            prod = (diff * np.float32(cfg_scale)).astype(np.float32)                # __fmul_rn
            out[u] = (uu + prod).astype(np.float32)                                 # __fadd_rn
        else:
            out[u] = cc
    return out


def test_pair_table_gives_both_slots_the_guided_mix():
    rng = np.random.default_rng(5)
    raw = rng.standard_normal((6, NQ, 1025)).astype(np.float32) * 3
    # rows: 0 U, (1, 4) G at 2.5 with the unconditional row ABOVE, 2 U, (5, 3) G at 1.25 with the unconditional row BELOW, in the unguided layout
    table = [(1.0, 0, 0), (2.5, 2, 5), (1.0, 0, 0), (1.25, 6, 4), (2.5, 2, 5), (1.25, 6, 4)]
    got = _logits_stage(raw, table, mix=0, batch=6, pairs=1)
    for o, f, scale in ((1, 4, 2.5), (5, 3, 1.25)):
        assert got[o].tobytes() == got[f].tobytes(), "both slots of a pair obtain the same logits"
        guided = _logits_stage(np.stack([raw[o], raw[f]]), [(scale, 0, 0)], mix=1, batch=1, pairs=0)
        assert got[o].tobytes() == guided[0].tobytes(), "bit for bit the guided layout's mix on [raw[o], raw[f]]"
        assert got[o].tobytes() != raw[o].tobytes()
    for u in (0, 2):
        assert got[u].tobytes() == raw[u].tobytes()
    # all words zero: the layout of the launch decides, as before
    plain = [(2.0, 0, 0)] * 3
    assert _logits_stage(raw, plain, 1, 3, 1).tobytes() == _logits_stage(raw, plain, 1, 3, 0).tobytes()
    # the words are not looked at unless the launch follows pairs (zn_op_sample_rows)
    assert _logits_stage(raw, table, 0, 6, 0).tobytes() == raw.tobytes()


# ------------------------------------------------------------------------------------------------ the struct
def test_row_params_keeps_its_size_and_the_abi_its_version():
    assert C.sizeof(_lib.zn_row_params) == 64 == _lib.ZN_ROW_PARAMS_BYTES
    assert _lib.zn_row_params.reserved.offset == 56 and _lib.zn_row_params.reserved.size == 8
    assert _lib.load().zn_abi_version() == 9 == _lib.ZN_ABI_VERSION
    e = _lib.zn_row_params()
    assert (e.reserved[0], e.reserved[1]) == (0, 0)
    e.reserved[0], e.reserved[1] = 4, 2
    words = np.frombuffer(bytes(e), dtype=np.int32)
    assert words[14] == 4 and words[15] == 2
