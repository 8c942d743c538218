"""zonos_amd/rows.py on the CPU: the delayed rows of the code buffer, the zn_row_params table and its seeds, and the three constructors of
`GenCall`."""
import ctypes as C

import pytest
import torch

from zonos_amd import _lib
from zonos_amd.codebook_pattern import revert_delay_pattern
from zonos_amd.rows import GenCall, GenRequest, code_rows, row_table

NQ, MASK, D = 9, 1025, 16


def _prefix(P, salt):
    return None if P == 0 else (torch.arange(NQ * P).reshape(1, NQ, P) * 7 + salt) % 1024


def _req(halves, L=4, **kw):
    kw.setdefault("cfg_scale", 2.0 if halves == 2 else 1.0)
    return GenRequest(torch.randn(halves, L, D, generator=torch.Generator().manual_seed(halves * 100 + L)).to(torch.bfloat16), **kw)


def _bytes(entry):
    return C.string_at(C.addressof(entry), C.sizeof(entry))


def _draw():
    return int(torch.randint(0, 2 ** 62, (1,)).item())


# ------------------------------------------------------------------------------------------------ code_rows
@pytest.mark.parametrize("slack", [0, 24])
@pytest.mark.parametrize("plens, budgets", [([0], [1]), ([3], [4]), ([0, 2, 5], [4, 1, 7])])
def test_code_rows_are_left_aligned_and_independent_of_width_and_neighbours(plens, budgets, slack):
    prefixes = [_prefix(P, 11 * b) for b, P in enumerate(plens)]
    width = max(plens) + max(budgets) + NQ + slack
    rows = code_rows(prefixes, budgets, width, NQ, MASK, "cpu")
    assert rows.dtype == torch.int32 and tuple(rows.shape) == (len(plens), NQ, width) and rows.is_contiguous()
    flat = revert_delay_pattern(rows)
    for b, (P, n) in enumerate(zip(plens, budgets)):
        if P:
            assert torch.equal(flat[b, :, :P], prefixes[b][0].to(torch.int32))
        assert bool((flat[b, :, P:P + n] == -1).all())
        assert bool((flat[b, :, P + n:] == MASK).all())
        alone = code_rows([prefixes[b]], [n], P + n + NQ, NQ, MASK, "cpu")           # the request alone, at its own width
        assert torch.equal(rows[b:b + 1, :, :P + n + NQ], alone)


# ------------------------------------------------------------------------------------------------ row_table
def test_row_table_has_one_entry_per_request():
    reqs = [_req(2, seed=3, max_new_tokens=4, sampling_params=dict(min_p=0.2)),
            _req(2, seed=4, max_new_tokens=9, cfg_scale=3.5, sampling_params=dict(top_k=7, temperature=0.5)),
            _req(2, seed=5, max_new_tokens=6, sampling_params=dict(top_p=0.9, repetition_penalty=1.5, repetition_penalty_window=8))]
    table = row_table(reqs)
    assert len(table) == 3
    assert [e.max_new_tokens for e in table] == [4, 9, 6] and [e.cfg_scale for e in table] == [2.0, 3.5, 2.0]
    assert [e.sp.seed for e in table] == [3, 4, 5]
    assert [tuple(e.reserved) for e in table] == [(0, 0)] * 3
    assert table[0].sp.min_p == pytest.approx(0.2) and table[0].sp.top_k == 0 and table[0].sp.repetition_penalty == 3.0
    assert table[1].sp.top_k == 7 and table[1].sp.temperature == 0.5 and table[1].sp.min_p == 0.0
    assert table[2].sp.top_p == pytest.approx(0.9) and table[2].sp.repetition_penalty == 1.5 and table[2].sp.repetition_penalty_window == 8


def test_row_table_of_a_mixed_call_names_every_pair_twice():
    reqs = [_req(2, seed=1, max_new_tokens=4), _req(1, seed=2, max_new_tokens=5), _req(2, seed=3, max_new_tokens=6)]      # G, U, G
    table = row_table(reqs, [0, 2, 3])
    assert C.sizeof(_lib.zn_row_params) == 64 == _lib.ZN_ROW_PARAMS_BYTES
    assert len(table) == 5
    assert [tuple(e.reserved) for e in table] == [(1, 2), (1, 2), (0, 0), (4, 5), (4, 5)]
    assert _bytes(table[0]) == _bytes(table[1]) and _bytes(table[3]) == _bytes(table[4])
    assert [e.sp.seed for e in table] == [1, 1, 2, 3, 3] and [e.max_new_tokens for e in table] == [4, 4, 5, 6, 6]
    assert [e.cfg_scale for e in table] == [2.0, 2.0, 1.0, 2.0, 2.0]


# ------------------------------------------------------------------------------------------------ seeds
@pytest.mark.parametrize("halves, seeds, first", [((2, 2, 2), [None, 5, None], None), ((2, 1, 2), [None, None, 9], [0, 2, 3])])
def test_one_draw_per_request_without_a_seed_in_request_order(halves, seeds, first):
    reqs = [_req(h, seed=s) for h, s in zip(halves, seeds)]
    torch.manual_seed(7)
    drawn = [_draw(), _draw()]
    state = torch.get_rng_state()
    torch.manual_seed(7)
    table = row_table(reqs, first)
    assert torch.equal(torch.get_rng_state(), state)                 # exactly two draws
    it = iter(drawn)
    per_request = [next(it) if s is None else s for s in seeds]
    assert [e.sp.seed for e in table] == [s for s, h in zip(per_request, halves) for _ in range(h if first is not None else 1)]


# ------------------------------------------------------------------------------------------------ the constructors
def test_a_guided_call_lays_its_rows_out_in_halves():
    reqs = [_req(2, 6, seed=1, max_new_tokens=4), _req(2, 4, seed=2, max_new_tokens=9), _req(2, 5, seed=3, max_new_tokens=6)]
    call = GenCall.batch(reqs, True, False, "cpu")
    assert tuple(call.cond.shape) == (6, 6, D) and call.engine_rows == 6 and call.B == 3
    for b, r in enumerate(reqs):
        L = r.conditioning.shape[1]
        assert torch.equal(call.cond[b, :L], r.conditioning[0]) and torch.equal(call.cond[3 + b, :L], r.conditioning[1])
    assert call.cond_lengths == [6, 4, 5]
    assert call.max_new_tokens == 9 and call.budgets == [4, 9, 6]
    assert call.cadence == 3 and call.request_rows is None and call.cfg_scale == 2.0 and not call.ragged
    assert len(call.table) == 3 and call.prefix_lens == [0, 0, 0] and call.P == 0


def test_a_mixed_call_has_a_row_per_conditioning_row():
    reqs = [_req(2, 6, seed=1, max_new_tokens=4), _req(1, 4, seed=2, max_new_tokens=9), _req(2, 5, seed=3, max_new_tokens=6)]       # G, U, G
    call = GenCall.mixed(reqs, False, "cpu")
    assert call.B == call.engine_rows == call.cond.shape[0] == 5
    assert call.cfg_scale == 1.0 and call.cadence == 3 and call.request_rows == [0, 2, 3]
    assert call.cond_lengths == [6, 6, 4, 5, 5] and call.budgets == [4, 4, 9, 6, 6] and call.max_new_tokens == 9
    assert [tuple(e.reserved) for e in call.table] == [(1, 2), (1, 2), (0, 0), (4, 5), (4, 5)]


def test_a_ragged_call_keeps_each_rows_prefix_length():
    reqs = [_req(2, 6, seed=1, max_new_tokens=4), _req(2, 4, seed=2, max_new_tokens=9, audio_prefix_codes=_prefix(2, 1)),
            _req(2, 5, seed=3, max_new_tokens=6, audio_prefix_codes=_prefix(5, 2))]
    call = GenCall.batch(reqs, True, True, "cpu")
    assert call.ragged and call.prefix_lens == [0, 2, 5] and call.P == 5
    assert call.prefixes[0] is None and call.prefixes[2] is reqs[2].audio_prefix_codes
    mixed = GenCall.mixed([reqs[1], _req(1, 3, seed=4, max_new_tokens=2), reqs[2]], True, "cpu")
    assert mixed.ragged and mixed.prefix_lens == [2, 2, 0, 5, 5] and mixed.P == 5


def test_a_plain_call_shares_prefix_budget_and_sampling():
    cond = torch.zeros(6, 6, D, dtype=torch.bfloat16)
    call = GenCall.plain(cond, _prefix(3, 0), 12, 2.0, 3, dict(min_p=0.1), 42, (6, 4, 5))
    assert call.B == 3 and call.engine_rows == 6 and call.cadence == 3 and call.table is None and not call.ragged
    assert call.prefix_lens == [3, 3, 3] and call.budgets == [12, 12, 12] and call.max_new_tokens == 12 and call.cond_lengths == [6, 4, 5]
    assert call.sp.seed == 42 and call.sp.min_p == pytest.approx(0.1)
