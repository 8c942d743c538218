"""An audio prefix of its own length per request of one generate_batch() call (`ragged_prefix=True`, zn_gen_set_prefix_rows,
zn_op_assemble_prefill) - the parts that need no GPU.

* What `check_requests(..., ragged_prefix=True)` accepts and still refuses.
* The call, transcribed: the left-aligned code buffer, the device's bookkeeping with a column shift per row (frame_update_body) under
  `_decode_loop`'s stop-check cadence, and `GenCall.finalise`'s per-row cut - every row equals the row generated alone with its own prefix
  and budget.
* The new entry points: declared, bound, and refusing bad arguments with a status."""
import os
import re

import numpy as np
import pytest
import torch

from zonos_amd import _lib, synth
from zonos_amd.codebook_pattern import apply_delay_pattern, revert_delay_pattern
from zonos_amd.model import GenRequest, check_requests, finalise_codes, row_end_offset, stop_check_at
from zonos_amd.parallel import generate_sharded_requests, request_groups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ, EOS, MASK = 9, 1024, 1025
D = synth.TINY_CFG["d_model"]


# ---------------------------------------------------------------------------------------------------- request validation
def _req(cseed, L=6, halves=2, P=None, **kw):
    pre = None if P is None else torch.from_numpy(synth.randint(cseed, "prefix_rows.prefix", (1, NQ, P), 1024))
    return GenRequest(synth.conditioning(cseed, "prefix_rows.cond", halves, L, D), audio_prefix_codes=pre, **kw)


def test_check_requests_accepts_mixed_prefixes_only_when_asked():
    reqs = [_req(1, P=3), _req(2), _req(3, P=12), _req(4, P=0)]
    assert check_requests(reqs, NQ, D, ragged_prefix=True) == (True, [3, 0, 12, 0])
    assert check_requests(reqs, NQ, D, True) == (True, [3, 0, 12, 0])
    with pytest.raises(ValueError, match="audio prefixes of different lengths"):
        check_requests(reqs, NQ, D)                                                    # the default refuses, with the message callers know
    with pytest.raises(ValueError, match="audio prefixes of different lengths"):
        check_requests(reqs, NQ, D, ragged_prefix=False)
    assert check_requests([_req(1, P=3), _req(2, P=3)], NQ, D) == (True, 3)            # the default's two values are what they were
    assert check_requests([_req(1, P=3), _req(2, P=3)], NQ, D, ragged_prefix=True) == (True, [3, 3])
    unguided = [_req(1, halves=1, cfg_scale=1.0, P=2), _req(2, halves=1, cfg_scale=1.0)]
    assert check_requests(unguided, NQ, D, ragged_prefix=True) == (False, [2, 0])


def test_check_requests_still_refuses_the_rest_with_mixed_prefixes():
    with pytest.raises(ValueError, match="cfg_scale == 1"):
        check_requests([_req(1, P=3), _req(2, halves=1, cfg_scale=1.0)], NQ, D, ragged_prefix=True)
    bad_rank = _req(2)
    bad_rank.audio_prefix_codes = torch.zeros(NQ, 4, dtype=torch.long)
    with pytest.raises(ValueError, match=r"audio_prefix_codes of shape"):
        check_requests([_req(1, P=3), bad_rank], NQ, D, ragged_prefix=True)
    bad_nq = _req(3)
    bad_nq.audio_prefix_codes = torch.zeros(1, NQ - 1, 4, dtype=torch.long)
    with pytest.raises(ValueError, match=r"audio_prefix_codes of shape"):
        check_requests([_req(1, P=3), bad_nq], NQ, D, ragged_prefix=True)
    two = _req(4)
    two.audio_prefix_codes = torch.zeros(2, NQ, 4, dtype=torch.long)
    with pytest.raises(ValueError, match=r"audio_prefix_codes of shape"):
        check_requests([_req(1, P=3), two], NQ, D, ragged_prefix=True)
    with pytest.raises(ValueError, match="no requests"):
        check_requests([], NQ, D, ragged_prefix=True)
    with pytest.raises(ValueError, match="max_new_tokens"):
        check_requests([_req(1, P=3), _req(2, max_new_tokens=0)], NQ, D, ragged_prefix=True)


def test_generate_batch_takes_the_keyword_and_keeps_the_default_refusal():
    from zonos_amd.testing import build_model
    model, _ = build_model(synth.TINY_CFG, 77, "cpu")
    mixed = [_req(1, P=3, max_new_tokens=5), _req(2, max_new_tokens=7)]
    with pytest.raises(ValueError, match="audio prefixes of different lengths"):
        model.generate_batch(mixed)
    with pytest.raises(_lib.ZonosHipError, match="MI355X only"):                       # accepted: on to the device check (no GPU here)
        model.generate_batch(mixed, ragged_prefix=True)
    with pytest.raises(ValueError, match="cfg_scale == 1"):
        model.generate_batch([_req(1, P=3), _req(2, halves=1, cfg_scale=1.0)], ragged_prefix=True)


def test_sharded_requests_pass_the_keyword_through():
    """With ragged_prefix the groups no longer split by prefix length, and every call carries the keyword."""
    reqs = [_req(i, L=4 + i % 3, P=(None, 2, 5)[i % 3], max_new_tokens=3 + i) for i in range(7)]
    assert len(request_groups(reqs, list(range(7)), 8)) == 3
    assert request_groups(reqs, list(range(7)), 8, ragged_prefix=True) == [list(range(7))]
    calls = []

    def fake(batch, ragged_prefix=False):
        calls.append((len(batch), ragged_prefix))
        return [torch.full((1, NQ, r.max_new_tokens), r.max_new_tokens, dtype=torch.int64) for r in batch]
    out = generate_sharded_requests(fake, reqs, batch_size=4, ragged_prefix=True)
    assert calls == [(4, True), (3, True)]
    assert [tuple(o.shape) for o in out] == [(NQ, 3 + i) for i in range(7)]
    calls.clear()
    generate_sharded_requests(fake, reqs, batch_size=4)
    assert all(not kw for _, kw in calls) and sorted(n for n, _ in calls) == [2, 2, 3]


# ---------------------------------------------------------------------------------------------------- the call, transcribed
def run_call(tokens: np.ndarray, budgets, prefixes, cadence_B: int, deferred: bool):
    """One generate_batch(ragged_prefix=True) call of len(budgets) rows on scripted raw tokens [calls, rows, 9] (call 0 = the first frame).
    `prefixes`: per row, int array [9, P_b] (P_b may be 0).  The host's buffer (`Zonos._generation`): row b left-aligned - its prefix, its
    budgets[b] unknown cells, the mask token up to P_call + max(budgets) - under the delay pattern; zn_gen_begin gets offset0 = P_call + 1.
    The device (zn_decode_kernels.h frame_update_body with FrameArgs::shift): at loop state `o` row b's column is o + shift[b],
    shift[b] = P_b - P_call; the first frame is a plain write into that column, loop step i writes the next one; remaining_steps[b] =
    budgets[b] + 9 - 1 (zn_gen_set_rows).  The loop is `Zonos._decode_loop`'s, shared by the rows: one step counter, the stop checks of a
    call of `cadence_B` utterances, the stop flag read at once or (`deferred`) at the next check with the roll-back.
    Returns (delayed codes [rows, 9, t_total], the column offset the loop ends at, loop steps run)."""
    rows = len(budgets)
    Ps = [p.shape[1] for p in prefixes]
    P, max_new = max(Ps), max(budgets)
    codes = torch.full((rows, NQ, P + max_new), -1, dtype=torch.int64)
    for b in range(rows):
        codes[b, :, :Ps[b]] = torch.from_numpy(np.asarray(prefixes[b], dtype=np.int64))
        codes[b, :, Ps[b] + budgets[b]:] = MASK
    delayed = apply_delay_pattern(codes, MASK)
    t_total = delayed.shape[2]
    offset = P + 1
    shift = [p - P for p in Ps]
    tok = lambda call: torch.from_numpy(tokens[call]).long() if call < len(tokens) else torch.zeros(rows, NQ, dtype=torch.long)
    first = tok(0)
    for b in range(rows):                                  # zn_sample_first: column offset0 + shift[b]
        col = delayed[b, :, offset + shift[b]]
        col.copy_(torch.where(col == -1, first[b], col))
    remaining = [b + NQ - 1 for b in budgets]
    stopping = [False] * rows
    cb = torch.arange(NQ)
    steps = 0

    def device_step(step):
        o = P + 1 + step                                   # GenState.offset before the step
        t = tok(step + 1)
        for b in range(rows):
            nxt = t[b]
            if int(nxt[0]) == EOS:
                remaining[b], stopping[b] = min(remaining[b], NQ), True
            if stopping[b]:
                eos_idx = min(NQ - remaining[b], NQ - 1)
                nxt = torch.where(cb < eos_idx, MASK, torch.where(cb == eos_idx, EOS, nxt))
            col = o + 1 + shift[b]
            if 0 <= col < t_total:
                c = delayed[b, :, col]
                c.copy_(torch.where(c == -1, nxt, c))
            remaining[b] -= 1
        return all(r <= 0 for r in remaining)              # GenState.all_done

    max_steps = t_total - offset
    all_done, begun_at, flag_at_begin = False, None, False
    for step_idx in range(max_steps):
        offset += 1
        if offset >= t_total:
            break
        all_done = device_step(step_idx)
        steps += 1
        check = stop_check_at(step_idx, cadence_B)
        if check and deferred:
            if begun_at is not None and flag_at_begin:
                offset, begun_at = begun_at, None
                break
            flag_at_begin, begun_at = all_done, offset
        elif check:
            if all_done:
                break
    if begun_at is not None and flag_at_begin:
        offset = begun_at
    return delayed, offset, steps


def finalise_row(delayed, b, P_b, budget, B):
    """`GenCall.finalise` (`rows.finalise_row`) for row b: its own P_b + budget + 9 columns, cut at row_end_offset(P_b + 1, ...)."""
    offset0, t_b = P_b + 1, P_b + budget + NQ
    row = delayed[b:b + 1, :, :t_b]
    hit = (row[0, 0, offset0 + 1:] == EOS).nonzero()
    eos_column = offset0 + 1 + int(hit[0, 0]) if len(hit) else None
    end = row_end_offset(offset0, t_b, B, NQ, eos_column)
    return finalise_codes(revert_delay_pattern(row), end, NQ, EOS), end


def check_batch(tokens, budgets, prefixes, watch=None):
    """Every row of the mixed-prefix call equals the row generated alone with its own prefix and budget under the same cadence, with the
    immediate and the deferred stop check on either side; the call runs max(budgets) + 9 - 1 loop steps at most, whatever the prefixes.
    `watch`: the rows to compare (default: all)."""
    B = len(budgets)
    for deferred in (False, True):
        delayed, call_end, steps = run_call(tokens, budgets, prefixes, B, deferred)
        assert steps <= max(budgets) + NQ - 1
        assert delayed.shape[2] == max(p.shape[1] for p in prefixes) + max(budgets) + NQ
        for b in (range(B) if watch is None else watch):
            P_b = prefixes[b].shape[1]
            got, end_b = finalise_row(delayed, b, P_b, budgets[b], B)
            assert got.shape[2] <= P_b + budgets[b]
            for solo_deferred in (False, True):
                solo, solo_end, _ = run_call(tokens[:, b:b + 1], [budgets[b]], [prefixes[b]], B, solo_deferred)
                assert end_b == solo_end, (b, budgets, deferred, solo_deferred, end_b, solo_end)
                want = finalise_codes(revert_delay_pattern(solo), solo_end, NQ, EOS)
                assert torch.equal(got, want), (b, budgets, [p.shape[1] for p in prefixes], deferred, solo_deferred)
            # a row's cells left of its own column 0 do not exist, and nothing is written right of its own columns
            assert bool((delayed[b, :, P_b + budgets[b] + NQ:] == MASK).all())


def script(rng, calls, rows, eos_steps):
    """Random raw tokens [calls, rows, 9]; row b samples codebook-0 EOS at loop step eos_steps[b] (None: never)."""
    t = rng.integers(0, 1024, size=(calls, rows, NQ)).astype(np.int64)
    for b, s in enumerate(eos_steps):
        if s is not None and s + 1 < calls:
            t[s + 1, b, 0] = EOS
    return t


def _prefixes(rng, Ps):
    return [rng.integers(0, 1024, size=(NQ, p)).astype(np.int64) for p in Ps]


@pytest.mark.parametrize("seed", range(24))
def test_mixed_prefix_rows_equal_their_solo_calls_on_random_trajectories(seed):
    rng = np.random.default_rng(1000 + seed)
    B = (2, 3, 8)[seed % 3]
    budgets = [int(v) for v in rng.integers(1, 41, size=B)]
    Ps = [int(v) for v in rng.integers(0, 13, size=B)]
    Ps[int(rng.integers(0, B))] = 0
    Ps[(Ps.index(0) + 1) % B] = 12
    calls = max(budgets) + NQ + 2
    eos_steps = [int(rng.integers(0, calls - 1)) if rng.random() < 0.75 else None for _ in range(B)]
    check_batch(script(rng, calls, B, eos_steps), budgets, _prefixes(rng, Ps))


@pytest.mark.parametrize("B", [2, 3, 8])
def test_mixed_prefix_rows_at_the_edges(B):
    """EOS at loop step 0, and in each of the last 9 steps of a row's budget (and the step after it), for the shortest and the longest
    prefix of the call, in the first and the last slot, beside rows that run on."""
    rng = np.random.default_rng(2000 + B)
    for P_slot, P_other in ((0, 12), (12, 0), (5, 12)):
        for budget in (1, 4, 12, 40):
            for eos_step in sorted({0, *range(max(0, budget - NQ), budget + 1)}):
                for slot in sorted({0, B - 1}):
                    budgets = [int(v) for v in rng.integers(1, 41, size=B)]
                    budgets[slot] = budget
                    Ps = [P_other if b % 2 == 0 else int(rng.integers(0, 13)) for b in range(B)]
                    Ps[slot] = P_slot
                    Ps[(slot + 1) % B] = P_other
                    eos_steps = [None] * B
                    eos_steps[slot] = eos_step
                    eos_steps[(slot + 1) % B] = 20
                    check_batch(script(rng, max(budgets) + NQ + 2, B, eos_steps), budgets, _prefixes(rng, Ps), watch=sorted({slot, (slot + 1) % B}))


def test_golden_eos_trajectories_with_prefixes_attached(golden_dir):
    """The golden EOS trajectories (tests/golden/tiny_eos.npz) as rows of mixed-prefix calls.  Alone, under a one-utterance cadence, the
    transcription reproduces the golden codes (with and without the golden prefix); as batch-mates with prefixes of 0 .. 12 frames
    attached, every row equals its solo call."""
    g = np.load(f"{golden_dir}/tiny_eos.npz")
    max_new, p_max_new = int(g["max_new"]), int(g["p_max_new"])
    pre = synth.randint(int(g["seed"]), "prefix", (1, 9, int(g["prefix_len"])), 1024).astype(np.int64)
    keys = sorted((k for k in g.files if k.startswith("out_")), key=lambda k: int(k[4:]))
    none = np.zeros((NQ, 0), dtype=np.int64)
    for k in keys:
        tokens = g[f"tokens_{k[4:]}"].astype(np.int64)
        for deferred in (False, True):
            delayed, end, _ = run_call(tokens, [max_new], [none], 1, deferred)
            got, end_b = finalise_row(delayed, 0, 0, max_new, 1)
            assert end == end_b and np.array_equal(got.numpy(), g[k].astype(np.int64)), (k, deferred)
    pkeys = [k for k in g.files if k.startswith("pout_")]
    for k in pkeys:
        tokens = g[f"ptokens_{k[5:]}"].astype(np.int64)
        delayed, end, _ = run_call(tokens, [p_max_new], [pre[0]], 1, True)
        got, end_b = finalise_row(delayed, 0, pre.shape[2], p_max_new, 1)
        assert end == end_b and np.array_equal(got.numpy(), g[k].astype(np.int64)), k
    rng = np.random.default_rng(0)
    calls = max(max_new, p_max_new) + NQ + 2
    for B in (2, 3, 8):
        for rep in range(4):
            pick = rng.choice(len(keys), size=B, replace=len(keys) < B)
            tokens = rng.integers(0, 1024, size=(calls, B, NQ)).astype(np.int64)
            for b, i in enumerate(pick):
                t = g[f"tokens_{keys[i][4:]}"].astype(np.int64)
                tokens[:len(t), b] = t[:, 0]
            budgets = [int(v) for v in rng.integers(4, max_new + 1, size=B)]
            budgets[int(rng.integers(0, B))] = max_new
            Ps = [int(v) for v in rng.integers(0, 13, size=B)]
            Ps[0], Ps[B - 1] = (0, 12) if rep % 2 == 0 else (12, 0)
            prefixes = _prefixes(rng, Ps)
            if pkeys and rep == 3:                          # a golden prefixed trajectory, with its own prefix, among the rows
                t = g[f"ptokens_{pkeys[0][5:]}"].astype(np.int64)
                tokens[:len(t), 0] = t[:, 0]
                prefixes[0], budgets[0] = pre[0], min(p_max_new, 40)
            check_batch(tokens, budgets, prefixes)


# ---------------------------------------------------------------------------------------------------- ABI
def test_header_declares_and_binding_binds_the_new_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zonos_hip.h")).read(), flags=re.S)
    m = re.search(r"int\s+zn_gen_set_prefix_rows\s*\(\s*zn_handle\s+h\s*,\s*const\s+int32_t\s*\*\s*prefix_len_host\s*,\s*int32_t\s+n\s*\)\s*;", src)
    assert m, "include/zonos_hip.h must declare int zn_gen_set_prefix_rows(zn_handle h, const int32_t* prefix_len_host, int32_t n)"
    assert re.search(r"int\s+zn_op_assemble_prefill\s*\(", src)
    for name in ("zn_gen_set_prefix_rows", "zn_op_assemble_prefill"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["zn_gen_set_prefix_rows"][1]) == 3 and len(_lib.SIGNATURES["zn_op_assemble_prefill"][1]) == 13
    assert int(re.search(r"#define\s+ZN_ABI_VERSION\s+(\d+)", src).group(1)) == _lib.ZN_ABI_VERSION
    # zn_row_params stays as it is: the prefix lengths have their own call and their own device array
    assert _lib.ZN_ROW_PARAMS_BYTES == 64 and [f[0] for f in _lib.zn_row_params._fields_] == ["sp", "cfg_scale", "max_new_tokens", "reserved"]


def test_new_entry_points_report_bad_arguments():
    from zonos_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.zn_abi_version() == _lib.ZN_ABI_VERSION
    lens = (_lib.C.c_int32 * 2)(0, 3)
    assert lib.zn_gen_set_prefix_rows(None, lens, 2) == -1
    assert lib.zn_op_assemble_prefill(None, None, 8, None, None, 10, None, 2, 4, None, 9, None, None) == -1
