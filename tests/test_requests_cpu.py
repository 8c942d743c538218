"""Per-utterance requests in one batch (Zonos.generate_batch, zn_gen_set_rows) - the parts that need no GPU.

* `row_end_offset`, the column at which a request is finalised, against a straight transcription of the decode loop: the device's frame
  bookkeeping (frame_update_body) on scripted token streams under `_decode_loop`'s stop-check cadence, with the immediate and the
  deferred read-back of the stop flag.
* What generate_batch refuses before any launch.
* zn_row_params: one layout in include/zonos_hip.h and in zonos_amd/_lib.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from zonos_amd import _lib, synth
from zonos_amd.codebook_pattern import apply_delay_pattern, revert_delay_pattern
from zonos_amd.model import MAX_BATCH_REQUESTS, GenRequest, check_requests, finalise_codes, row_end_offset
from zonos_amd.parallel import generate_sharded_requests, request_groups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ, EOS, MASK = 9, 1024, 1025


# ---------------------------------------------------------------------------------------------------- the loop, transcribed
def run_call(tokens: np.ndarray, budgets, cadence_B: int, deferred: bool, prefix: np.ndarray | None = None):
    """One generation of len(budgets) rows on scripted raw tokens [calls, rows, 9] (call 0 = the first frame): zn_sample_first's plain
    write, then `Zonos._decode_loop` with the stop checks of a call of `cadence_B` utterances; every loop step runs the device's
    bookkeeping (zn_decode_kernels.h frame_update_body) per row with remaining_steps[b] = budgets[b] + 9 - 1 (zn_gen_set_rows).
    `deferred`: the stop flag of a check is read at the next check and rolls the offset back (generate() without callback or trace);
    otherwise it is read at once.  Returns (delayed codes [rows, 9, t_total], the column offset the loop ends at, loop steps run)."""
    rows = len(budgets)
    P = 0 if prefix is None else prefix.shape[2]
    max_new = max(budgets)
    codes = torch.full((rows, NQ, P + max_new), -1, dtype=torch.int64)
    if prefix is not None:
        codes[..., :P] = torch.from_numpy(prefix)
    for b in range(rows):
        codes[b, :, P + budgets[b]:] = MASK              # generate_batch: a row's cells beyond its own budget are never written
    delayed = apply_delay_pattern(codes, MASK)
    t_total = delayed.shape[2]
    offset = P + 1
    tok = lambda call: torch.from_numpy(tokens[call]).long() if call < len(tokens) else torch.zeros(rows, NQ, dtype=torch.long)
    col = delayed[:, :, offset]
    col.copy_(torch.where(col == -1, tok(0), col))
    remaining = [b + NQ - 1 for b in budgets]
    stopping = [False] * rows
    cb = torch.arange(NQ)
    steps = 0

    def device_step(step):
        o = P + 1 + step                                   # GenState.offset before the step; it writes column o + 1
        t = tok(step + 1)
        for b in range(rows):
            nxt = t[b]
            if int(nxt[0]) == EOS:
                remaining[b], stopping[b] = min(remaining[b], NQ), True
            if stopping[b]:
                eos_idx = min(NQ - remaining[b], NQ - 1)
                nxt = torch.where(cb < eos_idx, MASK, torch.where(cb == eos_idx, EOS, nxt))
            if o + 1 < t_total:
                c = delayed[b, :, o + 1]
                c.copy_(torch.where(c == -1, nxt, c))
            remaining[b] -= 1
        return all(r <= 0 for r in remaining)              # GenState.all_done

    max_steps = t_total - offset
    all_done, begun_at, flag_at_begin = False, None, False
    cpu_step_counter = 0
    for step_idx in range(max_steps):
        offset += 1
        cpu_step_counter += 1
        if offset >= t_total:
            break
        all_done = device_step(step_idx)
        steps += 1
        check = (step_idx % 16 == 15) or (step_idx % 8 == 7 and max(0, cadence_B * 10 - cpu_step_counter) < 5)
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


def eos_column(delayed_row: torch.Tensor, offset0: int):
    hit = (delayed_row[0, offset0 + 1:] == EOS).nonzero()
    return offset0 + 1 + int(hit[0, 0]) if len(hit) else None


def check_batch(tokens, budgets, prefix=None, watch=None):
    """Every row of the batched call, cut to its own columns and finalised at row_end_offset, equals the row generated alone (one row,
    its own budget) under the same cadence - with the immediate and with the deferred stop check on either side.  `watch`: the rows
    to compare (default: all)"""
    B = len(budgets)
    P = 0 if prefix is None else prefix.shape[2]
    offset0 = P + 1
    ends = []
    for deferred in (False, True):
        delayed, call_end, steps = run_call(tokens, budgets, B, deferred, prefix)
        row_ends = []
        for b in (range(B) if watch is None else watch):
            t_b = P + budgets[b] + NQ
            row = delayed[b:b + 1, :, :t_b]
            end_b = row_end_offset(offset0, t_b, B, NQ, eos_column(row[0], offset0))
            for solo_deferred in (False, True):
                solo, solo_end, _ = run_call(tokens[:, b:b + 1], [budgets[b]], B, solo_deferred, None if prefix is None else prefix[b:b + 1])
                assert end_b == solo_end, (b, budgets, deferred, solo_deferred, end_b, solo_end)
                want = finalise_codes(revert_delay_pattern(solo), solo_end, NQ, EOS)
                got = finalise_codes(revert_delay_pattern(row), end_b, NQ, EOS)
                assert torch.equal(got, want), (b, budgets, deferred, solo_deferred)
            row_ends.append(end_b)
        # the call itself ends no earlier than any row that stopped at a check, and with immediate checks runs exactly to its end column
        if watch is None:
            assert call_end >= max(e for e, bud in zip(row_ends, budgets) if bud == max(budgets))
        if not deferred:
            assert steps == call_end - offset0 or call_end == delayed.shape[2]
        ends.append((call_end, tuple(row_ends)))
    assert ends[0] == ends[1]                              # the deferred read-back changes when the loop learns of the stop, not where it ends
    return ends[0]


def script(rng, calls, rows, eos_steps):
    """Random raw tokens [calls, rows, 9]; row b samples codebook-0 EOS at loop step eos_steps[b] (None: never)."""
    t = rng.integers(0, 1024, size=(calls, rows, NQ)).astype(np.int64)
    for b, s in enumerate(eos_steps):
        if s is not None:
            t[s + 1, b, 0] = EOS
    return t


def test_row_end_offset_on_the_golden_eos_trajectories(golden_dir):
    """B = 1: the rule is the reference's own loop end (the replay reproduces the golden codes).  B = 3 and 8: golden trajectories as
    batch-mates with budgets of their own."""
    g = np.load(f"{golden_dir}/tiny_eos.npz")
    max_new, p_max_new = int(g["max_new"]), int(g["p_max_new"])
    pre = synth.randint(int(g["seed"]), "prefix", (1, 9, int(g["prefix_len"])), 1024)
    keys = sorted((k for k in g.files if k.startswith("out_")), key=lambda k: int(k[4:]))
    for k in keys:
        tokens = g[f"tokens_{k[4:]}"].astype(np.int64)
        for deferred in (False, True):
            delayed, end, _ = run_call(tokens, [max_new], 1, deferred)
            assert end == row_end_offset(1, delayed.shape[2], 1, NQ, eos_column(delayed[0], 1)), (k, deferred)
            assert np.array_equal(finalise_codes(revert_delay_pattern(delayed), end, NQ, EOS).numpy(), g[k].astype(np.int64)), (k, deferred)
    for k in (k for k in g.files if k.startswith("pout_")):
        tokens = g[f"ptokens_{k[5:]}"].astype(np.int64)
        delayed, end, _ = run_call(tokens, [p_max_new], 1, True, pre)
        P = pre.shape[2]
        assert end == row_end_offset(P + 1, delayed.shape[2], 1, NQ, eos_column(delayed[0], P + 1)), k
        assert np.array_equal(finalise_codes(revert_delay_pattern(delayed), end, NQ, EOS).numpy(), g[k].astype(np.int64)), k
    rng = np.random.default_rng(0)
    calls = max_new + NQ + 2
    for B in (3, 8):
        for rep in range(4):
            pick = rng.choice(len(keys), size=B, replace=False)
            tokens = rng.integers(0, 1024, size=(calls, B, NQ)).astype(np.int64)
            for b, i in enumerate(pick):
                t = g[f"tokens_{keys[i][4:]}"].astype(np.int64)
                tokens[:len(t), b] = t[:, 0]
            budgets = [int(v) for v in rng.integers(4, max_new + 1, size=B)]
            budgets[int(rng.integers(0, B))] = max_new
            check_batch(tokens, budgets)


@pytest.mark.parametrize("B", [1, 3, 8])
def test_row_end_offset_edge_cases(B):
    """An EOS in the first 8 steps, an EOS whose ninth column lands exactly on a check step, one step before and one after it, and a
    budget that ends before the EOS - in every slot of a batch whose other rows run on."""
    rng = np.random.default_rng(100 + B)
    checks = [s for s in range(80) if (s % 16 == 15) or (s % 8 == 7 and max(0, B * 10 - (s + 1)) < 5)]
    assert (7 in checks) == (B == 1) and 15 in checks
    seen = set()
    big = 44
    for chk in checks[:3 if B == 1 else 2]:
        for eos_step in (0, 3, 7, chk - NQ, chk - NQ + 1, chk - NQ + 2, chk):
            if eos_step < 0:
                continue
            for budget in (max(1, eos_step - 12), max(1, eos_step - 3), eos_step + 1, eos_step + 2, eos_step + NQ, big):   # the first three: spent before the EOS
                for slot in sorted({0, B - 1}):
                    budgets = [big] * B
                    budgets[slot] = budget
                    eos_steps = [None] * B
                    eos_steps[slot] = eos_step
                    if B > 1:
                        eos_steps[(slot + 1) % B] = 20
                    tokens = script(rng, big + NQ + 2, B, eos_steps)
                    call_end, row_ends = check_batch(tokens, budgets, watch=[slot])
                    t_b = budget + NQ
                    # stopped rows end on a check step (offset0 = 1: column = step + 1), budget-limited ones at their t_total
                    assert row_ends[0] == t_b or (row_ends[0] - 2) in checks
                    seen.add("budget" if row_ends[0] == t_b else "check")
                    # the row is done from step eos_step + 9 on (remaining_steps capped at 9, one off per step) ...
                    done_at = min(eos_step + NQ - 1, budget + NQ - 2)
                    first = next(c for c in checks if c >= done_at)
                    assert row_ends[0] == min(first + 2, t_b), (chk, eos_step, budget, slot)
    assert seen == {"budget", "check"}


@pytest.mark.parametrize("seed", range(24))
def test_row_end_offset_on_random_trajectories(seed):
    rng = np.random.default_rng(seed)
    B = (1, 3, 8)[seed % 3]
    budgets = [int(v) for v in rng.integers(1, 70, size=B)]
    calls = max(budgets) + NQ + 2
    eos_steps = [int(rng.integers(0, calls - 1)) if rng.random() < 0.75 else None for _ in range(B)]
    prefix = rng.integers(0, 1024, size=(B, NQ, int(rng.integers(1, 9)))) if seed % 4 == 3 else None
    check_batch(script(rng, calls, B, eos_steps), budgets, prefix)


# ---------------------------------------------------------------------------------------------------- request validation
def _req(cseed, L=6, halves=2, **kw):
    return GenRequest(synth.conditioning(cseed, "req.cond", halves, L, synth.TINY_CFG["d_model"]), **kw)


def test_generate_batch_refuses_before_any_launch():
    from zonos_amd.testing import build_model
    model, _ = build_model(synth.TINY_CFG, 77, "cpu")
    pre = lambda P: torch.from_numpy(synth.randint(3, "req.prefix", (1, 9, P), 1024))
    with pytest.raises(ValueError, match="no requests"):
        model.generate_batch([])
    with pytest.raises(ValueError, match="cfg_scale == 1"):
        model.generate_batch([_req(1), _req(2, halves=1, cfg_scale=1.0)])
    with pytest.raises(ValueError, match="audio prefixes of different lengths"):
        model.generate_batch([_req(1, audio_prefix_codes=pre(3)), _req(2, audio_prefix_codes=pre(5))])
    with pytest.raises(ValueError, match="audio prefixes of different lengths"):
        model.generate_batch([_req(1, audio_prefix_codes=pre(3)), _req(2)])
    with pytest.raises(ValueError, match=f"at most {MAX_BATCH_REQUESTS}"):
        model.generate_batch([_req(1)] * (MAX_BATCH_REQUESTS + 1))
    with pytest.raises(ValueError, match="conditioning of shape"):
        model.generate_batch([_req(1), _req(2, halves=1)])                       # a guided request needs [cond ‖ uncond]
    with pytest.raises(ValueError, match="max_new_tokens"):
        model.generate_batch([_req(1), _req(2, max_new_tokens=0)])
    with pytest.raises(TypeError, match="unexpected keyword"):
        model.generate_batch([_req(1), _req(2, sampling_params=dict(temprature=1.0))])
    # requests that pass go on to the device check (no GPU here): different lengths, parameters, seeds, cfg_scale and budgets are fine
    good = [_req(1, L=5, cfg_scale=1.5, max_new_tokens=6, seed=3, sampling_params=dict(temperature=0.8)),
            _req(2, L=9, cfg_scale=3.0, max_new_tokens=14, sampling_params=dict(temperature=0.0, repetition_penalty=5.0))]
    assert check_requests(good, NQ, synth.TINY_CFG["d_model"]) == (True, 0)
    with pytest.raises(_lib.ZonosHipError, match="MI355X only"):
        model.generate_batch(good)
    with pytest.raises(_lib.ZonosHipError, match="MI355X only"):
        model.generate_batch(good[:1])                                            # one request is generate() with its arguments
    assert GenRequest(good[0].conditioning).sampling_params == dict(min_p=0.1) and GenRequest(good[0].conditioning).max_new_tokens == 86 * 30


def test_sharded_requests_keep_request_order_and_group_what_may_share_a_call():
    """parallel.generate_sharded_requests on one rank: groups hold only requests that may share a call, results come back in request order."""
    pre = torch.zeros(1, 9, 2, dtype=torch.long)
    reqs = [_req(i, L=4 + i % 3, halves=1 if i % 4 == 1 else 2, cfg_scale=1.0 if i % 4 == 1 else 2.0, max_new_tokens=3 + i,
                 audio_prefix_codes=pre if i % 5 == 2 else None) for i in range(11)]
    groups = request_groups(reqs, list(range(11)), 3)
    assert sorted(i for grp in groups for i in grp) == list(range(11)) and max(len(grp) for grp in groups) == 3
    for grp in groups:
        check_requests([reqs[i] for i in grp], NQ, synth.TINY_CFG["d_model"])
    calls = []

    def fake(batch):
        calls.append(len(batch))
        return [torch.full((1, 9, r.max_new_tokens), r.max_new_tokens, dtype=torch.int64) for r in batch]
    out = generate_sharded_requests(fake, reqs, batch_size=3)
    assert [tuple(o.shape) for o in out] == [(9, 3 + i) for i in range(11)] and all(int(o[0, 0]) == 3 + i for i, o in enumerate(out))
    assert calls == [len(grp) for grp in groups]


# ---------------------------------------------------------------------------------------------------- ABI
_CTYPES = {"float": (4, C.c_float), "int32_t": (4, C.c_int32), "uint64_t": (8, C.c_uint64)}


def _header_struct(name, src, known):
    """(fields [(name, offset, size)], size, alignment) of `typedef struct name { ... } name;` under the C layout rules."""
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), src, flags=re.S).group(1)
    fields, off, align = [], 0, 1
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, rest = decl.split(None, 1)
        for item in (i.strip() for i in rest.split(",")):
            m = re.fullmatch(r"(?:(float|int32_t|uint64_t)\s+)?(\w+)(?:\[(\d+)\])?", item)      # `float top_p; int32_t top_k` on one line
            assert m, (name, decl)
            ctype = m.group(1) or ctype
            size, al = known[ctype][:2] if ctype in known else (_CTYPES[ctype][0], _CTYPES[ctype][0])
            count = int(m.group(3) or 1)
            off = (off + al - 1) // al * al
            fields.append((m.group(2), off, size * count))
            off += size * count
            align = max(align, al)
    return fields, (off + align - 1) // align * align, align


def test_row_params_layout_agrees_between_header_and_binding():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zonos_hip.h")).read(), flags=re.S)
    src = re.sub(r";\s*(float|int32_t|uint64_t)\s", r"; \1 ", src)
    # (a declaration list like `float top_p; int32_t top_k; float min_p;` on one line is split at the semicolons)
    sp_fields, sp_size, sp_align = _header_struct("zn_sampling", src, {})
    rp_fields, rp_size, _ = _header_struct("zn_row_params", src, {"zn_sampling": (sp_size, sp_align)})
    stated = int(re.search(r"#define\s+ZN_ROW_PARAMS_BYTES\s+(\d+)", src).group(1))
    assert rp_size == stated == 64 == C.sizeof(_lib.zn_row_params) == _lib.ZN_ROW_PARAMS_BYTES
    assert sp_size == C.sizeof(_lib.zn_sampling) == 48
    for cls, fields in ((_lib.zn_sampling, sp_fields), (_lib.zn_row_params, rp_fields)):
        assert [f[0] for f in cls._fields_] == [f[0] for f in fields]
        for fname, off, size in fields:
            d = getattr(cls, fname)
            assert (d.offset, d.size) == (off, size), (cls.__name__, fname, d.offset, d.size, off, size)
    assert [f[0] for f in rp_fields] == ["sp", "cfg_scale", "max_new_tokens", "reserved"]
    assert int(re.search(r"#define\s+ZN_ABI_VERSION\s+(\d+)", src).group(1)) == _lib.ZN_ABI_VERSION == 9


def test_new_entry_points_report_bad_arguments():
    from zonos_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    rows = (_lib.zn_row_params * 2)()
    assert lib.zn_gen_set_rows(None, rows, 2) == -1
    assert lib.zn_op_sample_rows(None, None, None, 0, None, 0, None, None, 2, None) == -1
