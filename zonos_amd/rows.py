"""The host's row layout, as pure functions: what a request is, its `zn_row_params` entry and seed, its delayed row of the
code buffer, the column its own loop ends at and its final codes - and `GenCall`, the record of what one zn_gen_begin .. zn_gen_end runs
on, with one constructor per kind of call.

torch on any device and the ctypes structs of `_lib`; no engine and no library call, so everything here runs on a CPU.
"""
from __future__ import annotations

from collections import namedtuple
from dataclasses import dataclass, field
from typing import Sequence

import torch

from . import _lib
from .codebook_pattern import apply_delay_pattern, revert_delay_pattern
from .conditioning import pad_conditioning_rows, pad_conditionings

SAMPLING_DEFAULTS = dict(temperature=1.0, top_p=0.0, top_k=0, min_p=0.0, linear=0.0, conf=0.0, quad=0.0,
                         repetition_penalty=3.0, repetition_penalty_window=2)   # zonos/sampling.py:166-178


def sampling_struct(params: dict, seed: int) -> _lib.zn_sampling:
    unknown = set(params) - set(SAMPLING_DEFAULTS)
    if unknown:
        raise TypeError(f"sample_from_logits() got unexpected keyword arguments {sorted(unknown)}")
    p = {**SAMPLING_DEFAULTS, **params}
    return _lib.zn_sampling(temperature=p["temperature"], top_p=p["top_p"], top_k=int(p["top_k"]), min_p=p["min_p"],
                            linear=p["linear"], conf=p["conf"], quad=p["quad"], repetition_penalty=p["repetition_penalty"],
                            repetition_penalty_window=int(p["repetition_penalty_window"]), seed=seed & (2 ** 64 - 1))


@dataclass
class GenRequest:
    """One utterance of `Zonos.generate_batch`: `generate()`'s per-call arguments, per request.  `conditioning` is what
    `prepare_conditioning` returns for the utterance: [2, L, d] = [cond ‖ uncond], or [1, L, d] when cfg_scale == 1."""
    conditioning: torch.Tensor
    sampling_params: dict = field(default_factory=lambda: dict(min_p=0.1))
    seed: int | None = None
    cfg_scale: float = 2.0
    max_new_tokens: int = 86 * 30
    audio_prefix_codes: torch.Tensor | None = None


def check_request_shapes(where: str, cond_shape: Sequence[int], halves: int, d_model: int, cfg_scale: float, max_new_tokens,
                         prefix_shape: Sequence[int] | None, nq: int) -> tuple[int, int]:
    """The shape checks every request passes, in a call or a session (ValueError; `where` opens the message: "generate_batch: request i: "
    or "serve: "): the conditioning [halves, L >= 1, d_model], a positive integer max_new_tokens, the audio prefix None or [1, nq, P].
    Returns (L, P)."""
    c = tuple(cond_shape)
    if len(c) != 3 or c[0] != halves or c[1] < 1 or c[2] != d_model:
        raise ValueError(f"{where}conditioning of shape {c}, expected [{halves}, L >= 1, {d_model}] at cfg_scale={cfg_scale}")
    if int(max_new_tokens) != max_new_tokens or int(max_new_tokens) < 1:
        raise ValueError(f"{where}max_new_tokens must be a positive integer, got {max_new_tokens}")
    a = None if prefix_shape is None else tuple(prefix_shape)
    if a is not None and (len(a) != 3 or a[0] != 1 or a[1] != nq):
        raise ValueError(f"{where}audio_prefix_codes of shape {a}, expected [1, {nq}, P]")
    return int(c[1]), 0 if a is None else int(a[2])


# ---------------------------------------------------------------------------------------------- seeds and zn_row_params
def draw_seed(seed: int | None) -> int:
    """A request's seed: its own, or one draw from torch's global generator."""
    return int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else seed


def row_entry(request, seed: int, pair: tuple[int, int] | None = None) -> _lib.zn_row_params:
    """The entry of one row that runs `request` with the random stream of `seed`.  `pair` = (cond_row, uncond_row) of a guided request in
    the unguided layout (a mixed call or session): both of its rows carry the same entry, which names the pair."""
    e = _lib.zn_row_params(sp=sampling_struct(request.sampling_params, seed), cfg_scale=float(request.cfg_scale),
                           max_new_tokens=int(request.max_new_tokens))
    if pair is not None:
        e.reserved[0], e.reserved[1] = pair[0] + 1, pair[1] + 1
    return e


def row_table(requests: Sequence, first: Sequence[int] | None = None):
    """The zn_row_params table of a call (zn_gen_set_rows).  Without `first`: one entry per request (the guided and the unguided layout).
    With `first`, the first row of each request as `pad_conditioning_rows` returns it: one entry per row of a mixed call, a guided
    request's two adjacent rows with equal entries that name the pair.  One seed per request, drawn in request order."""
    entries = []
    for i, r in enumerate(requests):
        n = 1 if first is None else int(r.conditioning.shape[0])
        entries += [row_entry(r, draw_seed(r.seed), (first[i], first[i] + 1) if n == 2 else None)] * n
    return (_lib.zn_row_params * len(entries))(*entries)


# ---------------------------------------------------------------------------------------------- the code buffer
def code_rows(prefixes: Sequence, budgets: Sequence[int], width: int, nq: int, mask_id: int, device) -> torch.Tensor:
    """The delayed rows int32 [n, nq, width] of a code buffer.  Row b is left-aligned: its P_b prefix frames (`prefixes[b]`: None, or
    [1, nq, P_b]), `budgets[b]` unknown cells (-1), then the mask token up to width - nq - as the delay pattern of a generation of that
    length leaves them: they are never written, and the steps that run past the row's end embed what its own generation would have
    embedded.  The first P_b + budgets[b] + nq columns of a row therefore do not depend on the width or on the other rows."""
    codes = torch.full((len(budgets), nq, width - nq), mask_id, dtype=torch.int32, device=device)
    for b, (a, n) in enumerate(zip(prefixes, budgets)):
        P = 0 if a is None else int(a.shape[2])
        if P:
            codes[b, :, :P] = a[0].to(device=device, dtype=torch.int32)
        codes[b, :, P:P + int(n)] = -1
    return apply_delay_pattern(codes, mask_id).contiguous()


# ---------------------------------------------------------------------------------------------- when a row ends, and its final codes
def stop_check_at(step_idx: int, batch_size: int) -> bool:
    """The reference's stop-check cadence (tensor_ops.py:90-103) as `_loop_after_prefill` runs it: is the stop flag read after loop step
    `step_idx` (0-based) of a call of `batch_size` utterances?"""
    return step_idx % 16 == 15 or (step_idx % 8 == 7 and max(0, batch_size * 10 - (step_idx + 1)) < 5)


def row_end_offset(offset0: int, t_total: int, batch_size: int, nq: int, eos_column: int | None) -> int:
    """The column at which the decode loop of a call of `batch_size` utterances would have ended had it watched one row alone
    (`generate_batch`: every request is cut and finalised for itself, while the call runs on to its last row).  The row starts at column
    `offset0` (audio prefix + 1) with its own `t_total` = prefix + max_new_tokens + nq columns and remaining_steps = t_total - offset0;
    `eos_column` is the first column beyond offset0 whose codebook 0 holds EOS (None: there is none below t_total).  Loop step i writes
    column offset0 + i + 1; a step that samples EOS in codebook 0 caps remaining_steps at nq; every step takes one off (tensor_ops.py:87,
    155-211).  The loop leaves at the first check of the call's cadence (`stop_check_at`) at which remaining_steps <= 0 - the deferred
    read-back of `_loop_after_prefill` rolls back to that same check - or at t_total when the row's budget ends before any such check."""
    remaining, offset = t_total - offset0, offset0
    for step_idx in range(t_total - offset0):
        offset += 1
        if offset >= t_total:
            break
        if eos_column is not None and offset == eos_column:
            remaining = min(remaining, nq)
        remaining -= 1
        if stop_check_at(step_idx, batch_size) and remaining <= 0:
            return offset
    return t_total


def map_codes(out: torch.Tensor) -> torch.Tensor:
    """model.py:530-539: EOS / mask tokens to codes, clamped to the codebook."""
    out = torch.where(out > 1024, 512, out)
    out = torch.where(out == 1024, 0, out)
    return torch.clamp(out, 0, 1023)


def finalise_codes(out: torch.Tensor, offset: int, nq: int, eos_id: int) -> torch.Tensor:
    """model.py:511-539 on the reverted codes [B, nq, audio_len] of a generation whose loop ended at column `offset`: the EOS boundary
    search over the last min(50, valid_length // 4) frames, then the code mapping.  `generate()` and `stream()` both end here."""
    valid_length = offset - nq
    window = min(50, valid_length // 4)
    for pos in range(max(0, valid_length - window), valid_length):   # model.py:516-528
        if int((out[:, :, pos] == eos_id).sum()) >= nq // 2:
            valid_length = pos
            break
    return map_codes(out[..., :valid_length])


def finalise_row(delayed_row: torch.Tensor, P_b: int, max_new_tokens: int, B: int, nq: int, eos_id: int):
    """One row [1, nq, >= t_b] of a call of B utterances (or of a session of B slots): (its final codes, its first codebook-0 EOS column
    or None, the column its own loop ends at).  The row keeps its own t_b = P_b + max_new_tokens + nq columns and is finalised at the
    column its own loop would have ended at (`row_end_offset`): a row's step index does not depend on its prefix, only its columns do."""
    offset0 = P_b + 1
    t_b = P_b + max_new_tokens + nq
    row = delayed_row[:, :, :t_b].to(torch.int64)
    hit = (row[0, 0, offset0 + 1:] == eos_id).nonzero()
    eos_column = offset0 + 1 + int(hit[0, 0]) if len(hit) else None
    end = row_end_offset(offset0, t_b, B, nq, eos_column)
    return finalise_codes(revert_delay_pattern(row), end, nq, eos_id), eos_column, end


# ---------------------------------------------------------------------------------------------- one generation
@dataclass
class GenCall:
    """What one zn_gen_begin .. zn_gen_end runs on.  B utterances (`len(budgets)`) over the R rows of `cond`: R = 2 B with guidance
    ([cond_0..cond_{B-1}, uncond_0..uncond_{B-1}]), R = B in the unguided layout - which a mixed call uses too, with one utterance per
    cfg_scale == 1 request and two adjacent ones per guided request, paired by `table`."""
    cond: torch.Tensor                         # [R, L_c, d]
    cond_lengths: list[int] | None             # the B valid lengths of a right-padded `cond`; None: every row holds L_c positions
    prefixes: list                             # per utterance, None or [1, nq, P_b]
    prefix_lens: list[int]
    budgets: list[int]                         # per utterance, its max_new_tokens
    max_new_tokens: int                        # the call's: the largest budget
    cfg_scale: float                           # with `table`, only fixes the row layout: every sampler reads its row's entry
    sp: _lib.zn_sampling                       # the call-wide sampling parameters (read where there is no `table`)
    ragged: bool = False                       # prefixes of different lengths: zn_gen_set_prefix_rows, prefill rows assembled by the kernel
    table: object = None                       # zn_row_params per utterance (zn_gen_set_rows), or None
    request_rows: list[int] | None = None      # a mixed call: the row each request's result is read from

    def __post_init__(self):
        # derived: the utterances, the call's audio prefix length (the longest prefix), R (the rows to size the engine by), and the batch
        # size whose stop-check cadence the loop follows (a mixed call has more utterance rows than requests)
        self.B, self.P, self.engine_rows = len(self.budgets), max(self.prefix_lens), self.cond.shape[0]
        self.cadence = self.B if self.request_rows is None else len(self.request_rows)

    @classmethod
    def plain(cls, cond, prefix, max_new_tokens, cfg_scale, B, sampling_params, seed, cond_lengths=None) -> "GenCall":
        """`generate()` and `stream()`: B utterances that share the prefix length, the budget and the sampling parameters."""
        prefixes = [None] * B if prefix is None else [prefix.expand(B, -1, -1)[b:b + 1] for b in range(B)]
        return cls(cond, None if cond_lengths is None else [int(v) for v in cond_lengths], prefixes, [0 if prefix is None else int(prefix.shape[2])] * B, [max_new_tokens] * B,
                   max_new_tokens, cfg_scale, sampling_struct(sampling_params, draw_seed(seed)))

    @classmethod
    def batch(cls, reqs, guided: bool, ragged: bool, device) -> "GenCall":
        """`generate_batch()` of requests of one kind: utterance b is request b."""
        scale = 2.0 if guided else 1.0
        cond, lengths = pad_conditionings([r.conditioning.to(device) for r in reqs], scale)
        return cls._of_rows(reqs, range(len(reqs)), cond, lengths, scale, ragged, row_table(reqs))

    @classmethod
    def mixed(cls, reqs, ragged: bool, device) -> "GenCall":
        """`generate_batch(mixed_guidance=True)` with both kinds of request present: one utterance per conditioning row, in request order;
        a guided request is read from its first row."""
        cond, lengths, first = pad_conditioning_rows([r.conditioning.to(device) for r in reqs])
        owner = [i for i, r in enumerate(reqs) for _ in range(r.conditioning.shape[0])]          # row -> request
        return cls._of_rows(reqs, owner, cond, lengths, 1.0, ragged, row_table(reqs, first), first)

    @classmethod
    def _of_rows(cls, reqs, owner, cond, lengths, cfg_scale, ragged, table, request_rows=None) -> "GenCall":
        prefixes, budgets = [reqs[i].audio_prefix_codes for i in owner], [int(reqs[i].max_new_tokens) for i in owner]
        # zn_gen_begin's own sampling parameters only fix the row layout: every sampler reads the table
        return cls(cond, lengths, prefixes, [0 if a is None else int(a.shape[-1]) for a in prefixes], budgets, max(budgets), cfg_scale, sampling_struct(reqs[0].sampling_params, 0), ragged, table, request_rows)

    def finalise(self, delayed: torch.Tensor, offset: int, nq: int, eos_id: int):
        """The call's result from its delayed codes (one device->host copy) and the column `offset` its loop ended at: jointly for plain
        `generate()` (model.py:511), else one tensor per utterance - or per request, read from its row - each cut for itself."""
        if self.table is None:
            return finalise_codes(revert_delay_pattern(delayed.to(torch.int64)).cpu(), offset, nq, eos_id)
        host = delayed.cpu()
        return [finalise_row(host[u:u + 1], self.prefix_lens[u], self.budgets[u], self.cadence, nq, eos_id)[0]
                for u in (range(self.B) if self.request_rows is None else self.request_rows)]


# What watches a generation: `callback` (generate()), `trace` (the `_trace` dict) and `chunk` (stream(): yield every `chunk` steps).
Hooks = namedtuple("Hooks", "callback trace chunk", defaults=(None, None, None))
