"""The session of `Zonos.serve()` and `Zonos.serve_stream()` on an engine: what `SlotScheduler` and `StreamLedger`
(serving.py) decide, enqueued through the C ABI.  `Zonos._serve_gen` holds the engine and loops over `point()`."""
from __future__ import annotations

import ctypes as C
import time
from collections import namedtuple

import torch

from . import _lib
from .codebook_pattern import revert_delay_pattern
from .conditioning import pad_conditionings
from .rows import GenRequest, code_rows, draw_seed, finalise_row, map_codes, row_entry, sampling_struct
from .serving import ServeChunk, ServeResult, SlotScheduler, StreamLedger, check_serve_request, serve_slack


# What sizes a session once: serve()'s checked arguments (`guided` None: a mixed session, `slots` counts rows).
ServeShape = namedtuple("ServeShape", "slots max_prompt max_new_tokens guided sched_every")


class ServeSession:
    """One session: `open` (zn_gen_begin, zn_gen_open_slots), then `point` per scheduling point - admissions (`accept`, `admit`), the
    steps, the row state, the ledger's scan, retirements and chunks - until it says stop; `close` (zn_gen_end) whatever happened.
    `chunk_frames` None: serve(), results are ServeResult; else serve_stream(), ServeChunk."""

    def __init__(self, model, ts, source, shape: ServeShape, trace=None, stats=None, chunk_frames=None, audio=(None, False)):
        self.model, self.ts, self.source, self.shape, self.trace, self.stats = model, ts, source, shape, trace, stats
        self.dev, self.st = model.device, ts.cuda_stream
        self.nq, self.d, self.mask = model.config.codebook_dimension, model.config.backbone.d_model, model.masked_token_id
        # (a mixed session: rows in the unguided layout; a guided request holds two of them)
        self.slots, self.guided, self.mixed, self.halves = shape.slots, shape.guided, shape.guided is None, 2 if shape.guided else 1
        self.R, self.slack = shape.slots * self.halves, serve_slack(shape.sched_every)
        self.width = shape.max_prompt + shape.max_new_tokens + self.nq + self.slack       # columns of a slot's row of the code buffer
        self.sched = SlotScheduler(shape.slots, self.nq, shape.sched_every)
        self.streaming = chunk_frames is not None
        self.ledger = StreamLedger(self.nq, chunk_frames, model.eos_token_id) if self.streaming else None
        self.dacs = model.autoencoder.stream_set(ts, *audio) if self.streaming else None      # audio: (sample_rate, pcm16)
        self.rem, self.own = (C.c_int32 * shape.slots)(), (C.c_int32 * shape.slots)()
        self.eng, self.begun = None, False

    def open(self, eng) -> None:
        model, shape, self.eng = self.model, self.shape, eng
        with torch.inference_mode(), torch.cuda.device(self.dev), torch.cuda.stream(self.ts):
            self.kv = model._kv_buffers(eng, self.R, self.width)       # (the KV caches - bf16, codes or both - live as long as the session)
            self.ip = ip = self.kv.ip
            self.delayed = torch.full((self.slots, self.nq, self.width), self.mask, dtype=torch.int32, device=self.dev)   # an idle slot's cells are never -1
            sp = sampling_struct({}, 0)                                # (every sampler of a session reads its slot's entry)
            eng.call("zn_gen_begin", self.slots, self.kv.kv_ptrs, ip.max_seqlen, ip.lengths_per_sample.data_ptr(), self.delayed.data_ptr(), self.width, 1,
                     shape.max_new_tokens, 2.0 if self.guided else 1.0, C.byref(sp), self.st)
            self.begun = True
            model._bind_kv_buffers(eng, self.kv)
            eng.call("zn_gen_open_slots", self.slack)

    def close(self) -> None:
        if self.begun:
            self.ts.synchronize()
            self.eng.call("zn_gen_end")

    def accept(self, r):
        """`SlotScheduler.pull`'s judge: (prefix frames, budget, slots needed) of a request, or the ValueError that refuses it."""
        if not isinstance(r, GenRequest):
            raise ValueError(f"serve: expected a GenRequest or None, got {type(r).__name__}")
        c, a = r.conditioning, r.audio_prefix_codes
        if not hasattr(c, "shape") or (a is not None and not hasattr(a, "shape")):
            raise ValueError("serve: conditioning and audio_prefix_codes must be tensors")
        L, P = check_serve_request(c.shape, None if a is None else a.shape, r.max_new_tokens, r.cfg_scale, nq=self.nq, d_model=self.d,
                                   guided=self.guided, max_len=self.ip.max_seqlen, width=self.width, slack=self.slack)
        try:
            sampling_struct(r.sampling_params, 0)
        except TypeError as e:
            raise ValueError(f"serve: {e}") from None
        return P, int(r.max_new_tokens), (2 if self.mixed and float(r.cfg_scale) != 1.0 else 1)

    def record(self, kind, holders) -> None:
        if self.trace is not None:
            self.trace.setdefault("logits", []).append(self.model._step_logits(self.eng, self.slots, self.nq))
            self.trace.setdefault("slots", []).append((kind, self.sched.step, list(holders)))

    def admit(self, admitted) -> None:
        """Prefill the admitted requests into their slots (zn_op_assemble_prefill, zn_gen_admit) while the other rows keep their state."""
        dev, nq, halves, sched, eng = self.dev, self.nq, self.halves, self.sched, self.eng
        # one entry per admitted row: (slot, request, conditioning rows of that slot).  A two-slot request of a mixed session gives
        # two entries, its conditional row into its owner slot and its unconditional one into the partner, both naming the pair.
        entries = []
        for slot, _, r in admitted:
            c, f = r.conditioning.to(dev), sched.partner(slot)
            if f is None:
                entries.append((slot, r, c, None))
            else:
                entries += [(slot, r, c[0:1], (slot, f)), (f, r, c[1:2], (slot, f))]
        n = len(entries)
        Ls = [int(c.shape[1]) for _, _, c, _ in entries]
        Ps = [0 if r.audio_prefix_codes is None else int(r.audio_prefix_codes.shape[2]) for _, r, _, _ in entries]
        cond, _ = pad_conditionings([c for _, _, c, _ in entries], 2.0 if self.guided else 1.0)
        cond = cond.to(device=dev, dtype=torch.bfloat16).contiguous()
        rows = code_rows([r.audio_prefix_codes for _, r, _, _ in entries], [r.max_new_tokens for _, r, _, _ in entries], self.width, nq, self.mask, dev)
        adm = (_lib.zn_admit * n)()
        seeds = {}
        for j, (slot, r, _, pair) in enumerate(entries):
            self.delayed[slot].copy_(rows[j])
            if id(r) not in seeds:                                     # one draw per request, not per row
                seeds[id(r)] = draw_seed(r.seed)
            adm[j].slot, adm[j].row_len, adm[j].prefix_len = slot, Ls[j] + Ps[j] + 1, Ps[j]
            adm[j].params = row_entry(r, seeds[id(r)], pair)
        S = max(L + P + 1 for L, P in zip(Ls, Ps))
        meta = torch.tensor([Ls, Ps], dtype=torch.int32).to(dev)
        hidden = torch.empty(halves * n, S, self.d, dtype=torch.bfloat16, device=dev)
        row_len_dev = torch.empty(halves * n, dtype=torch.int32, device=dev)
        eng.call("zn_op_assemble_prefill", cond.data_ptr(), cond.shape[1], meta[0].data_ptr(), rows.data_ptr(), self.width, meta[1].data_ptr(), n,
                 halves * n, hidden.data_ptr(), S, row_len_dev.data_ptr(), self.st)
        eng.call("zn_gen_admit", adm, n, hidden.data_ptr(), S, self.st)
        held = [None] * self.slots
        for slot, index, _ in admitted:
            held[slot] = index
            if sched.partner(slot) is not None:
                held[sched.partner(slot)] = index
        self.record("admit", held)
        for slot, index, r in admitted:
            if self.streaming:
                self.ledger.open(slot, 0 if r.audio_prefix_codes is None else int(r.audio_prefix_codes.shape[2]), int(r.max_new_tokens))
            if self.stats is not None:
                self.stats.setdefault("admitted_at", {})[index] = time.perf_counter()

    def _steps(self) -> None:
        """`sched_every` decode steps in one call (one by one under `_trace`), the device's row state into `rem` / `own`, and with streaming
        codebook 0 of the columns that decide a slot's EOS frame: one gather, one read-back."""
        eng, sched, st, slots = self.eng, self.sched, self.st, self.slots
        if self.trace is None:
            eng.call("zn_decode_steps", sched.sched_every, st)
            sched.advance()
        else:
            for _ in range(sched.sched_every):
                eng.call("zn_decode_steps", 1, st)
                sched.advance(1)
                self.record("step", sched.holders())
        if self.stats is not None:
            self.stats["steps"] = sched.step
        eng.call("zn_gen_row_state", self.rem, self.own, st)
        if [self.own[b] for b in range(slots)] != [sched.own_steps(b) for b in range(slots)]:
            raise _lib.ZonosHipError(f"serve: the device counts {list(self.own)} steps per slot, the scheduler {[sched.own_steps(b) for b in range(slots)]}")
        cells = self.ledger.cells(self.own) if self.streaming else None
        if cells:
            flat = [b * self.nq * self.width + c for b, lo, hi in cells for c in range(lo, hi)]
            toks = self.delayed.view(-1)[torch.tensor(flat, dtype=torch.int64).to(self.dev)].cpu().tolist()
            for b, lo, hi in cells:
                self.ledger.scan(b, lo, toks[:hi - lo])
                del toks[:hi - lo]

    def _retire(self) -> list:
        """The rows whose own loop has left: finalised, retired on the device; with streaming, also the chunks of the rows that run on."""
        sched, delayed, slots, nq, eos, dev = self.sched, self.delayed, self.slots, self.nq, self.model.eos_token_id, self.dev
        out, rows_host = [], {}
        for b in sched.wants_eos(self.rem):
            rows_host[b] = delayed[b:b + 1].cpu()
            r = sched.rows[b]
            sched.set_eos(b, finalise_row(rows_host[b], r.prefix_len, r.max_new_tokens, slots, nq, eos)[1])
        known = {b: sched.rows[b] for b in range(slots) if sched.rows[b] is not None}
        tails = {}
        for b, index, end in sched.due():
            row = rows_host[b] if b in rows_host else delayed[b:b + 1].cpu()
            codes, _, end_b = finalise_row(row, known[b].prefix_len, known[b].max_new_tokens, slots, nq, eos)
            assert end_b == end, (end_b, end)
            held = [b] if known[b].partner is None else [b, known[b].partner]
            if self.mixed and self.trace is not None:
                self.trace.setdefault("retired", []).append((index, held, delayed[held].cpu()))
            for slot in held:                          # a guided request of a mixed session leaves both of its rows at once
                self.eng.call("zn_gen_retire", slot)
            if self.streaming:
                tails[index] = codes[..., self.ledger.close(b, codes.shape[2]):].to(dev)
            else:
                out.append(ServeResult(index, codes.to(dev), None))
        if self.streaming:
            # the frames that became final in the rows that run on, built on the device; then every window in one DAC pass
            pieces = {known[b].index: map_codes(revert_delay_pattern(delayed[b:b + 1, :, lo:hi + nq].to(torch.int64)))
                      for b, lo, hi in self.ledger.take(self.own)}
            wavs = self.dacs.push({**pieces, **tails}, end=set(tails))
            out += [ServeChunk(index, c, wavs[index], False, None) for index, c in pieces.items()]
            out += [ServeChunk(index, c, wavs[index], True, None) for index, c in tails.items()]
        return out

    def point(self) -> tuple[list, bool]:
        """One scheduling point -> (what to yield, whether the session has ended)."""
        stats, ts = self.stats, self.ts
        with torch.inference_mode(), torch.cuda.device(self.dev), torch.cuda.stream(ts):
            admitted, refused = self.sched.pull(self.source, self.accept)
            out = [ServeChunk(index, None, None, True, err) if self.streaming else ServeResult(index, None, err) for index, err in refused]
            if admitted:
                timed = stats is not None and stats.get("time_admissions")
                if timed:
                    ts.synchronize()
                    t0 = time.perf_counter()
                self.admit(admitted)
                if timed:
                    ts.synchronize()
                    stats["admit_seconds"] = stats.get("admit_seconds", 0.0) + time.perf_counter() - t0
                if stats is not None:
                    stats["admissions"] = stats.get("admissions", 0) + 1
                    stats["admitted"] = stats.get("admitted", 0) + len(admitted)
            stop = self.sched.finished()
            if not stop and not self.sched.all_idle():
                self._steps()
                out += self._retire()
        return out, stop
