"""The host side of `Zonos.serve()`: which request holds which slot of a running batch, and when it leaves - and of
`Zonos.serve_stream()`: which frames of a slot's row are final while it still runs (`StreamLedger`).

Pure Python: no torch device, no library.  A session has `slots` rows that step together; a request joins at a scheduling point (every
`sched_every` decode steps), runs its own decode loop inside its slot - the device keeps the slot's length, stop state, parameters, column
and step origin per row - and is retired at the first scheduling point at which a `generate_batch()` call of `slots` requests would have
stopped watching it (`row_end_offset`).  Its codes are then cut and finalised exactly as `rows.finalise_row` does for that call.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Iterator, NamedTuple, Sequence

from .rows import check_request_shapes, row_end_offset, stop_check_at     # noqa: F401  (the last two: defined there, re-exported here)

STOP_CHECK_SPAN = 16          # a row whose remaining_steps reached 0 leaves at the next check of its own cadence: at most 16 steps on


def release_limit(offset: int, nq: int, eos_frame: int | None) -> int:
    """Frames [0, limit) that are final while the generation runs, once the steps up to column `offset` have run: a frame is complete
    when its codebook nq-1 (column f + nq) is written, and every frame before the first one whose codebook 0 is EOS (`eos_frame`, None
    while there is none) survives `finalise_codes` (codebooks 1.. cannot sample EOS before the stop; the EOS diagonal after it lands on
    the stop frame itself).  What the end keeps beyond that, `finalise_codes` decides."""
    limit = max(0, offset - nq + 1)
    return limit if eos_frame is None else min(limit, eos_frame)


def serve_slack(sched_every: int) -> int:
    """The furthest a row can run past its own end before it is retired: to the next check of its own cadence, then to the next
    scheduling point."""
    return STOP_CHECK_SPAN + int(sched_every)


def check_serve_request(cond_shape: Sequence[int], prefix_shape: Sequence[int] | None, max_new_tokens, cfg_scale: float, *, nq: int,
                        d_model: int, guided: bool | None, max_len: int, width: int, slack: int) -> tuple[int, int]:
    """What a session refuses (ValueError) before the request takes a slot; returns (L, P), its conditioning positions and audio prefix
    frames.  `max_len`: KV positions per row of the session; `width`: columns of a row of its code buffer.  A request fits when its
    prompt, its own steps and the slack stay inside both: L + P + max_new_tokens + nq + slack <= max_len (the last append of an
    overrunning row) and P + max_new_tokens + nq + slack <= width (its penalty history stays in its own buffer row).  `guided=None`: a
    mixed session takes both kinds; the conditioning's first dimension follows the request's own cfg_scale."""
    if guided is None:
        halves = 2 if float(cfg_scale) != 1.0 else 1
    else:
        halves = 2 if guided else 1
    if guided is not None and (float(cfg_scale) != 1.0) != guided:
        raise ValueError(f"serve: cfg_scale={cfg_scale} in a session {'with' if guided else 'without'} guidance (guided and cfg_scale == 1 "
                         "requests cannot share a session: the row layout differs)")
    L, P = check_request_shapes("serve: ", cond_shape, halves, d_model, cfg_scale, max_new_tokens, prefix_shape, nq)
    n = int(max_new_tokens)
    if L + P + n + nq + slack > max_len:
        raise ValueError(f"serve: {L} conditioning positions + {P} prefix frames + {n} frames + {nq} + slack {slack} exceed the session's "
                         f"{max_len} KV positions per row (max_prompt / max_new_tokens of serve())")
    if P + n + nq + slack > width:
        raise ValueError(f"serve: {P} prefix frames + {n} frames + {nq} + slack {slack} exceed the session's code buffer width {width}")
    return L, P


class ServeResult(NamedTuple):
    """One request of `Zonos.serve()`: its pull index, and either its codes (int64 [1, 9, P + T], as `generate_batch` returns them) or
    the ValueError that refused it."""
    index: int
    codes: object
    error: Exception | None = None


@dataclass
class _Row:
    index: int                  # the request's pull index
    prefix_len: int
    max_new_tokens: int
    step0: int                  # the session step at which it was admitted
    eos_known: bool = False
    eos_column: int | None = None
    partner: int | None = None  # a request that holds two slots (a guided request of a mixed session): the other one
    owner: bool = True          # the slot whose row the request is read from; the second slot only runs along


class SlotScheduler:
    """Admits requests FIFO into free slots, retires rows, and says when the session ends.  The caller drives it at every scheduling
    point: `pull` (admissions), `advance` (the steps it enqueued), `wants_eos` / `set_eos` (the codebook-0 cells of the rows whose
    remaining_steps reached 0), `due` (the rows to retire).

    A request needs one slot, or two (a guided request of a mixed session: `accept` returns a third value).  Admission
    stays FIFO without overtaking: a two-slot request at the head of the queue waits, held in `waiting`, until two slots are idle, and
    nothing behind it is pulled meanwhile.  It takes the two lowest idle slots, the lower one as its owner (`partner`, `is_owner`); both
    are admitted at one scheduling point and retired at one - the point at which the owner's row is due."""

    def __init__(self, slots: int, nq: int, sched_every: int):
        if int(slots) < 1 or int(sched_every) < 1 or int(nq) < 1:
            raise ValueError(f"SlotScheduler: slots={slots}, nq={nq}, sched_every={sched_every} must all be >= 1")
        self.slots, self.nq, self.sched_every = int(slots), int(nq), int(sched_every)
        self.slack = serve_slack(sched_every)
        self.step = 0                                  # decode steps of the session so far
        self.rows: list[_Row | None] = [None] * self.slots
        self.pulled = 0                                # items that were requests (an index each)
        self.exhausted = False
        self.waiting: tuple | None = None              # (index, item, prefix_len, max_new_tokens, need): pulled, accepted, not yet placed

    # ---------------------------------------------------------------- admission
    def free_slots(self) -> list[int]:
        return [b for b, r in enumerate(self.rows) if r is None]

    def pull(self, source: Iterator, accept: Callable) -> tuple[list, list]:
        """One scheduling point's admissions: while a slot is free, take the next item of `source` - lazily, one item per free slot.
        None: nothing is waiting right now.  `accept(request)` returns (prefix_len, max_new_tokens) - or (prefix_len, max_new_tokens,
        slots needed: 1 or 2) - or raises ValueError: a refused request takes no slot.  A request that needs more slots than are free
        stays at the head of the queue (`waiting`) and ends this point's admissions.  Returns ([(slot, index, request)], [(index, error)]);
        a two-slot request is named once, by its owner slot (`partner(slot)` is its other one)."""
        admitted, refused = [], []
        while True:
            free = self.free_slots()
            if not free:
                break
            if self.waiting is None:
                if self.exhausted:
                    break
                try:
                    item = next(source)
                except StopIteration:
                    self.exhausted = True
                    break
                if item is None:
                    break
                index, self.pulled = self.pulled, self.pulled + 1
                try:
                    got = tuple(accept(item))
                    need = int(got[2]) if len(got) > 2 else 1
                    if need not in (1, 2) or need > self.slots:
                        raise ValueError(f"serve: the request needs {need} slots, the session has {self.slots}")
                except ValueError as e:
                    refused.append((index, e))
                    continue
                self.waiting = (index, item, int(got[0]), int(got[1]), need)
            index, item, prefix_len, max_new, need = self.waiting
            if need > len(free):
                break                                   # the head of the queue waits for a second idle slot; nothing overtakes it
            self.waiting = None
            own = free[0]
            self.rows[own] = _Row(index, prefix_len, max_new, self.step, partner=free[1] if need == 2 else None)
            if need == 2:
                self.rows[free[1]] = _Row(index, prefix_len, max_new, self.step, partner=own, owner=False)
            admitted.append((own, index, item))
        return admitted, refused

    def partner(self, slot: int) -> int | None:
        r = self.rows[slot]
        return None if r is None else r.partner

    def is_owner(self, slot: int) -> bool:
        r = self.rows[slot]
        return r is not None and r.owner

    # ---------------------------------------------------------------- the steps
    def advance(self, steps: int | None = None) -> None:
        self.step += self.sched_every if steps is None else int(steps)

    def own_steps(self, slot: int) -> int:
        r = self.rows[slot]
        return -1 if r is None else self.step - r.step0

    def holders(self) -> list[int | None]:
        return [None if r is None else r.index for r in self.rows]

    # ---------------------------------------------------------------- retirement
    def wants_eos(self, remaining: Sequence[int]) -> list[int]:
        """The busy slots whose remaining_steps reached 0 (stopped, or budget spent) and whose first codebook-0 EOS column is not known
        yet: every column that decides it has been written."""
        return [b for b, r in enumerate(self.rows) if r is not None and r.owner and not r.eos_known and remaining[b] <= 0]

    def set_eos(self, slot: int, eos_column: int | None) -> None:
        r = self.rows[slot]
        r.eos_known, r.eos_column = True, eos_column

    def end_offset(self, slot: int) -> int:
        r = self.rows[slot]
        offset0 = r.prefix_len + 1
        return row_end_offset(offset0, r.prefix_len + r.max_new_tokens + self.nq, self.slots, self.nq, r.eos_column)

    def due(self) -> list[tuple[int, int, int]]:
        """(slot, index, end offset) of every row whose own loop has left by now; the slots become idle.  A two-slot request is named by
        its owner slot, and its second slot (`partner`, asked before this call) becomes idle with it."""
        out = []
        for b, r in enumerate(self.rows):
            if r is None or not r.owner or not r.eos_known:
                continue
            end = self.end_offset(b)
            if self.step - r.step0 >= end - (r.prefix_len + 1):
                out.append((b, r.index, end))
                self.rows[b] = None
                if r.partner is not None:
                    self.rows[r.partner] = None
        return out

    def all_idle(self) -> bool:
        return all(r is None for r in self.rows)

    def finished(self) -> bool:
        return self.exhausted and self.waiting is None and self.all_idle()


class ServeChunk(NamedTuple):
    """One piece of one request of `Zonos.serve_stream()`: the frames that became final (int64 [1, 9, k], in the coordinates of
    `ServeResult.codes`: an audio prefix comes first) and the samples they completed (float32 [1, 1, m] on the model's device); k or m
    may be 0.  `done`: the request's last chunk.  A refused request yields one chunk with codes = wav = None, done and its ValueError."""
    index: int
    codes: object
    wav: object
    done: bool
    error: Exception | None = None


@dataclass
class _Tap:
    prefix_len: int
    max_new_tokens: int
    released: int = 0               # frames handed out
    scanned: int = 0                # codebook-0 columns up to here have been looked at
    eos_frame: int | None = None    # the first generated frame whose codebook 0 is EOS


class StreamLedger:
    """Per slot of a streaming session: the frames released, the codebook-0 columns scanned and the first EOS frame.  A slot's own column
    after `own` steps is prefix + 1 + own (a step writes the column after the one it read), capped at the last column of its row,
    prefix + max_new_tokens + nq - 1: an overrunning row writes beyond its own columns only.  The frames [0, release_limit(column)) are
    final; a chunk goes out when they have grown by `chunk_frames`.  The caller drives it at every scheduling point: `cells` (which
    codebook-0 cells to read, for all slots in one gather), `scan` (what they held), `close` (the rows retired at this point), `take`
    (the chunks of the rows that run on).  Of a request that holds two slots (a mixed session) only the owner slot is opened here: its
    second slot holds the same cells."""

    def __init__(self, nq: int, chunk_frames: int, eos_id: int):
        if int(chunk_frames) < 1:
            raise ValueError(f"chunk_frames must be >= 1, got {chunk_frames}")
        self.nq, self.chunk_frames, self.eos_id = int(nq), int(chunk_frames), int(eos_id)
        self.taps: dict[int, _Tap] = {}

    def open(self, slot: int, prefix_len: int, max_new_tokens: int) -> None:
        if slot in self.taps:
            raise ValueError(f"StreamLedger: slot {slot} is already open")
        self.taps[slot] = _Tap(int(prefix_len), int(max_new_tokens), scanned=int(prefix_len))

    def column(self, slot: int, own_steps: int) -> int:
        t = self.taps[slot]
        return min(t.prefix_len + 1 + int(own_steps), t.prefix_len + t.max_new_tokens + self.nq - 1)

    def limit(self, slot: int, own_steps: int) -> int:
        return release_limit(self.column(slot, own_steps), self.nq, self.taps[slot].eos_frame)

    def cells(self, own: Sequence[int]) -> list[tuple[int, int, int]]:
        """(slot, lo, hi): codebook 0 of columns [lo, hi) of the slot's row decides its EOS frame and has not been read."""
        out = []
        for b, t in sorted(self.taps.items()):
            hi = self.column(b, own[b]) + 1
            if t.eos_frame is None and hi > t.scanned + 1:
                out.append((b, t.scanned + 1, hi))
        return out

    def scan(self, slot: int, lo: int, tokens: Sequence[int]) -> None:
        """`tokens`: codebook 0 of columns lo, lo + 1, ... (`cells`).  Column c holds frame c - 1."""
        t = self.taps[slot]
        if lo != t.scanned + 1:
            raise ValueError(f"StreamLedger: slot {slot} scanned to column {t.scanned}, got cells from {lo}")
        for k, tok in enumerate(tokens):
            if t.eos_frame is None and int(tok) == self.eos_id:
                t.eos_frame = lo + k - 1
        t.scanned = lo + len(tokens) - 1

    def take(self, own: Sequence[int]) -> list[tuple[int, int, int]]:
        """(slot, lo, hi): frames [lo, hi) of the slot's row go out now; they count as released."""
        out = []
        for b, t in sorted(self.taps.items()):
            hi = self.limit(b, own[b])
            if hi - t.released >= self.chunk_frames:
                out.append((b, t.released, hi))
                t.released = hi
        return out

    def close(self, slot: int, final_frames: int) -> int:
        """The slot retires with `final_frames` frames: the first frame of its last chunk."""
        t = self.taps.pop(slot)
        if final_frames < t.released:
            raise RuntimeError(f"StreamLedger: slot {slot} released {t.released} frames, its request kept {final_frames}")
        return t.released
