"""The scheduler of Zonos.serve() (zonos_amd/serving.py) - the parts that need no GPU.

`SlotScheduler` is driven exactly as `Zonos._serve_gen` drives it, against a transcription of the device's per-slot bookkeeping
(zn_decode_kernels.h frame_update_body for codebook 0, admit_rows_kernel's words, zn_gen_retire): remaining_steps, stopping, the step
origin and codebook 0 of each slot's row of the code buffer, on scripted EOS steps.  `check_serve_request` holds what a session refuses."""
import heapq
import random

import pytest

from zonos_amd import model as zmodel
from zonos_amd.serving import ServeResult, SlotScheduler, check_serve_request, row_end_offset, serve_slack

NQ, EOS, MASK = 9, 1024, 1025


class Req:
    def __init__(self, budget, prefix=0, eos_at=None):
        self.budget, self.prefix, self.eos_at = budget, prefix, eos_at     # eos_at: the own loop step whose codebook-0 sample is EOS


class Device:
    """Per slot: remaining, stopping, step0 (-1 idle) and codebook 0 of the row, `width` columns."""
    def __init__(self, slots, width):
        self.slots, self.width, self.step = slots, width, 0
        self.remaining, self.stopping, self.step0 = [0] * slots, [0] * slots, [-1] * slots
        self.row = [[MASK] * width for _ in range(slots)]
        self.req = [None] * slots
        self.first_done = [None] * slots                                   # own steps at which remaining first reached 0

    def admit(self, b, r):
        assert self.step0[b] == -1, f"slot {b} holds two requests"
        assert r.prefix + r.budget + NQ <= self.width
        self.row[b] = [MASK] + [7] * r.prefix + [-1] * r.budget + [MASK] * (self.width - 1 - r.prefix - r.budget)
        self.remaining[b], self.stopping[b], self.step0[b], self.req[b], self.first_done[b] = r.budget + NQ - 1, 0, self.step, r, None
        col = r.prefix + 1                                                 # the first frame: plain write-where-unknown
        if self.row[b][col] == -1:
            self.row[b][col] = 5

    def run(self, n):
        for _ in range(n):
            for b in range(self.slots):
                rem, stop = self.remaining[b], self.stopping[b]
                if self.step0[b] >= 0:
                    r, own = self.req[b], self.step - self.step0[b]
                    tok0 = EOS if r.eos_at == own else 5
                    if tok0 == EOS:
                        rem, stop = min(rem, NQ), 1
                    eos_idx = min(NQ - rem, NQ - 1)
                    t = tok0
                    if stop and 0 < eos_idx:
                        t = MASK
                    elif stop and 0 == eos_idx:
                        t = EOS
                    col = r.prefix + 1 + own + 1
                    if 0 <= col < self.width and self.row[b][col] == -1:
                        self.row[b][col] = t
                rem -= 1
                self.remaining[b], self.stopping[b] = rem, stop
                if self.step0[b] >= 0 and rem <= 0 and self.first_done[b] is None:
                    self.first_done[b] = self.step + 1 - self.step0[b]
            self.step += 1

    def retire(self, b):
        assert self.step0[b] >= 0
        self.remaining[b], self.step0[b], self.req[b] = 0, -1, None

    def own(self):
        return [-1 if s < 0 else self.step - s for s in self.step0]

    def eos_column(self, b):
        r = self.req[b]
        offset0, t_b = r.prefix + 1, r.prefix + r.budget + NQ
        return next((c for c in range(offset0 + 1, t_b) if self.row[b][c] == EOS), None)


def drive(source, slots, sched_every, width=None):
    """The loop of Zonos._serve_gen on the transcribed device -> (events, device, scheduler).  events: ("admit", step, slot, index, req),
    ("retire", step, slot, index, req, end, own steps, own steps at which remaining first reached 0), ("refuse", step, index)."""
    reqs = [r for r in source if r is not None]
    width = width or max(r.prefix + r.budget for r in reqs) + NQ + serve_slack(sched_every)
    dev, sched, events = Device(slots, width), SlotScheduler(slots, NQ, sched_every), []
    it = iter(source)

    def accept(r):
        if r.prefix + r.budget + NQ + sched.slack > width:
            raise ValueError("too wide")
        return r.prefix, r.budget
    guard = 0
    while True:
        guard += 1
        assert guard < 100000
        admitted, refused = sched.pull(it, accept)
        events += [("refuse", sched.step, index) for index, _ in refused]
        for slot, index, r in admitted:
            dev.admit(slot, r)
            events.append(("admit", sched.step, slot, index, r))
        if sched.finished():
            break
        if sched.all_idle():
            continue
        dev.run(sched_every)
        sched.advance()
        assert dev.own() == [sched.own_steps(b) for b in range(slots)]
        held = {b: (dev.req[b], dev.first_done[b]) for b in range(slots)}
        for b in sched.wants_eos(dev.remaining):
            sched.set_eos(b, dev.eos_column(b))
        for b, index, end in sched.due():
            r, first_done = held[b]
            events.append(("retire", sched.step, b, index, r, end, dev.own()[b], first_done))
            dev.retire(b)
    return events, dev, sched


def check_session(source, slots, sched_every):
    events, dev, sched = drive(source, slots, sched_every)
    reqs = [r for r in source if r is not None]
    admits = [e for e in events if e[0] == "admit"]
    retires = [e for e in events if e[0] == "retire"]
    assert [e[3] for e in admits] == list(range(len(reqs))), "admission is FIFO and every request is admitted once"
    assert sorted(e[3] for e in retires) == list(range(len(reqs)))
    assert [e[1] for e in admits] == sorted(e[1] for e in admits)
    for _, step, slot, index, r, end, own, first_done in retires:
        t0 = next(e[1] for e in admits if e[3] == index)
        offset0, t_b = r.prefix + 1, r.prefix + r.budget + NQ
        # the true first EOS column follows from the script: the stop step writes EOS into codebook 0 only while remaining >= nq
        eos_col = None
        if r.eos_at is not None and r.eos_at <= r.budget - 2:
            eos_col = offset0 + r.eos_at + 1
        want = row_end_offset(offset0, t_b, slots, NQ, eos_col)
        assert end == want, (index, end, want)
        need = want - offset0
        assert step % sched_every == 0 and own == step - t0
        assert own >= need, f"request {index} retired {need - own} steps early"
        assert own - sched_every < need, f"request {index} was due one scheduling point earlier"
        assert first_done is not None and own - first_done <= sched.slack, f"request {index} ran {own - first_done} steps past its end"
    # the session ends exactly when the source is exhausted and every slot is idle: no step after the last retirement
    assert sched.finished() and dev.own() == [-1] * slots
    assert dev.step == (max(e[1] for e in retires) if retires else 0)
    return events, dev


# ------------------------------------------------------------------------------------------------ sessions
@pytest.mark.parametrize("slots", [1, 2, 3, 4])
@pytest.mark.parametrize("sched_every", [1, 8, 16])
def test_random_sessions(slots, sched_every):
    rng = random.Random(1000 * slots + sched_every)
    for _ in range(12):
        source = []
        for _ in range(rng.randint(1, 9)):
            budget = rng.randint(3, 40)
            eos_at = rng.choice([None, None, rng.randint(0, budget + NQ)])
            source.append(Req(budget, rng.choice([0, 1, 5, 12]), eos_at))
            if rng.random() < 0.3:
                source += [None] * rng.randint(1, 3)
        check_session(source, slots, sched_every)


@pytest.mark.parametrize("slots", [1, 2, 3, 4])
@pytest.mark.parametrize("sched_every", [1, 8, 16])
def test_total_steps_without_eos_follow_from_the_budgets(slots, sched_every):
    """No EOS, every request waiting from the start: request i takes the slot that frees first (the lowest on a tie) and holds it for
    ceil((budget + nq - 1) / sched_every) scheduling intervals; the session runs until the last slot frees."""
    rng = random.Random(77 * slots + sched_every)
    for _ in range(10):
        budgets = [rng.randint(3, 60) for _ in range(rng.randint(1, 12))]
        events, dev = check_session([Req(b, rng.choice([0, 5])) for b in budgets], slots, sched_every)
        free = [(0, b) for b in range(slots)]
        heapq.heapify(free)
        end = 0
        for budget in budgets:
            at, slot = heapq.heappop(free)
            need = budget + NQ - 1
            at += -(-need // sched_every) * sched_every
            end = max(end, at)
            heapq.heappush(free, (at, slot))
        assert dev.step == end, (budgets, dev.step, end)


def test_none_items_admit_nothing_and_requests_are_pulled_lazily():
    pulled = []

    def source():
        for k, item in enumerate([Req(5), None, Req(6), Req(7), None, None, Req(4)]):
            pulled.append(k)
            yield item
    sched, dev = SlotScheduler(2, NQ, 8), Device(2, 80)
    it = source()
    admitted, _ = sched.pull(it, lambda r: (r.prefix, r.budget))
    assert [(s, i) for s, i, _ in admitted] == [(0, 0)] and pulled == [0, 1], "a None item ends the point's admissions"
    admitted, _ = sched.pull(it, lambda r: (r.prefix, r.budget))
    assert [(s, i) for s, i, _ in admitted] == [(1, 1)] and pulled == [0, 1, 2], "an item is pulled only for a free slot"
    assert sched.pull(it, lambda r: (r.prefix, r.budget)) == ([], []) and pulled == [0, 1, 2]
    assert not sched.finished() and sched.holders() == [0, 1]
    events, _, _ = drive([Req(5), None, Req(6), Req(7), None, None, Req(4)], 2, 8)
    assert [e[3] for e in events if e[0] == "admit"] == [0, 1, 2, 3]


def test_a_refused_request_takes_no_slot():
    def accept(r):
        if r.budget > 10:
            raise ValueError("too long")
        return r.prefix, r.budget
    sched = SlotScheduler(2, NQ, 8)
    admitted, refused = sched.pull(iter([Req(50), Req(4), Req(60), Req(70), Req(5)]), accept)
    assert [(s, i) for s, i, _ in admitted] == [(0, 1), (1, 4)]
    assert [i for i, _ in refused] == [0, 2, 3] and all(isinstance(e, ValueError) for _, e in refused)
    assert not sched.exhausted and sched.pulled == 5


def test_an_empty_source_ends_the_session_at_once():
    events, dev, sched = drive([], 3, 8, width=40)
    assert events == [] and dev.step == 0 and sched.finished()
    with pytest.raises(ValueError):
        SlotScheduler(0, NQ, 8)
    with pytest.raises(ValueError):
        SlotScheduler(2, NQ, 0)


def test_the_model_module_uses_the_schedulers_own_arithmetic():
    assert zmodel.row_end_offset is row_end_offset and zmodel.ServeResult is ServeResult
    assert serve_slack(8) == 24 and SlotScheduler(2, NQ, 8).slack == 24
    assert ServeResult(3, None, ValueError("x")).codes is None


# ------------------------------------------------------------------------------------------------ refusals
KW = dict(nq=NQ, d_model=128, guided=True, max_len=64, width=50, slack=24)


def test_check_serve_request_refuses_and_holds_the_capacity_rule_at_its_boundary():
    assert check_serve_request((2, 10, 128), (1, NQ, 5), 8, 2.0, **KW) == (10, 5)
    assert check_serve_request((1, 10, 128), None, 8, 1.0, **{**KW, "guided": False}) == (10, 0)
    for cond, prefix, n, cfg, word in [((2, 10, 128), None, 8, 1.0, "cfg_scale"),            # unguided in a guided session
                                       ((1, 10, 128), None, 8, 2.0, "conditioning"),         # one half only
                                       ((2, 10, 64), None, 8, 2.0, "conditioning"),
                                       ((2, 0, 128), None, 8, 2.0, "conditioning"),
                                       ((2, 10), None, 8, 2.0, "conditioning"),
                                       ((2, 10, 128), None, 0, 2.0, "max_new_tokens"),
                                       ((2, 10, 128), None, 2.5, 2.0, "max_new_tokens"),
                                       ((2, 10, 128), (1, 8, 5), 8, 2.0, "audio_prefix_codes"),
                                       ((2, 10, 128), (2, NQ, 5), 8, 2.0, "audio_prefix_codes")]:
        with pytest.raises(ValueError, match=word):
            check_serve_request(cond, prefix, n, cfg, **KW)
    with pytest.raises(ValueError, match="cfg_scale"):
        check_serve_request((1, 10, 128), None, 8, 2.0, **{**KW, "guided": False})
    # KV capacity: L + P + n + nq + slack <= max_len.  10 + 5 + 16 + 9 + 24 = 64
    assert check_serve_request((2, 10, 128), (1, NQ, 5), 16, 2.0, **{**KW, "width": 100}) == (10, 5)
    with pytest.raises(ValueError, match="KV positions"):
        check_serve_request((2, 10, 128), (1, NQ, 5), 16, 2.0, **{**KW, "width": 100, "max_len": 63})
    with pytest.raises(ValueError, match="KV positions"):
        check_serve_request((2, 11, 128), (1, NQ, 5), 16, 2.0, **{**KW, "width": 100})
    # code buffer: P + n + nq + slack <= width.  5 + 12 + 9 + 24 = 50
    assert check_serve_request((2, 3, 128), (1, NQ, 5), 12, 2.0, **KW) == (3, 5)
    with pytest.raises(ValueError, match="width"):
        check_serve_request((2, 3, 128), (1, NQ, 5), 12, 2.0, **{**KW, "width": 49})
    with pytest.raises(ValueError, match="width"):
        check_serve_request((2, 3, 128), (1, NQ, 5), 13, 2.0, **KW)
