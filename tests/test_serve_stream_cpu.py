"""The host side of Zonos.serve_stream() - the parts that need no GPU.

`StreamLedger` is driven as `Zonos._serve_gen` drives it, beside `SlotScheduler`, against a transcription of the device's per-slot
bookkeeping with all nine codebooks (tests/test_serve_cpu.py's Device keeps codebook 0 only; a row is finalised from all of them), and
`DACStreamSet`'s window arithmetic against `DACStream`'s, key by key, with the device calls replaced by recorders."""
import contextlib
import random
import types

import pytest
import torch

from zonos_amd.autoencoder import DACAutoencoder, DACStream, DACStreamSet, window_step
from zonos_amd.codebook_pattern import apply_delay_pattern, revert_delay_pattern
from zonos_amd.model import Zonos, map_codes
from zonos_amd.serving import ServeChunk, SlotScheduler, StreamLedger, release_limit, serve_slack

NQ, EOS, MASK = 9, 1024, 1025
FINALISER = types.SimpleNamespace(eos_token_id=EOS)


class Req:
    def __init__(self, budget, prefix=0, eos_at=None):
        self.budget, self.prefix, self.eos_at = budget, prefix, eos_at     # eos_at: the own loop step whose codebook-0 sample is EOS


class Device:
    """Per slot: remaining, stopping, step0 (-1 idle) and the slot's row of the code buffer [nq, width] (frame_update_body's masking, as
    tests/test_stream_cpu.py's run_loop restates it; admit_rows_kernel's words; zn_gen_retire)."""
    def __init__(self, slots, width, seed):
        self.slots, self.width, self.step = slots, width, 0
        self.remaining, self.stopping, self.step0 = [0] * slots, [0] * slots, [-1] * slots
        self.rows = torch.full((slots, NQ, width), MASK, dtype=torch.int64)
        self.req = [None] * slots
        self.gen = torch.Generator().manual_seed(seed)

    def _sample(self):
        return torch.randint(0, 1024, (NQ,), generator=self.gen)

    def admit(self, b, r):
        assert self.step0[b] == -1
        codes = torch.full((1, NQ, self.width - NQ), MASK, dtype=torch.int64)
        codes[..., :r.prefix] = torch.randint(0, 1024, (1, NQ, r.prefix), generator=self.gen)
        codes[..., r.prefix:r.prefix + r.budget] = -1
        self.rows[b] = apply_delay_pattern(codes, MASK)[0]
        self.remaining[b], self.stopping[b], self.step0[b], self.req[b] = r.budget + NQ - 1, 0, self.step, r
        c = self.rows[b, :, r.prefix + 1]
        c.copy_(torch.where(c == -1, self._sample(), c))                   # the first frame: plain write-where-unknown

    def run(self, n):
        cb = torch.arange(NQ)
        for _ in range(n):
            for b in range(self.slots):
                rem, stop = self.remaining[b], self.stopping[b]
                if self.step0[b] >= 0:
                    r, own = self.req[b], self.step - self.step0[b]
                    nxt = self._sample()
                    if r.eos_at == own:
                        nxt[0] = EOS
                        rem, stop = min(rem, NQ), 1
                    if stop:
                        eos_idx = min(NQ - rem, NQ - 1)
                        nxt = torch.where(cb < eos_idx, MASK, torch.where(cb == eos_idx, EOS, nxt))
                    col = r.prefix + 1 + own + 1
                    if col < self.width:
                        c = self.rows[b, :, col]
                        c.copy_(torch.where(c == -1, nxt, c))
                rem -= 1
                self.remaining[b], self.stopping[b] = rem, stop
            self.step += 1

    def retire(self, b):
        self.remaining[b], self.step0[b], self.req[b] = 0, -1, None

    def own(self):
        return [-1 if s < 0 else self.step - s for s in self.step0]


def finalise(dev, b, r, slots):
    return Zonos._finalise_row(FINALISER, dev.rows[b:b + 1], r.prefix, r.budget, slots, NQ)


def drive(source, slots, sched_every, chunk_frames, seed):
    """The loop of Zonos._serve_gen with chunk_frames on the transcribed device.  Per request index: the (lo, hi, codes) of its chunks in
    order, the tail's first frame, and the final codes."""
    width = max(r.prefix + r.budget for r in source) + NQ + serve_slack(sched_every)
    dev, sched, ledger = Device(slots, width, seed), SlotScheduler(slots, NQ, sched_every), StreamLedger(NQ, chunk_frames, EOS)
    it = iter(source)
    chunks, tails, finals, reqs = {}, {}, {}, {}
    guard = 0
    while True:
        guard += 1
        assert guard < 100000
        admitted, _ = sched.pull(it, lambda r: (r.prefix, r.budget))
        for slot, index, r in admitted:
            dev.admit(slot, r)
            ledger.open(slot, r.prefix, r.budget)
            chunks[index], reqs[index] = [], r
        if sched.finished():
            break
        dev.run(sched_every)
        sched.advance()
        own = dev.own()
        assert own == [sched.own_steps(b) for b in range(slots)]
        for b, lo, hi in ledger.cells(own):
            assert lo <= hi - 1 <= dev.req[b].prefix + dev.req[b].budget + NQ - 1, "only columns of the row itself are read"
            ledger.scan(b, lo, dev.rows[b, 0, lo:hi].tolist())
        for b in sched.wants_eos(dev.remaining):
            sched.set_eos(b, finalise(dev, b, dev.req[b], slots)[1])
        known = {b: (sched.rows[b].index, dev.req[b]) for b in range(slots) if sched.rows[b] is not None}
        for b, index, end in sched.due():
            final, _, end_b = finalise(dev, b, known[b][1], slots)
            assert end_b == end
            tails[index], finals[index] = ledger.close(b, final.shape[2]), final
            dev.retire(b)
        for b, lo, hi in ledger.take(own):
            index, r = known[b]
            assert sched.rows[b] is not None, "a retired slot gets its last chunk only"
            # the independent statement of the rule: the slot's own column, and the first generated frame whose codebook 0 is EOS
            col = min(r.prefix + 1 + own[b], r.prefix + r.budget + NQ - 1)
            hit = (dev.rows[b, 0, r.prefix + 1:col + 1] == EOS).nonzero()
            eos_frame = r.prefix + int(hit[0, 0]) if len(hit) else None
            assert hi <= release_limit(col, NQ, eos_frame), (index, hi, col, eos_frame)
            assert hi - lo >= chunk_frames
            chunks[index].append((lo, hi, map_codes(revert_delay_pattern(dev.rows[b:b + 1, :, lo:hi + NQ]))))
    assert not ledger.taps
    return reqs, chunks, tails, finals


@pytest.mark.parametrize("slots", [1, 2, 3, 4])
@pytest.mark.parametrize("sched_every", [1, 5, 8])
def test_ledger_on_random_sessions(slots, sched_every):
    rng = random.Random(31 * slots + sched_every)
    early = short = 0
    for trial in range(10):
        source = []
        for _ in range(rng.randint(1, 7)):
            budget = rng.randint(1, 60)
            source.append(Req(budget, rng.randint(0, 7), rng.choice([None, 0, 3, budget - 1])))
        chunk_frames = rng.choice([1, 4, 8, 16])
        reqs, chunks, tails, finals = drive(source, slots, sched_every, chunk_frames, seed=1000 * slots + 10 * sched_every + trial)
        assert sorted(finals) == list(range(len(source))), "every request retires once"
        for index, final in finals.items():
            at = 0
            for lo, hi, codes in chunks[index]:
                assert lo == at and hi > lo, "the chunks' frame ranges are contiguous from 0"
                at = hi
            assert tails[index] == at
            # no frame is released that finalise_codes later cuts, and the released frames are the final ones
            assert at <= final.shape[2], (index, at, final.shape)
            for lo, hi, codes in chunks[index]:
                assert torch.equal(codes, final[..., lo:hi]), (index, lo, hi)
            # released frames plus the tail released at retirement: the length of the result
            assert at + final[..., tails[index]:].shape[2] == final.shape[2]
            early += bool(chunks[index])
            short += final.shape[2] < reqs[index].prefix + reqs[index].budget
    assert early > 0, "some request must get frames before it retires"
    assert short > 0, "some scripted EOS must shorten a result"


def test_ledger_refuses_misuse_and_a_result_shorter_than_what_it_released():
    led = StreamLedger(NQ, 4, EOS)
    led.open(0, 2, 30)
    with pytest.raises(ValueError):
        led.open(0, 0, 5)
    assert led.column(0, 0) == 3 and led.column(0, 1000) == 2 + 30 + NQ - 1
    assert led.cells([0]) == [(0, 3, 4)]
    led.scan(0, 3, [5])
    assert led.cells([0]) == [] and led.take([0]) == []
    assert led.cells([16]) == [(0, 4, 20)]
    with pytest.raises(ValueError):
        led.scan(0, 5, [5])
    led.scan(0, 4, [5] * 16)
    assert led.take([16]) == [(0, 0, 11)] and led.take([16]) == []        # column 19: frames 0 .. 10 are complete
    with pytest.raises(RuntimeError):
        led.close(0, 10)
    with pytest.raises(ValueError):
        StreamLedger(NQ, 0, EOS)
    c = ServeChunk(4, None, None, True, ValueError("x"))
    assert c.done and c.codes is None and c.index == 4


# ------------------------------------------------------------------------------------------------ DACStreamSet's host arithmetic
def _recorders(ae):
    """A DACStream and a DACStreamSet whose device calls only record what they were asked for."""
    log = {"single": [], "rows": []}

    def single(win, c0, at_end, m):
        log["single"].append((c0, win.shape[2], bool(at_end), m))
        return torch.zeros(win.shape[0], 1, m)

    def rows(codes, rr, t_max):
        assert codes.shape[0] == len(rr) and codes.shape[2] == max(n for _, n, _ in rr)
        log["rows"].append(([(c0, n, bool(e)) for c0, n, e in rr], t_max))
        return torch.zeros(len(rr), t_max)

    def make_stream():
        st = DACStream(ae)
        st._ctx, st._decode = contextlib.nullcontext, single
        return st
    ss = DACStreamSet(ae)
    ss._ctx, ss._decode_rows = contextlib.nullcontext, rows
    return make_stream, ss, log


@pytest.mark.parametrize("ratios", [(8, 8, 4, 2), (6, 2), (2, 6, 10)])
def test_stream_set_arithmetic_is_dac_streams_key_by_key(ratios):
    ae = DACAutoencoder(config=dict(upsampling_ratios=ratios), device="cpu")
    make_stream, ss, log = _recorders(ae)
    rng = random.Random(sum(ratios))
    lengths = {"a": 40, "b": 96, "c": 7, "d": 1, "e": 130}
    start = {"a": 0, "b": 2, "c": 1, "d": 3, "e": 0}
    sizes = {}
    for k, T in lengths.items():
        sizes[k], left = [], T
        while left:
            sizes[k].append(min(left, rng.choice([1, 7, 2, 23, 5, 64, 3])))
            left -= sizes[k][-1]
    singles, total, call = {}, {k: 0 for k in lengths}, 0
    while any(call - start[k] < len(sizes[k]) for k in lengths):
        chunks, end = {}, set()
        for k in lengths:
            i = call - start[k]
            if 0 <= i < len(sizes[k]):
                chunks[k] = torch.zeros(1, 9, sizes[k][i], dtype=torch.int64)
                if i == len(sizes[k]) - 1:
                    end.add(k)
        n_single, n_rows = len(log["single"]), len(log["rows"])
        want, want_rows = {}, []
        for k, c in chunks.items():
            st = singles.setdefault(k, make_stream())
            before = len(log["single"])
            w = st.push(c)
            if k in end:
                w = torch.cat([w, st.flush()], dim=2)
            want[k] = w.shape[2]
            if k not in end:                               # (a DACStream that ends decodes twice: push, then flush; the set flushes in one row)
                want_rows += [r[:3] for r in log["single"][before:]]
        got = ss.push(chunks, end=end)
        assert set(got) == set(chunks)
        assert len(log["rows"]) - n_rows <= 1, "one device call per push"
        rows_now = log["rows"][-1][0] if len(log["rows"]) > n_rows else []
        for k in chunks:
            assert got[k].shape == (1, 1, want[k]), (k, call)
            total[k] += want[k]
            if k in end:
                assert k not in ss
            else:
                st, w = singles[k], ss._keys[k]
                assert (w.c0, w.win.shape[2], w.emitted) == (st._c0, st._win.shape[2], st._emitted), (k, call)
        assert [r for r in rows_now if not r[2]] == want_rows, "the rows of keys that run on are DACStream's own calls; an idle key takes no row"
        assert sum(1 for r in rows_now if r[2]) == len(end), "a key that ends is flushed in one row of the same call"
        call += 1
    assert len(ss) == 0
    assert total == {k: ae.hop * T for k, T in lengths.items()}, "every sample of every key comes out once"
    assert any(len(rows) > 1 for rows, _ in log["rows"]), "some push decodes several keys in one call"


def test_window_step_is_the_shared_arithmetic():
    ae = DACAutoencoder(device="cpu")
    lead = ae.span(1, 1 << 12, True)[0] - ae.hop
    assert window_step(ae.span, ae.hop, lead, 0, 0, 0, False) is None
    assert window_step(ae.span, ae.hop, lead, 0, 3, 0, False) is None          # three frames complete no sample yet
    s0, s1, skip, keep = window_step(ae.span, ae.hop, lead, 0, 40, 0, False)
    assert (s0, skip, keep) == (0, 0, (s1 - lead) // ae.hop) and 0 < s1 < 40 * ae.hop
    s0b, s1b, skipb, _ = window_step(ae.span, ae.hop, lead, keep, 40 - keep, s1, True)
    assert s0b <= s1 and skipb == s1 - s0b and s1b == 40 * ae.hop
    with pytest.raises(RuntimeError):
        window_step(ae.span, ae.hop, lead, 30, 10, 0, True)
