"""Every refused call of tests/gen_state_check.cpp made through the C ABI on a synth.TINY_CFG handle, for comparing two builds of the library: one
"label | return code | zn_last_error" line per call, in the CPU check's own labels and format (the call-order lines state by state, where the CPU check goes
entry point by entry point: sort both to compare them).  The two outputs must be equal line for line.

    python tools/gen_refusals.py > OUT.txt

Apart from what a state needs to exist (a prefill, an admission, the steps of the slot script) nothing is launched.  Two of the table's entry points answer
another refusal first on this handle (zn_set_mlp_fp8: widths below 256; zn_set_mamba_fp8: a transformer); their lines are what the library says.
ZONOS_HIP_LIB selects the library."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from zonos_amd import _lib, synth  # noqa: E402
from zonos_amd.rows import sampling_struct  # noqa: E402
from zonos_amd.testing import build_model  # noqa: E402

DEV, NQ, INT_MAX = "cuda:0", 9, 2 ** 31 - 1
STATES = ("no generation", "begun", "row table set", "prefix shifts set", "prefilled", "session opened", "session with a busy slot", "ended")
INSIDE = STATES[1:7]
REFUSED = {      # entry point -> the states that refuse it
    "zn_prefill": ("no generation", "session opened", "session with a busy slot", "ended"),
    "zn_prefill_rows": ("no generation", "session opened", "session with a busy slot", "ended"),
    "zn_gen_set_rows": ("no generation", "prefilled", "session opened", "session with a busy slot", "ended"),
    "zn_gen_set_prefix_rows": ("no generation", "prefilled", "session opened", "session with a busy slot", "ended"),
    "zn_gen_open_slots": ("no generation", "row table set", "prefix shifts set", "prefilled", "session opened", "session with a busy slot", "ended"),
    "zn_gen_admit": ("no generation", "begun", "row table set", "prefix shifts set", "prefilled", "ended"),
    "zn_gen_retire": ("no generation", "begun", "row table set", "prefix shifts set", "prefilled", "ended"),
    "zn_gen_row_state": ("no generation", "begun", "row table set", "prefix shifts set", "prefilled", "ended"),
    "zn_sample_first": ("no generation", "session opened", "session with a busy slot"),
    "zn_decode_steps": ("no generation", "ended"),
    "zn_gen_bind_kv_fp8": ("no generation", "prefilled", "session with a busy slot", "ended"),
    "zn_set_mlp_fp8": INSIDE, "zn_set_mamba_fp8": INSIDE, "zn_set_kv_fp8": INSIDE, "zn_set_kv_fp8_only": INSIDE,
}


def entry(cfg_scale, max_new, penalty=2.0, w0=0, w1=0, window=2, seed=0):
    r = _lib.zn_row_params()
    r.sp = sampling_struct(dict(temperature=0.0, repetition_penalty=penalty, repetition_penalty_window=window), seed)
    r.cfg_scale, r.max_new_tokens, r.reserved[0], r.reserved[1] = cfg_scale, max_new, w0, w1
    return r


def pair_entry(o, f, n=6, penalty=3.0):
    return entry(2.0, n, penalty, o + 1, f + 1)


def paired(r, o, f):
    q = _lib.zn_row_params.from_buffer_copy(r)
    q.reserved[0], q.reserved[1] = o + 1, f + 1
    return q


def request(slot, row_len, prefix_len, params):
    a = _lib.zn_admit()
    a.slot, a.row_len, a.prefix_len, a.params = slot, row_len, prefix_len, params
    return a


class Gen:
    """One generation on the handle: zn_gen_begin on buffers of its own, zn_gen_end when done."""
    def __init__(self, model, eng, batch, guided, max_len, t_total, offset0, max_new, lengths=0):
        self.model, self.eng, self.lib, self.h, self.st = model, eng, eng.lib, eng.h, eng.stream()
        self.batch, self.rows, self.d = batch, 2 * batch if guided else batch, model.config.backbone.d_model
        n_layer = model.config.backbone.n_layer
        self.ip = model.setup_cache(batch_size=self.rows, max_seqlen=max_len)
        self.ip.lengths_per_sample.fill_(lengths)
        self.codes = torch.full((batch, NQ, t_total), model.masked_token_id, dtype=torch.int32, device=DEV)
        kv = (C.c_void_p * n_layer)(*[self.ip.key_value_memory_dict[i][0].data_ptr() for i in range(n_layer)])
        sp = sampling_struct(dict(temperature=0.0), 0)
        eng.call("zn_gen_begin", batch, kv, max_len, self.ip.lengths_per_sample.data_ptr(), self.codes.data_ptr(), t_total, offset0, max_new,
                 2.0 if guided else 1.0, C.byref(sp), self.st)
        self.keep = []

    def hidden(self, rows, S):
        t = torch.zeros(rows, S, self.d, dtype=torch.bfloat16, device=DEV)
        self.keep.append(t)
        return t.data_ptr()

    def say(self, label, rc):
        print("%s | %d | %s" % (label, rc, self.lib.zn_last_error(self.h).decode()), flush=True)

    def set_rows(self, label, rows, n=None):
        t = (_lib.zn_row_params * len(rows))(*rows)
        self.say(label, self.lib.zn_gen_set_rows(self.h, t if rows else None, len(rows) if n is None else n))

    def set_prefix(self, label, lens, n=None):
        self.say(label, self.lib.zn_gen_set_prefix_rows(self.h, (C.c_int32 * len(lens))(*lens) if lens else None, len(lens) if n is None else n))

    def prefill_rows(self, label, lens, S=9):
        self.say(label, self.lib.zn_prefill_rows(self.h, self.hidden(self.rows, S), S, (C.c_int32 * len(lens))(*lens), self.st))

    def admit(self, reqs, S, n=None, null=False):
        halves = 2 if self.rows == 2 * self.batch else 1
        a = (_lib.zn_admit * max(1, len(reqs)))(*reqs)
        return self.lib.zn_gen_admit(self.h, None if null else a, len(reqs) if n is None else n, self.hidden(max(1, len(reqs)) * halves, max(1, S)), S, self.st)

    def end(self):
        torch.cuda.synchronize()
        self.eng.call("zn_gen_end")


def call_order(model, eng):
    lib, h = eng.lib, eng.h
    n_layer = model.config.backbone.n_layer
    for state in STATES:
        g = None
        if state != "no generation":
            g = Gen(model, eng, 2, True, 48, 42, 6 if state == "prefix shifts set" else 1, 8)
        if state == "row table set":
            eng.call("zn_gen_set_rows", (_lib.zn_row_params * 2)(entry(2.0, 5), entry(2.0, 5)), 2)
        elif state == "prefix shifts set":
            eng.call("zn_gen_set_prefix_rows", (C.c_int32 * 2)(5, 2), 2)
        elif state == "prefilled":
            eng.call("zn_prefill", g.hidden(4, 7), 7, g.st)
        elif state in ("session opened", "session with a busy slot"):
            eng.call("zn_gen_open_slots", 24)
            if state == "session with a busy slot":
                assert g.admit([request(0, 8, 0, entry(2.0, 8))], 8) == 0, lib.zn_last_error(h)
        elif state == "ended":
            g.end()
        scratch = torch.zeros(4, 9, model.config.backbone.d_model, dtype=torch.bfloat16, device=DEV)
        st, ptr = eng.stream(), scratch.data_ptr()
        one = (_lib.zn_admit * 1)(request(1, 7, 0, entry(2.0, 8)))
        calls = {
            "zn_prefill": lambda: lib.zn_prefill(h, ptr, 7, st),
            "zn_prefill_rows": lambda: lib.zn_prefill_rows(h, ptr, 7, (C.c_int32 * 4)(7, 7, 7, 7), st),
            "zn_gen_set_rows": lambda: lib.zn_gen_set_rows(h, (_lib.zn_row_params * 2)(entry(2.0, 5), entry(2.0, 5)), 2),
            "zn_gen_set_prefix_rows": lambda: lib.zn_gen_set_prefix_rows(h, (C.c_int32 * 2)(0, 0), 2),
            "zn_gen_open_slots": lambda: lib.zn_gen_open_slots(h, 24),
            "zn_gen_admit": lambda: lib.zn_gen_admit(h, one, 1, ptr, 7, st),
            "zn_gen_retire": lambda: lib.zn_gen_retire(h, 0),
            "zn_gen_row_state": lambda: lib.zn_gen_row_state(h, None, None, st),
            "zn_sample_first": lambda: lib.zn_sample_first(h, st),
            "zn_decode_steps": lambda: lib.zn_decode_steps(h, 1, st),
            "zn_gen_bind_kv_fp8": lambda: lib.zn_gen_bind_kv_fp8(h, (C.c_void_p * n_layer)()),
            "zn_set_mlp_fp8": lambda: lib.zn_set_mlp_fp8(h, 0, None, None, None, None),
            "zn_set_mamba_fp8": lambda: lib.zn_set_mamba_fp8(h, 0, None, None, None, None),
            "zn_set_kv_fp8": lambda: lib.zn_set_kv_fp8(h, 1),
            "zn_set_kv_fp8_only": lambda: lib.zn_set_kv_fp8_only(h, 1),
        }
        for fn, states in REFUSED.items():
            if state in states:
                print("order: %s, %s | %d | %s" % (fn, state, calls[fn](), lib.zn_last_error(h).decode()), flush=True)
        if g is not None and state != "ended":
            g.end()
        del scratch


def set_rows_rules(model, eng):
    g = Gen(model, eng, 2, True, 32, 17, 1, 8)
    row = entry(2.0, 5)
    g.set_rows("set_rows: null", [], 2)
    g.set_rows("set_rows: 3 entries", [row, row, row])
    g.set_rows("set_rows: cfg_scale 1 with guidance", [row, entry(1.0, 5)])
    g.set_rows("set_rows: cfg_scale 1 twice with guidance", [entry(1.0, 5), entry(1.0, 5)])
    g.set_rows("set_rows: max_new_tokens 0", [entry(2.0, 0), row])
    g.set_rows("set_rows: max_new_tokens budget + 1", [row, entry(2.0, 9)])
    g.set_rows("set_rows: window 65", [entry(2.0, 5, window=65), row])
    g.set_rows("set_rows: window -1", [row, entry(2.0, 5, window=-1)])
    g.set_rows("set_rows: window before budget", [entry(2.0, 0, window=65), row])
    g.set_rows("set_rows: a pair with guidance", [pair_entry(0, 1), pair_entry(0, 1)])
    g.end()
    g = Gen(model, eng, 4, False, 32, 17, 1, 8)
    U = entry(1.0, 5)
    g.set_rows("set_rows: guided, no pair named", [U, entry(2.0, 6, 3.0), U, U])
    g.set_rows("set_rows: the partner is another request", [U, pair_entry(1, 3), U, U])
    g.set_rows("set_rows: the partner does not name the pair", [pair_entry(0, 1), U, U, U])
    g.set_rows("set_rows: the partner's penalty differs", [U, pair_entry(1, 3), U, pair_entry(1, 3, 6, 4.0)])
    g.set_rows("set_rows: the partner's budget differs", [U, pair_entry(1, 3), U, pair_entry(1, 3, 7)])
    g.set_rows("set_rows: a pair row out of range", [U, pair_entry(1, 4), U, U])
    g.set_rows("set_rows: a negative pair word", [U, entry(2.0, 6, 3.0, 2, -1), U, U])
    g.set_rows("set_rows: the same row twice", [U, pair_entry(1, 1), U, U])
    g.set_rows("set_rows: a pair of other rows", [U, pair_entry(2, 3), pair_entry(2, 3), pair_entry(2, 3)])
    g.set_rows("set_rows: a pair at cfg_scale 1", [entry(1.0, 5, 2.0, 1, 2), entry(1.0, 5, 2.0, 1, 2), U, U])
    g.end()


def prefix_rows_rules(model, eng):
    g = Gen(model, eng, 2, True, 32, 22, 6, 8)
    g.set_prefix("prefix_rows: null", [], 2)
    g.set_prefix("prefix_rows: 3 entries", [5, 2, 0])
    g.set_prefix("prefix_rows: -1", [5, -1])
    g.set_prefix("prefix_rows: p_call + 1", [6, 5])
    g.set_prefix("prefix_rows: none is the longest", [4, 2])
    g.end()


def prefill_rows_rules(model, eng):
    g = Gen(model, eng, 2, True, 25, 12, 1, 4)
    g.prefill_rows("prefill_rows: a pair out of lockstep", [9, 5, 9, 6])
    g.prefill_rows("prefill_rows: 0 positions", [9, 0, 9, 0])
    g.prefill_rows("prefill_rows: S + 1 positions", [9, 10, 9, 10])
    g.prefill_rows("prefill_rows: no row of S positions", [8, 5, 8, 5])
    g.end()
    g = Gen(model, eng, 1, True, 25, 12, 1, 4)
    g.prefill_rows("prefill_rows: one guided pair out of lockstep", [9, 5])
    g.end()


def session_rules(model, eng):
    lib, h = eng.lib, eng.h
    g = Gen(model, eng, 2, True, 48, 42, 1, 8)
    g.say("open_slots: slack -1", lib.zn_gen_open_slots(h, -1))
    g.end()
    g = Gen(model, eng, 2, True, 48, 42, 1, 8, lengths=3)
    g.say("open_slots: lengths not zero", lib.zn_gen_open_slots(h, 24))
    g.end()
    g = Gen(model, eng, 2, True, 48, 42, 1, 8)
    eng.call("zn_gen_open_slots", 24)
    p8 = entry(2.0, 8)
    g.say("admit: null", g.admit([], 7, n=1, null=True))
    g.say("admit: no request", g.admit([], 7))
    g.say("admit: 3 requests", g.admit([request(0, 7, 0, p8), request(1, 7, 0, p8), request(0, 7, 0, p8)], 7))
    g.say("admit: S 0", g.admit([request(0, 7, 0, p8)], 0))
    g.say("admit: S max_len + 1", g.admit([request(0, 7, 0, p8)], 49))
    eng.call("zn_all_stopped_begin", g.st)
    g.say("admit: a stop read-back pending", g.admit([request(0, 7, 0, p8)], 7))
    eng.call("zn_all_stopped_end", C.byref(C.c_int32(0)))
    g.say("admit: slot named twice", g.admit([request(0, 7, 1, entry(2.0, 6)), request(0, 6, 0, p8)], 7))
    g.say("admit: slot out of range", g.admit([request(2, 7, 1, entry(2.0, 6))], 7))
    g.say("admit: slot -1", g.admit([request(-1, 7, 1, entry(2.0, 6))], 7))
    g.say("admit: 0 positions", g.admit([request(0, 7, 0, p8), request(1, 0, 0, p8)], 7))
    g.say("admit: S + 1 positions", g.admit([request(1, 8, 0, p8)], 7))
    g.say("admit: prefix -1", g.admit([request(1, 7, -1, p8)], 7))
    g.say("admit: prefix row_len - 1", g.admit([request(1, 7, 6, p8)], 7))
    g.say("admit: 1 position has no prefix", g.admit([request(0, 7, 0, p8), request(1, 1, 0, p8)], 7))
    g.say("admit: window 65", g.admit([request(1, 7, 0, entry(2.0, 8, window=65))], 7))
    g.say("admit: window -1", g.admit([request(1, 7, 0, entry(2.0, 8, window=-1))], 7))
    g.say("admit: max_new_tokens 0", g.admit([request(1, 7, 0, entry(2.0, 0))], 7))
    g.say("admit: past max_len by one", g.admit([request(1, 9, 0, p8)], 9))
    g.say("admit: past the width by one", g.admit([request(1, 4, 0, entry(2.0, 10))], 4))
    g.say("admit: max_new_tokens INT32_MAX", g.admit([request(1, 4, 0, entry(2.0, INT_MAX))], 4))
    g.say("admit: cfg_scale 1 with guidance", g.admit([request(1, 6, 0, entry(1.0, 4))], 6))
    g.say("admit: a pair with guidance", g.admit([request(0, 7, 1, pair_entry(0, 1)), request(1, 7, 1, pair_entry(0, 1))], 7))
    g.say("admit: no request holds S", g.admit([request(0, 7, 0, p8)], 8))
    g.say("admit: the width passed by the prefix", g.admit([request(1, 8, 2, p8)], 8))
    # the slot script: admit, steps, retire, admit
    g.say("retire: slot out of range", lib.zn_gen_retire(h, 2))
    g.say("retire: slot -1", lib.zn_gen_retire(h, -1))
    g.say("retire: an idle slot", lib.zn_gen_retire(h, 1))
    assert g.admit([request(0, 8, 0, p8)], 8) == 0, lib.zn_last_error(h)
    g.say("admit: a busy slot", g.admit([request(0, 6, 0, p8)], 6))
    g.say("steps: past max_len by one", lib.zn_decode_steps(h, 41, g.st))
    eng.call("zn_decode_steps", 16, g.st)
    assert g.admit([request(1, 5, 0, p8)], 5) == 0, lib.zn_last_error(h)
    eng.call("zn_decode_steps", 8, g.st)
    g.say("steps: the longer slot decides", lib.zn_decode_steps(h, 17, g.st))
    eng.call("zn_gen_retire", 0)
    g.say("retire: retired already", lib.zn_gen_retire(h, 0))
    g.say("steps: the other slot past max_len by one", lib.zn_decode_steps(h, 36, g.st))
    g.end()
    g = Gen(model, eng, 4, False, 48, 42, 1, 8)
    eng.call("zn_gen_open_slots", 8)
    G, Uq = entry(2.0, 6), entry(1.0, 5)
    other = paired(entry(2.0, 6, seed=262), 2, 0)
    g.say("admit: guided, no pair named", g.admit([request(2, 7, 1, G), request(0, 7, 1, G)], 7))
    g.say("admit: the partner is missing", g.admit([request(2, 7, 1, paired(G, 2, 0)), request(1, 6, 0, Uq)], 7))
    g.say("admit: the partner is another request", g.admit([request(2, 7, 1, paired(G, 2, 0)), request(0, 7, 1, other)], 7))
    g.say("admit: the partner's row_len differs", g.admit([request(2, 7, 1, paired(G, 2, 0)), request(0, 6, 1, paired(G, 2, 0))], 7))
    g.say("admit: the partner's prefix_len differs", g.admit([request(2, 7, 1, paired(G, 2, 0)), request(0, 7, 0, paired(G, 2, 0))], 7))
    g.say("admit: a pair row out of range", g.admit([request(2, 7, 1, paired(G, 2, 4)), request(0, 7, 1, paired(G, 2, 4))], 7))
    g.say("admit: the same row twice", g.admit([request(2, 7, 1, paired(G, 2, 2)), request(0, 7, 1, paired(G, 2, 2))], 7))
    g.say("admit: a pair of other rows", g.admit([request(2, 7, 1, paired(G, 1, 0)), request(0, 7, 1, paired(G, 1, 0))], 7))
    g.say("admit: a pair at cfg_scale 1", g.admit([request(1, 6, 0, paired(Uq, 1, 3)), request(3, 6, 0, paired(Uq, 1, 3))], 6))
    g.end()


if __name__ == "__main__":
    model, _ = build_model(synth.TINY_CFG, 7, DEV)
    call_order(model, model._new_engine(4))
    eng = model._new_engine(4)
    set_rows_rules(model, eng)
    prefix_rows_rules(model, eng)
    prefill_rows_rules(model, eng)
    session_rules(model, eng)
    torch.cuda.synchronize()
