"""The codes-only FP8 KV cache (Zonos.set_kv_cache("fp8-only")) against the two-cache mode "fp8" (4.1k), at the Zonos-v0.1
dimensions with seeded synthetic weights, in one process, on one model and one engine.  The two sides differ in zn_set_kv_fp8_only alone, set
between generations, and alternate; every figure is a median over the repetitions with their extremes beside it.  Nothing here compares
against a figure from another file.  The mode is chosen for memory - no speed bar is set: the ratios say what it costs or gains in time.

  bytes      the KV bytes a session of 64 rows x 2600 and x 6144 positions allocates per mode (Zonos._kv_buffers, the helper generate() and serve()
             use; torch's allocator before and after), beside Zonos.kv_cache_bytes.
  launches   the prefill attention of one layer over 16 rows x 200 and x 2600 positions: zn_op_attn_prefill_rows_fp8 on the codes against
             zn_op_attn_prefill_rows on the dequantised bf16 cache, per launch between HIP events, cycling through 4 caches.
  prefill    zn_prefill of 16 rows x 200 positions (8 guided utterances), and one admission of 8 guided requests x 200 positions into a serving
             session of 8 slots (zn_gen_admit: the prefill on the scratch cache, then the copy of the rows), each in a generation of its own.
  steps      a guided, greedy decode step at 8 and 32 utterances (16 and 64 rows) around 450 and 2600 keys of context: generations through the C
             ABI, each prefilled once and followed by five blocks of 8 + 16 steps (the 8 capture the run graph, the 16 lie between HIP events; the
             first block is not counted); generations of the two modes alternate.

    python tools/kvfp8onlybench.py [--reps 20] [--only bytes|launches|prefill|steps]

One JSON line per figure; everything is also written to profiles/kvfp8onlybench.txt."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zonos_amd import _lib, synth  # noqa: E402
from zonos_amd.quant import kv_round_e4m3  # noqa: E402
from zonos_amd.rows import code_rows  # noqa: E402
from zonos_amd.serving import serve_slack  # noqa: E402
from zonos_amd.testing import build_model  # noqa: E402

DEV = "cuda:0"
MODES = ("fp8-only", "fp8")
N_CACHES = 4
BLOCK, WARM, PER_GEN = 16, 8, 4          # measured steps per block, steps in front of them, measured blocks per generation


def spread(values):
    return dict(median=round(statistics.median(values), 3), min=round(min(values), 3), max=round(max(values), 3))


def verdict(only, both):
    """ratio > 1: "fp8-only" is faster.  Beyond the spread: the medians differ by more than half of either side's own range."""
    o, b = spread(only), spread(both)
    gap = max(o["max"] - o["min"], b["max"] - b["min"]) / 2
    return dict(ratio_fp8_over_fp8_only=round(b["median"] / o["median"], 3), fp8_only_faster_beyond_spread=bool(b["median"] - o["median"] > gap),
                fp8_only_slower_beyond_spread=bool(o["median"] - b["median"] > gap))


def set_mode(eng, mode):
    eng.call("zn_set_kv_fp8_only", 1 if mode == "fp8-only" else 0)


def session_bytes(model, eng, rows, positions):
    out = {}
    for mode in MODES:
        set_mode(eng, mode)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated(DEV)
        bufs = model._kv_buffers(eng, rows, positions)
        out[mode] = torch.cuda.memory_allocated(DEV) - before         # (the int32 lengths array of the generation included: one allocator block)
        del bufs
    set_mode(eng, "fp8-only")
    return out


def attn_us(eng, rows, S, reps, pool):
    """Per form, the median microseconds of a prefill attention launch within each repetition (one pass over the caches): reps values."""
    zc, st = eng.zc, _lib.stream_ptr()
    hd = zc.d_model // zc.n_heads
    max_len = (S + 7) // 8 * 8
    n = rows * max_len * 2 * zc.n_heads_kv * hd
    pq, pdq = pool
    g = torch.Generator(device=DEV).manual_seed(rows * 10007 + S)
    caches = []
    for _ in range(N_CACHES):
        idx = torch.randint(0, pq.numel(), (n,), generator=g, device=DEV)
        caches.append((pdq[idx], pq[idx]))                  # the bf16 cache holds exactly the dequantised codes
    del idx
    q = torch.randn(rows, S, zc.n_heads * hd, generator=g, device=DEV).to(torch.bfloat16)
    out = torch.empty_like(q)
    big = torch.empty(8192, 8192, dtype=torch.bfloat16, device=DEV).normal_()
    times = {"codes": [], "bf16": []}
    for rep in range(reps + 2):                             # two warm-up repetitions
        for form in ("codes", "bf16"):
            for _ in range(8):                              # the launches queue behind matrix products: the device never waits for the host between two events
                big @ big
            evs = []
            for kv, codes in caches:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if form == "codes":
                    eng.call("zn_op_attn_prefill_rows_fp8", q.data_ptr(), codes.data_ptr(), max_len, out.data_ptr(), S, rows, 0, None, st)
                else:
                    eng.call("zn_op_attn_prefill_rows", q.data_ptr(), kv.data_ptr(), max_len, out.data_ptr(), S, rows, 0, None, st)
                e1.record()
                evs.append((e0, e1))
            if rep >= 2:
                times[form].append(evs)
    torch.cuda.synchronize()
    return {m: [statistics.median(a.elapsed_time(b) * 1e3 for a, b in evs) for evs in t] for m, t in times.items()}


class Generation:
    """zn_gen_begin .. zn_gen_end of `batch` guided utterances with the KV buffers of the engine's current mode."""

    def __init__(self, model, eng, batch, max_len, t_total, budget, session=False):
        self.model, self.eng, self.st = model, eng, _lib.stream_ptr()
        nq = model.config.codebook_dimension
        self.bufs = model._kv_buffers(eng, 2 * batch, max_len)
        if session:
            self.delayed = torch.full((batch, nq, t_total), model.masked_token_id, dtype=torch.int32, device=DEV)
        else:
            self.delayed = code_rows([None] * batch, [budget] * batch, t_total, nq, model.masked_token_id, DEV)
        self.sp = _lib.zn_sampling()                         # temperature 0: greedy
        eng.call("zn_debug_eos_bias", float("-inf"))
        ip = self.bufs.ip
        eng.call("zn_gen_begin", batch, self.bufs.kv_ptrs, ip.max_seqlen, ip.lengths_per_sample.data_ptr(), self.delayed.data_ptr(), t_total, 1, budget, 2.0,
                 C.byref(self.sp), self.st)

    def __enter__(self):
        self.model._bind_kv_buffers(self.eng, self.bufs)
        return self

    def __exit__(self, *a):
        torch.cuda.synchronize()
        self.eng.call("zn_gen_end")
        self.eng.call("zn_debug_eos_bias", 0.0)


def prefill_ms(model, eng, batch, S, reps, admission):
    """Per mode, milliseconds of zn_prefill (admission False) or zn_gen_admit (True) of 2 * batch rows x S positions: one generation each."""
    cfg, nq = model.config.backbone, model.config.codebook_dimension
    R, st = 2 * batch, _lib.stream_ptr()
    slack, budget = serve_slack(8), 8
    width = budget + nq + slack
    max_len = S - 1 + width
    g = torch.Generator(device=DEV).manual_seed(500 + S)
    hidden = torch.randn(R, S, cfg.d_model, generator=g, device=DEV).to(torch.bfloat16)
    times = {m: [] for m in MODES}
    for rep in range(reps + 1):                             # one warm-up repetition (workspaces, the scratch cache)
        for mode in MODES:
            set_mode(eng, mode)
            with Generation(model, eng, batch, max_len, width, budget, session=admission) as gen:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if admission:
                    eng.call("zn_gen_open_slots", slack)
                    adm = (_lib.zn_admit * batch)()
                    for j in range(batch):
                        gen.delayed[j].copy_(code_rows([None], [budget], width, nq, model.masked_token_id, DEV)[0])
                        adm[j].slot, adm[j].row_len, adm[j].prefix_len = j, S, 0
                        adm[j].params.sp, adm[j].params.cfg_scale, adm[j].params.max_new_tokens = _lib.zn_sampling(), 2.0, budget
                    torch.cuda.synchronize()
                    e0.record()
                    eng.call("zn_gen_admit", adm, batch, hidden.data_ptr(), S, st)
                else:
                    torch.cuda.synchronize()
                    e0.record()
                    eng.call("zn_prefill", hidden.data_ptr(), S, st)
                e1.record()
                torch.cuda.synchronize()
                if rep >= 1:
                    times[mode].append(e0.elapsed_time(e1))
    return times


def step_ms(model, eng, batch, keys, reps):
    """Per mode, milliseconds per decode step of each measured block: reps values, PER_GEN per generation."""
    cfg, nq = model.config.backbone, model.config.codebook_dimension
    R, st = 2 * batch, _lib.stream_ptr()
    n_blocks = PER_GEN + 1                                   # ... behind one unmeasured block
    steps = n_blocks * (WARM + BLOCK)
    L = max(8, keys - steps // 2)                            # the blocks' contexts centre on `keys`
    t_total = steps + nq + 2
    times = {m: [] for m in MODES}
    path = -1
    g = torch.Generator(device=DEV).manual_seed(900 + batch)
    cond = torch.randn(R, L, cfg.d_model, generator=g, device=DEV).to(torch.bfloat16)
    for gen_i in range((reps + PER_GEN - 1) // PER_GEN):
        for mode in MODES:
            set_mode(eng, mode)
            with Generation(model, eng, batch, L + 1 + t_total, t_total, steps + 1) as gen:
                hidden = torch.cat([cond, model.embed_codes(gen.delayed[..., :1], _eng=eng).repeat(2, 1, 1)], dim=1).contiguous()
                eng.call("zn_prefill", hidden.data_ptr(), hidden.shape[1], st)
                eng.call("zn_sample_first", st)
                evs = []
                for blk in range(n_blocks):
                    eng.call("zn_decode_steps", WARM, st)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    eng.call("zn_decode_steps", BLOCK, st)
                    e1.record()
                    if blk >= 1:
                        evs.append((e0, e1))
                torch.cuda.synchronize()
                times[mode] += [a.elapsed_time(b) / BLOCK for a, b in evs]
                path = int(eng.lib.zn_decode_path_detail(eng.h))
                del hidden
    return {m: t[:reps] for m, t in times.items()}, L + 1 + steps // 2, path


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=("bytes", "launches", "prefill", "steps"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kvfp8onlybench.txt"))
    args = ap.parse_args()
    lines = []

    def emit(**kw):
        s = json.dumps(kw)
        print(s, flush=True)
        lines.append(s)
    want = lambda part: args.only in (None, part)
    model, _ = build_model(synth.FULL_CFG, 1234, DEV)
    model.set_kv_cache("fp8-only")
    eng = model.engine(32)                                   # (max_rows 64)
    try:
        if want("bytes"):
            for positions in (2600, 6144):
                got = session_bytes(model, eng, 64, positions)
                said = {}
                for mode in ("bf16",) + MODES:
                    model.kv_cache = mode                    # (the attribute alone: the engine stays)
                    b = model.kv_cache_bytes(64, positions)
                    said[mode] = b["bf16"] + b["codes"]
                model.kv_cache = "fp8-only"
                emit(figure="kv_bytes", rows=64, positions=positions, allocated={m: got[m] for m in MODES}, kv_cache_bytes=said,
                     fp8_only_over_fp8=round(got["fp8-only"] / got["fp8"], 4), fp8_only_over_bf16=round(said["fp8-only"] / said["bf16"], 4))
                torch.cuda.empty_cache()
        if want("launches"):
            x = torch.from_numpy(synth.normal(64, "kvfp8onlybench.pool", (1 << 16,))).to(torch.bfloat16)
            pool = tuple(t.to(DEV) for t in kv_round_e4m3(x))
            for S in (200, 2600):
                t = attn_us(eng, 16, S, args.reps, pool)
                o, b = spread(t["codes"]), spread(t["bf16"])
                gap = max(o["max"] - o["min"], b["max"] - b["min"]) / 2
                emit(figure="prefill_attention_launch", rows=16, positions=S, launches_per_rep=N_CACHES, reps=args.reps, us_codes=o, us_bf16=b,
                     ratio_bf16_over_codes=round(b["median"] / o["median"], 3), codes_faster_beyond_spread=bool(b["median"] - o["median"] > gap),
                     codes_slower_beyond_spread=bool(o["median"] - b["median"] > gap))
                torch.cuda.empty_cache()
        if want("prefill"):
            for admission in (False, True):
                t = prefill_ms(model, eng, 8, 200, args.reps, admission)
                emit(figure="serve_admission" if admission else "prefill", rows=16, positions=200, reps=args.reps, ms_fp8_only=spread(t["fp8-only"]), ms_fp8=spread(t["fp8"]),
                     **verdict(t["fp8-only"], t["fp8"]))
                torch.cuda.empty_cache()
        if want("steps"):
            for batch in (8, 32):
                for keys in (450, 2600):
                    t, ctx, path = step_ms(model, eng, batch, keys, args.reps)
                    emit(figure="decode_step", utterances=batch, rows=2 * batch, mean_keys=ctx, steps_per_block=BLOCK, reps=args.reps, decode_path_detail=path,
                         ms_fp8_only=spread(t["fp8-only"]), ms_fp8=spread(t["fp8"]), **verdict(t["fp8-only"], t["fp8"]))
                    torch.cuda.empty_cache()
    finally:
        set_mode(eng, "fp8-only")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("python tools/kvfp8onlybench.py --reps %d%s\n" % (args.reps, f" --only {args.only}" if args.only else "") + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
