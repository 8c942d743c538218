"""The FP8 KV cache (Zonos.set_kv_cache("fp8")): the decode attention reading the one-byte codes against the same attention
reading the bf16 copy of the SAME rounded cache, at the Zonos-v0.1 dimensions with seeded synthetic weights, in one process, on one model
with the mode on.  The two sides differ in zn_debug_tune(ZN_TUNE_KV_FP8, .) alone - unset: the codes; 2: the bf16 cache - and alternate;
every figure is a median over the repetitions with their extremes beside it.  Nothing here compares against a figure from another file.

  launches  the decode attention of one layer (zn_op_attn_decode with a code cache bound) at 8, 16, 32 and 64 rows x 450, 900 and 2600 keys per
            row, per launch between HIP events, cycling through 26 caches as a decode step walks its 26 layers' (no launch finds the cache it
            reads warmer than a step would); K/V bytes per launch and what they amount to per second.
  steps     a guided, greedy decode step at 4, 8, 16 and 32 utterances (8 .. 64 rows) around 450 and 2600 keys of context: generations
            through the C ABI, each prefilled once and followed by ten blocks of 8 + 16 steps, alternately with the codes and with the bf16
            cache: the 8 capture the run graph again (the key drops it), the 16 (two runs of 8: the long graph) lie between HIP events; the
            first block of either side is not counted.  The context grows by 24 keys per block around the figure named; the alternation puts
            both sides at the same mean context.

    python tools/kvfp8bench.py [--reps 20] [--only launches|steps]

One JSON line per figure; everything is also written to profiles/kvfp8bench.txt."""
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
from zonos_amd.testing import build_model  # noqa: E402

DEV = "cuda:0"
N_CACHES = 26
BLOCK = 16          # measured steps per block: two runs of 8 (the long graph)
WARM = 8            # steps in front of them that capture the graph again


def spread(values):
    return dict(median=round(statistics.median(values), 3), min=round(min(values), 3), max=round(max(values), 3))


def launch_us(eng, rows, keys, reps, pool):
    """Per mode, the median microseconds of an attention launch within each repetition (one pass over the caches): reps values."""
    zc, st = eng.zc, _lib.stream_ptr()
    hd = zc.d_model // zc.n_heads
    max_len = (keys + 511) // 512 * 512
    n = rows * max_len * 2 * zc.n_heads_kv * hd
    pq, pdq = pool
    g = torch.Generator(device=DEV).manual_seed(rows * 10007 + keys)
    caches = []
    for _ in range(N_CACHES):
        idx = torch.randint(0, pq.numel(), (n,), generator=g, device=DEV)
        caches.append((pdq[idx], pq[idx]))                  # the bf16 cache holds exactly the dequantised codes, as the appends leave it
    del idx
    q = torch.randn(rows, zc.n_heads * hd, generator=g, device=DEV).to(torch.bfloat16)
    out = torch.empty_like(q)
    lengths = torch.full((rows,), keys - 1, dtype=torch.int32, device=DEV)
    big = torch.empty(8192, 8192, dtype=torch.bfloat16, device=DEV).normal_()
    times = {"fp8": [], "bf16": []}
    for rep in range(reps + 2):                             # two warm-up repetitions
        for mode, tune in (("fp8", 1), ("bf16", 2)):
            eng.call("zn_debug_tune", _lib.ZN_TUNE_KV_FP8, tune)
            for _ in range(8):                              # the launches queue behind matrix products: the device never waits for the host between two events
                big @ big
            evs = []
            for kv, codes in caches:
                eng.call("zn_op_bind_kv_fp8", codes.data_ptr())
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng.call("zn_op_attn_decode", q.data_ptr(), kv.data_ptr(), max_len, lengths.data_ptr(), None, out.data_ptr(), rows, st)
                e1.record()
                evs.append((e0, e1))
            if rep >= 2:
                times[mode].append(evs)
    torch.cuda.synchronize()
    eng.call("zn_op_bind_kv_fp8", None)
    eng.call("zn_debug_tune", _lib.ZN_TUNE_KV_FP8, 1)
    return {m: [statistics.median(a.elapsed_time(b) * 1e3 for a, b in evs) for evs in t] for m, t in times.items()}, max_len


def step_ms(model, eng, batch, keys, reps):
    """Per mode, milliseconds per decode step of each measured block: reps values, four per generation."""
    cfg, nq = model.config.backbone, model.config.codebook_dimension
    R, st = 2 * batch, _lib.stream_ptr()
    per_gen = 4                                              # measured blocks per mode and generation
    n_blocks = 2 * per_gen + 2                               # ... behind one unmeasured block per mode
    steps = n_blocks * (WARM + BLOCK)
    L = max(8, keys - steps // 2)                            # the blocks' contexts centre on `keys`
    t_total = steps + nq + 2
    times = {"fp8": [], "bf16": []}
    path = -1
    g = torch.Generator(device=DEV).manual_seed(900 + batch)
    for gen in range((reps + per_gen - 1) // per_gen):
        ip = model.setup_cache(batch_size=R, max_seqlen=L + 1 + t_total)
        delayed = code_rows([None] * batch, [steps + 1] * batch, t_total, nq, model.masked_token_id, DEV)
        kv_ptrs = (C.c_void_p * cfg.n_layer)(*[ip.key_value_memory_dict[i][0].data_ptr() for i in range(cfg.n_layer)])
        sp = _lib.zn_sampling()                              # temperature 0: greedy
        eng.call("zn_debug_eos_bias", float("-inf"))
        eng.call("zn_debug_tune", _lib.ZN_TUNE_KV_FP8, 1)
        eng.call("zn_gen_begin", batch, kv_ptrs, ip.max_seqlen, ip.lengths_per_sample.data_ptr(), delayed.data_ptr(), t_total, 1, steps + 1, 2.0, C.byref(sp), st)
        try:
            kept = model._bind_kv_codes(eng, R, ip.max_seqlen)
            assert kept is not None, "the mode is not in effect"
            cond = torch.randn(R, L, cfg.d_model, generator=g, device=DEV).to(torch.bfloat16)
            hidden = torch.cat([cond, model.embed_codes(delayed[..., :1], _eng=eng).repeat(2, 1, 1)], dim=1).contiguous()
            eng.call("zn_prefill", hidden.data_ptr(), hidden.shape[1], st)
            eng.call("zn_sample_first", st)
            evs = []
            for blk in range(n_blocks):
                mode, tune = (("fp8", 1), ("bf16", 2))[blk % 2]
                torch.cuda.synchronize()                                  # the key drops the captured graphs: none may still be queued
                eng.call("zn_debug_tune", _lib.ZN_TUNE_KV_FP8, tune)
                eng.call("zn_decode_steps", WARM, st)                     # captures the run graph again
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng.call("zn_decode_steps", BLOCK, st)
                e1.record()
                if blk >= 2:
                    evs.append((mode, e0, e1))
            torch.cuda.synchronize()
            for mode, e0, e1 in evs:
                times[mode].append(e0.elapsed_time(e1) / BLOCK)
            path = int(eng.lib.zn_decode_path_detail(eng.h))
        finally:
            torch.cuda.synchronize()
            eng.call("zn_gen_end")
            eng.call("zn_debug_tune", _lib.ZN_TUNE_KV_FP8, 1)
            eng.call("zn_debug_eos_bias", 0.0)
        del kept, ip, hidden, cond
    return {m: t[:reps] for m, t in times.items()}, L + 1 + steps // 2, path


def verdict(fp8, bf16):
    """Faster beyond the spread of the repetitions: the slowest FP8 repetition beats the fastest bf16 one, or at least the medians differ by more than
    either side's own range."""
    f, b = spread(fp8), spread(bf16)
    clear = f["median"] < b["median"] and (b["median"] - f["median"]) > max(f["max"] - f["min"], b["max"] - b["min"]) / 2
    return dict(ratio_bf16_over_fp8=round(b["median"] / f["median"], 3), fp8_faster_beyond_spread=bool(clear))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=("launches", "steps"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kvfp8bench.txt"))
    args = ap.parse_args()
    lines = []

    def emit(**kw):
        s = json.dumps(kw)
        print(s, flush=True)
        lines.append(s)
    model, _ = build_model(synth.FULL_CFG, 1234, DEV)
    model.set_kv_cache("fp8")
    eng = model.engine(32)
    zc = eng.zc
    hd = zc.d_model // zc.n_heads
    if args.only != "steps":
        x = torch.from_numpy(synth.normal(64, "kvfp8bench.pool", (1 << 16,))).to(torch.bfloat16)
        pool = tuple(t.to(DEV) for t in kv_round_e4m3(x))
        for rows in (8, 16, 32, 64):
            for keys in (450, 900, 2600):
                t, max_len = launch_us(eng, rows, keys, args.reps, pool)
                elems = rows * keys * 2 * zc.n_heads_kv * hd
                emit(figure="attention_launch", rows=rows, keys=keys, max_len=max_len, launches_per_rep=N_CACHES, reps=args.reps, us_fp8=spread(t["fp8"]), us_bf16=spread(t["bf16"]),
                     kv_bytes_fp8=elems, kv_bytes_bf16=2 * elems, tb_per_s_fp8=round(elems / statistics.median(t["fp8"]) / 1e6, 3),
                     tb_per_s_bf16=round(2 * elems / statistics.median(t["bf16"]) / 1e6, 3), **verdict(t["fp8"], t["bf16"]))
                torch.cuda.empty_cache()
    if args.only != "launches":
        for batch in (4, 8, 16, 32):
            for keys in (450, 2600):
                t, ctx, path = step_ms(model, eng, batch, keys, args.reps)
                emit(figure="decode_step", utterances=batch, rows=2 * batch, mean_keys=ctx, steps_per_block=BLOCK, reps=args.reps, decode_path_detail=path, ms_fp8=spread(t["fp8"]),
                     ms_bf16=spread(t["bf16"]), **verdict(t["fp8"], t["bf16"]))
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("python tools/kvfp8bench.py --reps %d%s\n" % (args.reps, f" --only {args.only}" if args.only else "") + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
