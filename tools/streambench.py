"""Zonos.stream() against generate() + autoencoder.decode() at the Zonos-v0.1 dimensions, alternated on the same seed.

A 10 s clip (861 frames, greedy, EOS suppressed as bench.py does) with the full-size synthetic DAC.  Per repetition: the stream's time
to its first chunk and to its first audio (host clock after a synchronise, to the yield), its total wall time and chunk count; the
generate() + decode() wall time; and whether codes and waveform are identical.  One JSON line per repetition, then a summary line.

    python tools/streambench.py [--frames 861] [--chunk 16] [--reps 5] [--warmup 1]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zonos_amd import synth  # noqa: E402
from zonos_amd.autoencoder import DACAutoencoder  # noqa: E402
from zonos_amd.testing import build_model  # noqa: E402

L_C = 24


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=861)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    dev = "cuda:0"
    cfg, seed = synth.FULL_CFG, 1234
    dac = DACAutoencoder(synth.dac_state_dict(4321, encoder=False), device=dev)
    model, _ = build_model(cfg, seed, dev, dac=dac)
    c = synth.conditioning(seed, "cond", 1, L_C, cfg["d_model"]).to(dev)
    cond = torch.cat([c, c], 0)
    kw = dict(max_new_tokens=args.frames, sampling_params={"temperature": 0.0}, seed=7)
    eng = model.engine(1)
    eng.call("zn_debug_eos_bias", float("-inf"))

    def batch():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        codes = model.generate(cond, **kw)
        wav = model.autoencoder.decode(codes)
        torch.cuda.synchronize()
        return codes, wav, time.perf_counter() - t0

    def stream():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first = first_audio = None
        chunks = []
        for ch in model.stream(cond, chunk_frames=args.chunk, **kw):
            now = time.perf_counter() - t0
            first = now if first is None else first
            if first_audio is None and ch.wav.shape[2]:
                first_audio = now
            chunks.append(ch)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        return torch.cat([x.codes for x in chunks], 2), torch.cat([x.wav for x in chunks], 2), first, first_audio, total, len(chunks)

    rows = []
    for r in range(args.warmup + args.reps):
        codes, wav, t_batch = batch()
        scodes, swav, first, first_audio, t_stream, n = stream()
        row = dict(rep=r, warmup=r < args.warmup, frames=int(codes.shape[2]), first_chunk_ms=round(first * 1e3, 2),
                   first_audio_ms=round(first_audio * 1e3, 2), stream_total_ms=round(t_stream * 1e3, 2),
                   generate_decode_ms=round(t_batch * 1e3, 2), chunks=n,
                   identical=bool(torch.equal(codes, scodes) and torch.equal(wav, swav)), decode_path=eng.lib.zn_decode_path_detail(eng.h))
        print(json.dumps(row), flush=True)
        if r >= args.warmup:
            rows.append(row)
    med = lambda k: round(statistics.median(x[k] for x in rows), 2)  # noqa: E731
    summary = dict(summary=True, frames=args.frames, chunk_frames=args.chunk, reps=len(rows), first_chunk_ms=med("first_chunk_ms"),
                   first_audio_ms=med("first_audio_ms"), stream_total_ms=med("stream_total_ms"), generate_decode_ms=med("generate_decode_ms"),
                   stream_over_batch=round(med("stream_total_ms") / med("generate_decode_ms"), 4), chunks=rows[0]["chunks"],
                   identical=all(x["identical"] for x in rows), handoff=model.handoff_counters())
    print(json.dumps(summary), flush=True)
    eng.call("zn_debug_eos_bias", 0.0)
    return 0 if summary["identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
