"""Weight-only FP8 for the Mamba2 in_proj / out_proj (Zonos.quantize_mamba_fp8) against the bf16 stream of the SAME weights, at the
Zonos-v0.1-hybrid dimensions (synth.HYBRID_FULL_CFG: 46 layers, 42 of them Mamba2) with seeded synthetic weights.  One process, one quantised model; the
baseline is the same model and handle under zn_debug_tune(ZN_TUNE_MAMBA_FP8, 2), where every launch reads the dequantised bf16 copy - the same bits out.

  kernels   zn_bench_kernel(which = 7: in_proj with its conv-window epilogue, 8: out_proj) at 8, 16, 18, 32, 48 and 64 rows, cycling through the 42 Mamba2
            layers' weights: microseconds per projection over all its launches, stream on / off alternated per repetition; median, min and max.
  steps     a decode step at 4, 8, 9, 16, 24 and 32 guided utterances (8 .. 64 rows), greedy, EOS suppressed: wall time of generate() at two lengths, their
            difference per step - stream on / off alternated per repetition; median, min and max.
  counters  the handle's hand-off / timeout counters (zn_get_counters).  A hand-off timeout makes the tool fail.

    python tools/hybridfp8bench.py [--reps 20]

One JSON line per figure; everything is also written to profiles/hybridfp8bench.txt.  The verdict lines say, per row count, whether the stream beats bf16 by
more than the spread of the repetitions (max - min of either): that is what plan_linear's w8k decision (zn_linear_plan.h) should follow."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zonos_amd import _lib, synth  # noqa: E402
from zonos_amd.testing import build_model  # noqa: E402

DEV = "cuda:0"
GREEDY = dict(temperature=0.0)
MODES = {1: "fp8", 2: "bf16"}                      # values of ZN_TUNE_MAMBA_FP8
OPS = {7: "mamba_in_proj", 8: "mamba_out_proj"}    # zn_bench_kernel's `which`


def generate(model, batch, steps, seed=500):
    d = model.config.backbone.d_model
    cond = torch.cat([synth.conditioning(seed + i, "hybridfp8bench.cond", 2, 24, d) for i in range(batch)], 0)
    cond = torch.cat([cond[0::2], cond[1::2]], 0).to(DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.generate(cond, max_new_tokens=steps, cfg_scale=2.0, batch_size=batch, sampling_params=GREEDY)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(v):
    return statistics.median(v), min(v), max(v)


def kernel_us(eng, which, rows, reps, iters):
    """us per projection (all its launches) with the stream on and off, alternated per repetition: {mode: (median, min, max)}."""
    ms, by = C.c_float(0), C.c_double(0)
    per = {m: [] for m in MODES}
    st = _lib.stream_ptr()
    for rep in range(reps + 1):                          # repetition 0 warms up
        for mode in MODES:
            eng.call("zn_debug_tune", _lib.ZN_TUNE_MAMBA_FP8, mode)
            eng.call("zn_bench_kernel", which, rows, iters, C.byref(ms), C.byref(by), st)
            if rep:
                per[mode].append(ms.value * 1e3)
    return {m: stats(v) for m, v in per.items()}, by.value


def step_ms(model, eng, batch, reps, short=24, long=88):
    """ms per decode step with the stream on and off, alternated per repetition: {mode: (median, min, max)}."""
    per = {m: [] for m in MODES}
    for mode in MODES:                                   # warm-up: graphs of both launch lists
        eng.call("zn_debug_tune", _lib.ZN_TUNE_MAMBA_FP8, mode)
        generate(model, batch, short)
        generate(model, batch, long)
    for _ in range(reps):
        for mode in MODES:
            eng.call("zn_debug_tune", _lib.ZN_TUNE_MAMBA_FP8, mode)
            a, b = generate(model, batch, short), generate(model, batch, long)
            per[mode].append((b - a) / (long - short) * 1e3)
    return {m: stats(v) for m, v in per.items()}


def verdict(res):
    """Whether the stream (mode 1) beats bf16 (mode 2) by more than the spread of the repetitions; the spread."""
    spread = max(res[m][2] - res[m][1] for m in MODES)
    return bool(res[2][0] - res[1][0] > spread), spread


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hybridfp8bench.txt"))
    args = ap.parse_args()
    lines = []

    def emit(**kw):
        s = json.dumps(kw)
        print(s, flush=True)
        lines.append(s)
    model, _ = build_model(synth.HYBRID_FULL_CFG, 1234, DEV)
    model.quantize_mamba_fp8()
    eng = model.engine(32)
    eng.call("zn_debug_eos_bias", float("-inf"))
    n_mamba = sum(1 for blk in model.backbone.layers if blk.is_mamba)
    emit(figure="model", layers=len(model.backbone.layers), mamba_layers=n_mamba, mamba_weights=model.mamba_weights,
         reads_fp8={rows: eng.mamba_fp8_plan(rows) for rows in (2, 4, 5, 8, 16, 18, 32, 48, 64)}, rows_per_weight_pass={rows: eng.hybrid_rows_plan(rows) for rows in (8, 16, 18, 32, 48, 64)})
    for which, op in OPS.items():
        for rows in (8, 16, 18, 32, 48, 64):
            res, nbytes = kernel_us(eng, which, rows, args.reps, 2 * n_mamba)
            for mode, (med, lo, hi) in res.items():
                eng.call("zn_debug_tune", _lib.ZN_TUNE_MAMBA_FP8, mode)
                reads = eng.mamba_fp8_plan(rows)[which - 7]
                stream_bytes = nbytes / 2 if reads else nbytes
                emit(figure="kernel", op=op, rows=rows, stream=MODES[mode], reads_fp8=reads, rows_per_weight_pass=eng.hybrid_rows_plan(rows)[op], us_per_projection_median=round(med, 2),
                     min=round(lo, 2), max=round(hi, 2), reps=args.reps, stream_bytes=stream_bytes, tb_per_s=round(stream_bytes / (med * 1e-6) / 1e12, 3))
            faster, spread = verdict(res)
            emit(figure="kernel.verdict", op=op, rows=rows, fp8_over_bf16=round(res[1][0] / res[2][0], 4), spread_us=round(spread, 2), fp8_faster_beyond_spread=faster)
    for batch in (4, 8, 9, 16, 24, 32):
        res = step_ms(model, eng, batch, args.reps)
        for mode, (med, lo, hi) in res.items():
            eng.call("zn_debug_tune", _lib.ZN_TUNE_MAMBA_FP8, mode)
            emit(figure="step", utterances=batch, rows=2 * batch, stream=MODES[mode], reads_fp8=eng.mamba_fp8_plan(2 * batch), ms_per_step_median=round(med, 4), min=round(lo, 4),
                 max=round(hi, 4), reps=args.reps, audio_s_per_s=round(batch / 86 / (med * 1e-3), 1))
        faster, spread = verdict(res)
        emit(figure="step.verdict", utterances=batch, rows=2 * batch, fp8_over_bf16=round(res[1][0] / res[2][0], 4), saved_ms=round(res[2][0] - res[1][0], 4), spread_ms=round(spread, 4),
             fp8_faster_beyond_spread=faster)
    eng.call("zn_debug_tune", _lib.ZN_TUNE_MAMBA_FP8, 1)
    counters = model.handoff_counters()
    emit(figure="counters", **counters)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("python tools/hybridfp8bench.py --reps %d\n" % args.reps + "\n".join(lines) + "\n")
    bad = counters.get("repeated_generations", 0) + sum(v.get("handoff_timeouts", 0) + v.get("demoted", 0) for v in counters.values() if isinstance(v, dict))
    if bad:
        print("hand-off timeouts or demotions were counted: FAIL", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
