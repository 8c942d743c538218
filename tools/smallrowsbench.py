"""The GEMV of 1..4 decode rows reading the FP8 streams (ZN_TUNE_FP8_SMALL_ROWS, Zonos.set_fp8_small_rows) against the bf16 GEMV of the SAME
quantised model in the same run (the key off), at the Zonos-v0.1 and Zonos-v0.1-hybrid dimensions with seeded synthetic weights.  The same bits out either way.

  kernels   zn_bench_kernel at 1, 2, 3 and 4 rows, cycling through the layers' weights (every launch streams from HBM): the transformer's fc1 (which = 0) and
            fc2 (1), the Mamba2 in_proj (7) and out_proj (8: with the gated-norm prologue on the checkpoint's one norm group, and without it on a model of two
            norm groups).  Microseconds per launch with the key unset (bf16), = 2 (the stream, the next unit requested ahead) and = 3 (a ring of two units ahead), alternated
            per repetition; median, min and max.
  steps     ms per decode step, greedy, EOS suppressed - wall time of a call at two lengths, their difference per step - key off / on alternated per
            repetition: the 46-layer hybrid stack at 1 and 2 guided utterances and at 1 and 3 unguided; the 26-layer transformer at 2 guided utterances and in
            a one-slot guided serve() session.
  observed  the transformer at batch 1: the launches path (ZN_TUNE_PERSISTENT = 2) reading the stream against the whole-step kernel on the bf16 copy.  No
            default follows from this figure.
  counters  the handles' hand-off / timeout counters.  A hand-off timeout makes the tool fail.

    python tools/smallrowsbench.py [--reps 20]

One JSON line per figure; everything is also written to profiles/smallrowsbench.txt.  The verdict lines say whether the stream beats bf16 by more than the
spread of the repetitions (max - min of either): a (projection, row count) keeps the stream in plan_linear (zn_linear_plan.h) only where it does."""
import argparse
import ctypes as C
import gc
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zonos_amd import _lib, synth  # noqa: E402
from zonos_amd.model import GenRequest  # noqa: E402
from zonos_amd.testing import build_model  # noqa: E402

DEV = "cuda:0"
GREEDY = dict(temperature=0.0)
KEY = _lib.ZN_TUNE_FP8_SMALL_ROWS
MODES = {1: "bf16", 2: "fp8, one unit ahead", 3: "fp8, two units ahead"}          # values of the key
ROWS = (1, 2, 3, 4)
SHORT, LONG = 24, 88
ITERS = 32                                          # launches per repetition and layer: a repetition runs for some 10 ms, so that one interruption does not set the spread


def stats(v):
    return statistics.median(v), min(v), max(v)


def kernel_us(eng, which, rows, reps, iters):
    """us per launch under each value of the key, alternated per repetition: {mode: (median, min, max)}."""
    ms, by = C.c_float(0), C.c_double(0)
    per = {m: [] for m in MODES}
    st = _lib.stream_ptr()
    for rep in range(reps + 1):                          # repetition 0 warms up
        for mode in MODES:
            eng.call("zn_debug_tune", KEY, mode)
            eng.call("zn_bench_kernel", which, rows, iters, C.byref(ms), C.byref(by), st)
            if rep:
                per[mode].append(ms.value * 1e3)
    eng.call("zn_debug_tune", KEY, 1)
    return {m: stats(v) for m, v in per.items()}, by.value


def verdict(res, on=2):
    """Whether the stream (key = on) beats bf16 (key = 1) by more than the spread of the repetitions; the spread."""
    spread = max(res[m][2] - res[m][1] for m in (1, on))
    return bool(res[1][0] - res[on][0] > spread), spread


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def gen_call(model, batch, guided):
    d = model.config.backbone.d_model
    if guided:
        cond = torch.cat([synth.conditioning(500 + i, "smallrowsbench.cond", 2, 24, d) for i in range(batch)], 0)
        cond = torch.cat([cond[0::2], cond[1::2]], 0).to(DEV)
    else:
        cond = torch.cat([synth.conditioning(500 + i, "smallrowsbench.cond", 1, 24, d) for i in range(batch)], 0).to(DEV)
    return lambda steps: timed(lambda: model.generate(cond, max_new_tokens=steps, cfg_scale=2.0 if guided else 1.0, batch_size=batch, sampling_params=GREEDY))


def serve_call(model):
    d = model.config.backbone.d_model
    cond = synth.conditioning(500, "smallrowsbench.cond", 2, 24, d).to(DEV)

    def run(steps):
        reqs = [GenRequest(cond, sampling_params=GREEDY, cfg_scale=2.0, max_new_tokens=steps)]
        return timed(lambda: list(model.serve(iter(reqs), slots=1, max_prompt=32, max_new_tokens=LONG, guided=True)))
    return run


def step_ms(call, settings, reps):
    """ms per decode step under each setting (a function that puts the engine into it), alternated per repetition: {name: (median, min, max)}."""
    per = {name: [] for name in settings}
    for name, put in settings.items():                  # warm-up: graphs of both launch lists
        put()
        call(SHORT)
        call(LONG)
    for _ in range(reps):
        for name, put in settings.items():
            put()
            a, b = call(SHORT), call(LONG)
            per[name].append((b - a) / (LONG - SHORT) * 1e3)
    return {name: stats(v) for name, v in per.items()}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smallrowsbench.txt"))
    args = ap.parse_args()
    lines = []
    counters = {}

    def emit(**kw):
        s = json.dumps(kw)
        print(s, flush=True)
        lines.append(s)

    def kernels(eng, name, which, iters, reads):
        for rows in ROWS:
            res, nbytes = kernel_us(eng, which, rows, args.reps, iters)
            for mode, (med, lo, hi) in res.items():
                eng.call("zn_debug_tune", KEY, mode)
                r8 = reads(rows)
                sb = nbytes / 2 if r8 else nbytes
                emit(figure="kernel", op=name, rows=rows, key=mode, stream=MODES[mode], reads_fp8=r8, us_per_launch_median=round(med, 2), min=round(lo, 2), max=round(hi, 2),
                     reps=args.reps, stream_bytes=sb, tb_per_s=round(sb / (med * 1e-6) / 1e12, 3))
            eng.call("zn_debug_tune", KEY, 1)
            for on in (2, 3):
                faster, spread = verdict(res, on)
                emit(figure="kernel.verdict", op=name, rows=rows, key=on, fp8_over_bf16=round(res[on][0] / res[1][0], 4), saved_us=round(res[1][0] - res[on][0], 2), spread_us=round(spread, 2),
                     fp8_faster_beyond_spread=faster)

    def steps(eng, name, rows, call, reads, audio_per_step):
        res = step_ms(call, {"bf16": lambda: eng.call("zn_debug_tune", KEY, 1), "fp8": lambda: eng.call("zn_debug_tune", KEY, 2)}, args.reps)
        for mode, key in (("bf16", 1), ("fp8", 2)):
            eng.call("zn_debug_tune", KEY, key)
            med, lo, hi = res[mode]
            emit(figure="step", case=name, rows=rows, stream=mode, reads_fp8=reads(rows), ms_per_step_median=round(med, 4), min=round(lo, 4), max=round(hi, 4), reps=args.reps,
                 audio_s_per_s=round(audio_per_step / 86 / (med * 1e-3), 1))
        eng.call("zn_debug_tune", KEY, 1)
        spread = max(res[m][2] - res[m][1] for m in res)
        emit(figure="step.verdict", case=name, rows=rows, fp8_over_bf16=round(res["fp8"][0] / res["bf16"][0], 4), saved_ms=round(res["bf16"][0] - res["fp8"][0], 4), spread_ms=round(spread, 4),
             fp8_faster_beyond_spread=bool(res["bf16"][0] - res["fp8"][0] > spread))

    # ------------------------------------------------------------------ the hybrid stack
    model, _ = build_model(synth.HYBRID_FULL_CFG, 1234, DEV)
    model.quantize_mamba_fp8()
    eng = model.engine(3)
    eng.call("zn_debug_eos_bias", float("-inf"))
    n_mamba = sum(1 for blk in model.backbone.layers if blk.is_mamba)
    reads = {}
    for mode in MODES:
        eng.call("zn_debug_tune", KEY, mode)
        reads[mode] = {rows: eng.mamba_fp8_plan(rows) for rows in (1, 2, 3, 4, 5)}
    eng.call("zn_debug_tune", KEY, 1)
    emit(figure="model", model="hybrid", layers=len(model.backbone.layers), mamba_layers=n_mamba, mamba_weights=model.mamba_weights, reads_fp8_by_key=reads)
    kernels(eng, "mamba_in_proj", 7, ITERS * n_mamba, lambda rows: eng.mamba_fp8_plan(rows)[0])
    kernels(eng, "mamba_out_proj, gated norm", 8, ITERS * n_mamba, lambda rows: eng.mamba_fp8_plan(rows)[1])
    for name, batch, guided in (("hybrid, 1 guided utterance", 1, True), ("hybrid, 2 guided utterances", 2, True), ("hybrid, 1 unguided utterance", 1, False),
                                ("hybrid, 3 unguided utterances", 3, False)):
        steps(eng, name, batch * (2 if guided else 1), gen_call(model, batch, guided), lambda rows: eng.mamba_fp8_plan(rows), batch)
    counters["hybrid"] = model.handoff_counters()
    del model, eng
    gc.collect()
    torch.cuda.empty_cache()
    # the out_proj without a prologue: a model of two norm groups (only its out_proj launches are measured)
    model, _ = build_model(dict(synth.HYBRID_FULL_CFG, ssm_cfg={"layer": "Mamba2", "d_state": 64, "ngroups": 2}), 1234, DEV)
    model.quantize_mamba_fp8()
    eng = model.engine(2)
    kernels(eng, "mamba_out_proj, two norm groups", 8, ITERS * n_mamba, lambda rows: eng.mamba_fp8_plan(rows)[1])
    del model, eng
    gc.collect()
    torch.cuda.empty_cache()
    # ------------------------------------------------------------------ the transformer
    model, _ = build_model(synth.FULL_CFG, 1234, DEV)
    model.quantize_mlp_fp8()
    eng = model.engine(2)
    eng.call("zn_debug_eos_bias", float("-inf"))
    n_layer = len(model.backbone.layers)
    reads = {}
    for mode in MODES:
        eng.call("zn_debug_tune", KEY, mode)
        reads[mode] = {rows: eng.mlp_fp8_plan(rows) for rows in (1, 2, 3, 4, 5)}
    eng.call("zn_debug_tune", KEY, 1)
    emit(figure="model", model="transformer", layers=n_layer, mlp_weights=model.mlp_weights, reads_fp8_by_key=reads)
    kernels(eng, "fc1", 0, ITERS * n_layer, lambda rows: eng.mlp_fp8_plan(rows)[0])
    kernels(eng, "fc2", 1, ITERS * n_layer, lambda rows: eng.mlp_fp8_plan(rows)[1])
    steps(eng, "transformer, 2 guided utterances", 4, gen_call(model, 2, True), lambda rows: eng.mlp_fp8_plan(rows), 2)
    steps(eng, "transformer, one-slot guided session", 2, serve_call(model), lambda rows: eng.mlp_fp8_plan(rows), 1)
    # observation only: batch 1 on the launches path with the stream against the whole-step kernel on the bf16 copy
    def launches_fp8():
        eng.call("zn_debug_tune", _lib.ZN_TUNE_PERSISTENT, 2)
        eng.call("zn_debug_tune", KEY, 2)

    def launches_bf16():
        eng.call("zn_debug_tune", _lib.ZN_TUNE_PERSISTENT, 2)
        eng.call("zn_debug_tune", KEY, 1)

    def whole_step():
        eng.call("zn_debug_tune", _lib.ZN_TUNE_PERSISTENT, 1)
        eng.call("zn_debug_tune", KEY, 1)
    res = step_ms(gen_call(model, 1, True), {"launches, fp8": launches_fp8, "launches, bf16": launches_bf16, "whole-step kernel, bf16": whole_step}, args.reps)
    whole_step()
    for name, (med, lo, hi) in res.items():
        emit(figure="observed", case="transformer, 1 guided utterance", rows=2, path=name, ms_per_step_median=round(med, 4), min=round(lo, 4), max=round(hi, 4), reps=args.reps)
    counters["transformer"] = model.handoff_counters()
    emit(figure="counters", **counters)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("python tools/smallrowsbench.py --reps %d\n" % args.reps + "\n".join(lines) + "\n")
    bad = sum(cs.get("repeated_generations", 0) + sum(v.get("handoff_timeouts", 0) + v.get("demoted", 0) for v in cs.values() if isinstance(v, dict)) for cs in counters.values())
    if bad:
        print("hand-off timeouts or demotions were counted: FAIL", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
