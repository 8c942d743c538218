"""The Mamba2 in_proj of a hybrid decode step of 17..64 rows in its three forms (ZN_TUNE_WIDE_HYBRID): 1 = groups of 16 rows (the weights
streamed once per group), 2 = row groups on the grid of gemm16k_kernel (one launch; the weight tile re-read through L2 per 16 rows), 3 = the row-tile loop
(gemm16k_rows_kernel: the weight tile requested once per up to 64 rows).  Zonos-v0.1-hybrid dimensions (synth.HYBRID_FULL_CFG: 46 layers, 42 of them
Mamba2) with seeded synthetic weights, one process and one model:

  kernels   zn_bench_kernel(which = 7) at 18, 32, 48 and 64 rows, cycling through the 42 Mamba2 layers' weights: microseconds per in_proj over all its
            launches, under each form, alternated per repetition; median, min and max of the repetitions.
  steps     a decode step at 9, 16, 24 and 32 guided utterances (18 .. 64 rows), greedy, EOS suppressed: wall time of generate() at two lengths, their
            difference per step - the three forms alternated per repetition; median, min and max.
  counters  the handle's hand-off / timeout counters (zn_get_counters).  A hand-off timeout makes the tool fail.

    python tools/hybridwidebench.py [--reps 20]

One JSON line per figure; everything is also written to profiles/hybridwidebench.txt.  The last lines name, per row count, the fastest form and whether
it beats groups of 16 by more than the spread of the repetitions (max - min of either): that is what wide_hybrid_form (zn_linear_plan.h) should return."""
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
FORMS = {1: "groups of 16", 2: "row groups on grid y", 3: "row-tile loop"}


def generate(model, batch, steps, seed=500):
    d = model.config.backbone.d_model
    cond = torch.cat([synth.conditioning(seed + i, "hybridwidebench.cond", 2, 24, d) for i in range(batch)], 0)
    cond = torch.cat([cond[0::2], cond[1::2]], 0).to(DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.generate(cond, max_new_tokens=steps, cfg_scale=2.0, batch_size=batch, sampling_params=GREEDY)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(v):
    return statistics.median(v), min(v), max(v)


def kernel_us(eng, rows, reps, iters):
    """us per Mamba2 in_proj (all its launches) under each form, alternated per repetition: {form: (median, min, max)}."""
    ms, by = C.c_float(0), C.c_double(0)
    per = {f: [] for f in FORMS}
    st = _lib.stream_ptr()
    for rep in range(reps + 1):                          # repetition 0 warms up
        for form in FORMS:
            eng.call("zn_debug_tune", _lib.ZN_TUNE_WIDE_HYBRID, form)
            eng.call("zn_bench_kernel", 7, rows, iters, C.byref(ms), C.byref(by), st)
            if rep:
                per[form].append(ms.value * 1e3)
    return {f: stats(v) for f, v in per.items()}, by.value


def step_ms(model, eng, batch, reps, short=24, long=88):
    """ms per decode step under each form, alternated per repetition: {form: (median, min, max)}."""
    per = {f: [] for f in FORMS}
    for form in FORMS:                                   # warm-up: graphs of every form's launch list
        eng.call("zn_debug_tune", _lib.ZN_TUNE_WIDE_HYBRID, form)
        generate(model, batch, short)
        generate(model, batch, long)
    for _ in range(reps):
        for form in FORMS:
            eng.call("zn_debug_tune", _lib.ZN_TUNE_WIDE_HYBRID, form)
            a, b = generate(model, batch, short), generate(model, batch, long)
            per[form].append((b - a) / (long - short) * 1e3)
    return {f: stats(v) for f, v in per.items()}


def verdict(res):
    """The fastest form, and whether it beats groups of 16 by more than the spread of the repetitions."""
    best = min(res, key=lambda f: res[f][0])
    spread = max(res[f][2] - res[f][1] for f in (1, best))
    return best if best != 1 and res[1][0] - res[best][0] > spread else 1, spread


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hybridwidebench.txt"))
    args = ap.parse_args()
    lines = []

    def emit(**kw):
        s = json.dumps(kw)
        print(s, flush=True)
        lines.append(s)
    model, _ = build_model(synth.HYBRID_FULL_CFG, 1234, DEV)
    eng = model.engine(32)
    eng.call("zn_debug_eos_bias", float("-inf"))
    emit(figure="default", note="ZN_TUNE_WIDE_HYBRID unset", rows_per_weight_pass={rows: eng.hybrid_rows_plan(rows) for rows in (18, 32, 48, 64)})
    n_mamba = sum(1 for blk in model.backbone.layers if blk.is_mamba)
    picks = {}
    for rows in (18, 32, 48, 64):
        res, nbytes = kernel_us(eng, rows, args.reps, 2 * n_mamba)
        for form, (med, lo, hi) in res.items():
            eng.call("zn_debug_tune", _lib.ZN_TUNE_WIDE_HYBRID, form)
            per = eng.hybrid_rows_plan(rows)["mamba_in_proj"]
            emit(figure="kernel", op="mamba_in_proj", rows=rows, wide_hybrid=form, form=FORMS[form], rows_per_weight_pass=per, weight_passes=-(-rows // per), us_per_projection_median=round(med, 2),
                 min=round(lo, 2), max=round(hi, 2), reps=args.reps, weight_bytes=nbytes, tb_per_s_of_one_pass=round(nbytes / (med * 1e-6) / 1e12, 3))
        best, spread = verdict(res)
        picks[rows] = best
        emit(figure="kernel.verdict", rows=rows, fastest=min(res, key=lambda f: res[f][0]), spread_us=round(spread, 2), pick=best)
    for batch in (9, 16, 24, 32):
        res = step_ms(model, eng, batch, args.reps)
        for form, (med, lo, hi) in res.items():
            eng.call("zn_debug_tune", _lib.ZN_TUNE_WIDE_HYBRID, form)
            emit(figure="step", utterances=batch, rows=2 * batch, wide_hybrid=form, form=FORMS[form], rows_per_weight_pass=eng.hybrid_rows_plan(2 * batch), ms_per_step_median=round(med, 4),
                 min=round(lo, 4), max=round(hi, 4), reps=args.reps, audio_s_per_s=round(batch / 86 / (med * 1e-3), 1))
        best, spread = verdict(res)
        emit(figure="step.verdict", utterances=batch, rows=2 * batch, fastest=min(res, key=lambda f: res[f][0]), spread_ms=round(spread, 4), pick=best)
    counters = model.handoff_counters()
    emit(figure="counters", **counters)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("python tools/hybridwidebench.py --reps %d\n" % args.reps + "\n".join(lines) + "\n")
    bad = counters.get("repeated_generations", 0) + sum(v.get("handoff_timeouts", 0) + v.get("demoted", 0) for v in counters.values() if isinstance(v, dict))
    if bad:
        print("hand-off timeouts or demotions were counted: FAIL", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
