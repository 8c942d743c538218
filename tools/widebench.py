"""Decode steps of 17..64 rows, each weight streamed once per step (the wide plan) against groups of 16 rows (ZN_TUNE_WIDE_ROWS = 1:
the path every such step took before, each weight streamed once per 16 rows), at the Zonos-v0.1 dimensions with seeded synthetic weights, in one
process and one model:

  kernels   zn_bench_kernel for fc1, fc2, out_proj, the heads and in_proj (which = 0 .. 4) at 18, 32, 48 and 64 rows, cycling through the 26
            layers' weights: microseconds per projection over all its launches, with the tune key unset and at 1.
  steps     a decode step at 9, 16, 24 and 32 guided utterances (18 .. 64 rows), greedy, EOS suppressed: wall time of generate() at two lengths,
            their difference per step, median over the repetitions - wide against grouped, alternated per repetition.
  steps     the same after quantize_mlp_fp8() (fc1 / fc2 read as the FP8 stream in both modes).
  serve     tools/servebench.py's 32 requests through one serve() session of 16 guided slots (32 rows, wide) against one of 8 slots (16 rows).

    python tools/widebench.py [--reps 20]

ZN_TUNE_WIDE_ROWS cannot be unset once set: after the kernel figures the tool switches between 1 and 2, and 2 plans a generation step exactly as
the unset key does (zn_decode_rows_plan is printed beside every figure).  One JSON line per figure; everything is also written to
profiles/widebench.txt."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from zonos_amd import _lib, synth  # noqa: E402
from zonos_amd.model import GenRequest  # noqa: E402
from zonos_amd.testing import build_model  # noqa: E402

DEV = "cuda:0"
GREEDY = dict(temperature=0.0)
GROUPED, WIDE = 1, 2
WHICH = ("fc1", "fc2", "out_proj", "heads", "in_proj")


def generate(model, batch, steps, seed=500):
    d = model.config.backbone.d_model
    cond = torch.cat([synth.conditioning(seed + i, "widebench.cond", 2, 24, d) for i in range(batch)], 0)
    cond = torch.cat([cond[0::2], cond[1::2]], 0).to(DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.generate(cond, max_new_tokens=steps, cfg_scale=2.0, batch_size=batch, sampling_params=GREEDY)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def step_ms(model, eng, batch, reps, short=24, long=88):
    """ms per decode step in both modes, alternated per repetition: {mode: (median, min, max)}."""
    per = {GROUPED: [], WIDE: []}
    for mode in (GROUPED, WIDE):                        # warm-up: graphs of both modes' launch lists
        eng.call("zn_debug_tune", _lib.ZN_TUNE_WIDE_ROWS, mode)
        generate(model, batch, short)
        generate(model, batch, long)
    for _ in range(reps):
        for mode in (GROUPED, WIDE):
            eng.call("zn_debug_tune", _lib.ZN_TUNE_WIDE_ROWS, mode)
            a, b = generate(model, batch, short), generate(model, batch, long)
            per[mode].append((b - a) / (long - short) * 1e3)
    return {m: (statistics.median(v), min(v), max(v)) for m, v in per.items()}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "widebench.txt"))
    ap.add_argument("--skip-serve", action="store_true")
    args = ap.parse_args()
    lines = []

    def emit(**kw):
        s = json.dumps(kw)
        print(s, flush=True)
        lines.append(s)
    model, _ = build_model(synth.FULL_CFG, 1234, DEV)
    eng = model.engine(32)
    eng.call("zn_debug_eos_bias", float("-inf"))
    st = _lib.stream_ptr()
    # ---- kernels: the tune key unset first (it cannot be unset again), then 1
    ms, by = C.c_float(0), C.c_double(0)
    for label, tune in (("unset", None), ("grouped", GROUPED)):
        if tune is not None:
            eng.call("zn_debug_tune", _lib.ZN_TUNE_WIDE_ROWS, tune)
        for rows in (18, 32, 48, 64):
            plan = eng.decode_rows_plan(rows)
            for which, name in enumerate(WHICH):
                eng.call("zn_bench_kernel", which, rows, 260, C.byref(ms), C.byref(by), st)
                passes = -(-rows // plan[name])
                emit(figure="kernel", op=name, rows=rows, wide_rows=label, rows_per_weight_pass=plan[name], weight_passes=passes, us_per_projection=round(ms.value * 1e3, 2),
                     weight_bytes=by.value, tb_per_s_of_one_pass=round(by.value / (ms.value * 1e-3) / 1e12, 3))
    # ---- steps, bf16 then FP8
    for stream in ("bf16", "fp8"):
        if stream == "fp8":
            model.quantize_mlp_fp8()
            eng = model.engine(32)
            eng.call("zn_debug_eos_bias", float("-inf"))
        for batch in (9, 16, 24, 32):
            res = step_ms(model, eng, batch, args.reps)
            for mode, label in ((GROUPED, "grouped"), (WIDE, "wide")):
                eng.call("zn_debug_tune", _lib.ZN_TUNE_WIDE_ROWS, mode)
                med, lo, hi = res[mode]
                emit(figure="step", utterances=batch, rows=2 * batch, mlp_stream=stream, reads_fp8=eng.mlp_fp8_plan(2 * batch), wide_rows=label, rows_per_weight_pass=eng.decode_rows_plan(2 * batch),
                     ms_per_step_median=round(med, 4), min=round(lo, 4), max=round(hi, 4), reps=args.reps, audio_s_per_s=round(batch / 86 / (med * 1e-3), 1))
    # ---- serve: servebench's requests through 32 rows (wide) against 16
    if not args.skip_serve:
        import servebench as sb
        d = synth.FULL_CFG["d_model"]
        reqs = [GenRequest(synth.conditioning(1234 + i, "servebench.cond", 2, sb.LENGTHS[i], d).to(DEV), sampling_params=GREEDY, cfg_scale=2.0, max_new_tokens=sb.BUDGETS[i])
                for i in range(sb.N)]
        eng.call("zn_debug_tune", _lib.ZN_TUNE_WIDE_ROWS, WIDE)
        for slots in (16, 8, 16, 8):                       # the first pair warms up
            stats = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = {r.index: r.codes.shape[2] for r in model.serve(iter(reqs), slots=slots, max_prompt=max(sb.LENGTHS), max_new_tokens=max(sb.BUDGETS), guided=True, sched_every=8, _stats=stats)}
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert [got[i] for i in range(sb.N)] == sb.BUDGETS
            emit(figure="serve", requests=sb.N, slots=slots, rows=2 * slots, mlp_stream="fp8", rows_per_weight_pass=eng.decode_rows_plan(2 * slots), seconds=round(dt, 3),
                 decode_steps=stats.get("steps"), audio_s_per_s=round(sum(sb.BUDGETS) / 86 / dt, 1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("python tools/widebench.py --reps %d\n" % args.reps + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
