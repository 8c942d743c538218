"""What the output stage (`sample_rate` / `pcm16`) costs, at the Zonos-v0.1 dimensions with synthetic weights.

  (1) a 10 s clip (861 frames) through `autoencoder.decode(codes, sample_rate, pcm16)` to 48 kHz PCM16 and to 8 kHz fp32, against
      `decode()` + `sinc_resample` (+ clamp for PCM16) on the same device, and against `decode()` alone;
  (2) `Zonos.stream()` of the clip (greedy, EOS suppressed) with sample_rate=48000, pcm16=True against the same call without them: time
      to the first audio and total wall time;
  (3) a `Zonos.serve_stream()` session (tools/servebench.py's workload), likewise: wall time per session step.

Every pair is alternated; the figures are medians over the repetitions with their extremes.  One JSON line per case; everything is also
written to profiles/resamplebench.txt.  No bar is set.

    python tools/resamplebench.py [--reps 20] [--stream-reps 20] [--serve-reps 20] [--skip-serve]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zonos_amd import synth  # noqa: E402
from zonos_amd.autoencoder import DACAutoencoder, sinc_resample  # noqa: E402
from zonos_amd.model import GenRequest  # noqa: E402
from zonos_amd.testing import build_model  # noqa: E402
from tools.servebench import BUDGETS, LENGTHS, N, SLOTS  # noqa: E402

FRAMES, L_C = 861, 24


def spread(xs, digits=3):
    xs = sorted(xs)
    return dict(median=round(statistics.median(xs), digits), min=round(xs[0], digits), max=round(xs[-1], digits))


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stream-reps", type=int, default=20)
    ap.add_argument("--serve-reps", type=int, default=20)
    ap.add_argument("--skip-serve", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resamplebench.txt"))
    args = ap.parse_args()
    dev = "cuda:0"
    cfg, seed = synth.FULL_CFG, 1234
    dac = DACAutoencoder(synth.dac_state_dict(4321, encoder=False), device=dev)
    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    # (1) the clip
    codes = torch.from_numpy(synth.randint(9, "resamplebench.codes", (1, 9, FRAMES), 1024)).to(dev)

    def torch_path(rate, pcm):
        y = sinc_resample(dac.decode(codes), dac.sampling_rate, rate)
        return torch.clamp(y * 32767.0, -32767.0, 32767.0).to(torch.int16) if pcm else y
    for rate, pcm in ((48000, True), (8000, False)):
        cols = {"decode": lambda: dac.decode(codes), "decode+stage": lambda: dac.decode(codes, rate, pcm), "decode+sinc_resample": lambda: torch_path(rate, pcm)}
        for fn in cols.values():
            fn()
        got, ref = cols["decode+stage"](), cols["decode+sinc_resample"]()
        diff = float((got.double() - ref.double()).abs().max()) / (32767.0 if pcm else 1.0)
        times = {k: [] for k in cols}
        for _ in range(args.reps):                             # alternated
            for k, fn in cols.items():
                times[k].append(wall_ms(fn)[1])
        emit(dict(case="10 s clip", sample_rate=rate, pcm16=pcm, reps=args.reps, samples_out=int(got.shape[2]),
                  ms={k: spread(v) for k, v in times.items()},
                  stage_ms_median=round(statistics.median(times["decode+stage"]) - statistics.median(times["decode"]), 3),
                  sinc_resample_ms_median=round(statistics.median(times["decode+sinc_resample"]) - statistics.median(times["decode"]), 3),
                  max_abs_difference_to_sinc_resample=diff))

    # (2) stream()
    model, _ = build_model(cfg, seed, dev, dac=dac)
    c = synth.conditioning(seed, "cond", 1, L_C, cfg["d_model"]).to(dev)
    cond = torch.cat([c, c], 0)
    kw = dict(max_new_tokens=FRAMES, sampling_params={"temperature": 0.0}, seed=7, chunk_frames=16)
    eng = model.engine(1)
    eng.call("zn_debug_eos_bias", float("-inf"))

    def stream(**audio):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first, samples = None, 0
        for ch in model.stream(cond, **kw, **audio):
            if first is None and ch.wav.shape[2]:
                ev = torch.cuda.Event()
                ev.record()
                ev.synchronize()
                first = 1e3 * (time.perf_counter() - t0)
            samples += ch.wav.shape[2]
        torch.cuda.synchronize()
        return first, 1e3 * (time.perf_counter() - t0), samples
    variants = {"plain": {}, "48 kHz PCM16": dict(sample_rate=48000, pcm16=True)}
    try:
        for a in variants.values():
            stream(**a)
        runs = {k: [] for k in variants}
        for _ in range(args.stream_reps):                      # alternated
            for k, a in variants.items():
                runs[k].append(stream(**a))
    finally:
        eng.call("zn_debug_eos_bias", 0.0)
    emit(dict(case="stream() of a 10 s clip", reps=args.stream_reps, chunk_frames=16,
              first_audio_ms={k: spread([r[0] for r in v], 2) for k, v in runs.items()},
              total_ms={k: spread([r[1] for r in v], 2) for k, v in runs.items()},
              samples={k: v[0][2] for k, v in runs.items()}, handoff=model.handoff_counters()))

    # (3) serve_stream()
    if not args.skip_serve:
        d = cfg["d_model"]
        reqs = [GenRequest(synth.conditioning(seed + i, "servebench.cond", 2, LENGTHS[i], d).to(dev), sampling_params=dict(temperature=0.0), cfg_scale=2.0,
                           max_new_tokens=BUDGETS[i]) for i in range(N)]
        seng = model.engine(SLOTS)
        seng.call("zn_debug_eos_bias", float("-inf"))
        skw = dict(slots=SLOTS, max_prompt=max(LENGTHS), max_new_tokens=max(BUDGETS), guided=True, sched_every=8, chunk_frames=16)

        def session(**audio):
            stats, samples = {}, 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for ch in model.serve_stream(iter(reqs), _stats=stats, **skw, **audio):
                samples += ch.wav.shape[2]
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / stats["steps"], stats["steps"], samples
        try:
            for a in variants.values():
                session(**a)
            sruns = {k: [] for k in variants}
            for _ in range(args.serve_reps):                   # alternated
                for k, a in variants.items():
                    sruns[k].append(session(**a))
        finally:
            seng.call("zn_debug_eos_bias", 0.0)
        emit(dict(case="serve_stream() session step", reps=args.serve_reps, requests=N, slots=SLOTS, sched_every=8, chunk_frames=16,
                  steps={k: v[0][1] for k, v in sruns.items()}, ms_per_step={k: spread([r[0] for r in v], 4) for k, v in sruns.items()},
                  samples={k: v[0][2] for k, v in sruns.items()}))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/resamplebench.py " + " ".join(sys.argv[1:]) + "\n" + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
