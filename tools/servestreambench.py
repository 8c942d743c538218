"""tools/servebench.py's workload (32 requests of 2 .. 10 s, eight slots, Zonos-v0.1 dimensions, guided, EOS suppressed) with audio out:

  (A) serve + decode   `Zonos.serve()`, and `autoencoder.decode()` of each result as it arrives: audio when the request has finished
  (B) serve_stream     `Zonos.serve_stream(chunk_frames)`: audio chunks while the request runs, all slots' DAC windows in one ragged pass

Per column, over three alternated repeats: aggregate audio seconds per second (frames / 86 / wall), wall time per session step, and per
request the time from its admission to its first non-empty audio (median and maximum over the 32 requests of the median repeat).  The
admission time is the host's clock when the admission was enqueued; the first audio counts once an event recorded behind it has completed
(one event wait per request; the session's own read-back keeps host and device within one scheduling interval of each other).

In a run of its own: one zn_dac_decode_spans call over eight 28-frame windows (interior windows at different places of their sequences)
against eight zn_dac_decode_span(batch = 1) calls, device time between events around 20 repetitions after 3 warm-up calls.

One JSON line per case; everything is also written to profiles/servestreambench.txt.

    python tools/servestreambench.py [--reps 3] [--sched-every 8] [--chunk-frames 16]
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
from zonos_amd import _lib, synth  # noqa: E402
from zonos_amd.autoencoder import DACAutoencoder  # noqa: E402
from zonos_amd.model import GenRequest  # noqa: E402
from zonos_amd.testing import build_model  # noqa: E402
from tools.servebench import BUDGETS, FPS, LENGTHS, N, SLOTS  # noqa: E402


def ragged_against_loop(ae, dev, rows=8, n=28, reps=20, warm=3):
    """(ms per ragged call, ms per `rows` single-row calls, max |difference| between their outputs)."""
    wins = [(10 + 37 * r, n, 0) for r in range(rows)]
    codes = torch.from_numpy(synth.randint(5, "servestreambench.codes", (rows, 9, n), 1024)).to(torch.int32).to(dev)
    spans = [ae.span(*w) for w in wins]
    t_max = max(s1 - s0 for s0, s1 in spans)
    wav = torch.zeros(rows, t_max, device=dev)
    one = [torch.zeros(1, s1 - s0, device=dev) for s0, s1 in spans]
    parts = [codes[r:r + 1].contiguous() for r in range(rows)]
    arr = (_lib.zn_dac_span_row * rows)(*[_lib.zn_dac_span_row(*w) for w in wins])
    lib, h, st = _lib.load(), ae._handle(), _lib.stream_ptr()

    def ragged():
        _lib.check_dac(lib.zn_dac_decode_spans(h, codes.data_ptr(), n, arr, rows, wav.data_ptr(), t_max, st), h, "zn_dac_decode_spans")

    def loop():
        for r, (c0, k, e) in enumerate(wins):
            _lib.check_dac(lib.zn_dac_decode_span(h, parts[r].data_ptr(), 1, c0, k, e, one[r].data_ptr(), st), h, "zn_dac_decode_span")

    def timed(fn):
        for _ in range(warm):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps
    t_ragged, t_loop = timed(ragged), timed(loop)
    diff = max(float((wav[r, :one[r].shape[1]] - one[r][0]).abs().max()) for r in range(rows))
    return t_ragged, t_loop, diff


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sched-every", type=int, default=8)
    ap.add_argument("--chunk-frames", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "servestreambench.txt"))
    args = ap.parse_args()
    dev = "cuda:0"
    cfg, seed = synth.FULL_CFG, 1234
    d = cfg["d_model"]
    dac = DACAutoencoder(synth.dac_state_dict(4321, encoder=False), device=dev)
    model, _ = build_model(cfg, seed, dev, dac=dac)
    reqs = [GenRequest(synth.conditioning(seed + i, "servebench.cond", 2, LENGTHS[i], d).to(dev), sampling_params=dict(temperature=0.0), cfg_scale=2.0,
                       max_new_tokens=BUDGETS[i]) for i in range(N)]
    eng = model.engine(SLOTS)
    eng.call("zn_debug_eos_bias", float("-inf"))
    frames = sum(BUDGETS)
    kw = dict(slots=SLOTS, max_prompt=max(LENGTHS), max_new_tokens=max(BUDGETS), guided=True, sched_every=args.sched_every)

    def heard(first, index):
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()
        first[index] = time.perf_counter()

    def column_a():
        stats, first, samples = {}, {}, 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for res in model.serve(iter(reqs), _stats=stats, **kw):
            wav = dac.decode(res.codes)
            samples += wav.shape[2]
            heard(first, res.index)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, stats, first, samples

    def column_b():
        stats, first, samples = {}, {}, 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for ch in model.serve_stream(iter(reqs), chunk_frames=args.chunk_frames, _stats=stats, **kw):
            samples += ch.wav.shape[2]
            if ch.wav.shape[2] and ch.index not in first:
                heard(first, ch.index)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, stats, first, samples

    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)
    column_a()                                                 # warm-up of the session's graphs, the DAC workspace and the scratch cache
    column_b()
    runs = {"serve+decode": [], "serve_stream": []}
    for _ in range(args.reps):                                 # alternated
        runs["serve+decode"].append(column_a())
        runs["serve_stream"].append(column_b())
    med = {}
    for name, rr in runs.items():
        assert all(s == frames * dac.hop for _, _, _, s in rr), "every sample of every request comes out once"
        walls = sorted(t for t, _, _, _ in rr)
        t, stats, first, _ = sorted(rr, key=lambda x: x[0])[len(rr) // 2]
        lat = sorted(1e3 * (first[i] - stats["admitted_at"][i]) for i in range(N))
        med[name] = dict(wall=t, lat=statistics.median(lat))
        emit(dict(case=name, slots=SLOTS, sched_every=args.sched_every, **({"chunk_frames": args.chunk_frames} if name == "serve_stream" else {}),
                  steps=stats["steps"], wall_s_all=[round(x, 4) for x in walls], audio_s_per_s=round(frames / FPS / t, 2),
                  ms_per_step_median=round(1e3 * t / stats["steps"], 4), ms_per_step_all=[round(1e3 * x / stats["steps"], 4) for x in walls],
                  first_audio_ms_median=round(statistics.median(lat), 1), first_audio_ms_max=round(lat[-1], 1), first_audio_ms_min=round(lat[0], 1)))
    t_ragged, t_loop, diff = ragged_against_loop(dac, dev)
    emit(dict(case="ragged pass against the loop", rows=8, frames_per_window=28, ms_zn_dac_decode_spans=round(t_ragged, 4),
              ms_eight_zn_dac_decode_span=round(t_loop, 4), ragged_over_loop=round(t_ragged / t_loop, 3), max_abs_difference=diff))
    a, b = med["serve+decode"], med["serve_stream"]
    counters = {f"engine_max_rows_{eng.max_rows}": eng.counters()}
    emit(dict(summary=dict(frames=frames, audio_s=round(frames / FPS, 1), throughput_stream_over_serve=round(a["wall"] / b["wall"], 3),
                           first_audio_ms_serve=round(a["lat"], 1), first_audio_ms_stream=round(b["lat"], 1)), handoff_counters=counters))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# tools/servestreambench.py --reps {args.reps} --sched-every {args.sched_every} --chunk-frames {args.chunk_frames}\n" + "\n".join(lines) + "\n")
    return 0 if diff == 0.0 and all(x["handoff_timeouts"] == 0 for x in counters.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
