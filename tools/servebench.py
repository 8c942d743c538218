"""32 requests of 2 .. 10 s through `Zonos.serve(slots=8)` against the same requests as four `generate_batch()` calls of eight in arrival
order, in one process, at the Zonos-v0.1 dimensions, guided, EOS suppressed:

  (a) batch    four generate_batch(ragged_prefix=True) calls: every call runs until its longest request has spent its budget
  (b) serve    one session of eight slots: a request leaves at the first scheduling point after its own end, the next one takes its slot

The step counts are arithmetic and printed next to the measured ones: (a) runs, per call, max budget + 9 - 2 steps (the loop ends at the
code buffer's last column), their sum over the four calls; (b) runs until its last slot frees, each request holding a slot for
ceil((budget + 9 - 1) / sched_every) scheduling intervals (tests/test_serve_cpu.py derives the same recurrence).  Reported per case:
decode steps, wall time, aggregate audio seconds per second (frames / 86 / wall), wall time per step; for (a) per repeat, with the
spread; for (b) also the time per admission (a run of its own with every admission bracketed by a synchronisation) and the time per step
with the admissions taken out.  One JSON line per case and a summary line; everything is also written to profiles/servebench.txt.

    python tools/servebench.py [--reps 3] [--sched-every 8]
"""
import argparse
import heapq
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from zonos_amd import synth  # noqa: E402
from zonos_amd.model import GenRequest  # noqa: E402
from zonos_amd.testing import build_model  # noqa: E402

N, SLOTS, NQ, FPS = 32, 8, 9, 86
ORDER = [(13 * i + 5) % N for i in range(N)]                                 # arrival order: a fixed permutation of the budget ladder
BUDGETS = [FPS * 2 + (FPS * 8 * k) // (N - 1) for k in ORDER]                 # 2 .. 10 s
LENGTHS = [16 + (24 * ((7 * i) % N)) // (N - 1) for i in range(N)]            # 16 .. 40 conditioning positions


def expected_steps(sched_every):
    batch = sum(max(BUDGETS[g:g + SLOTS]) + NQ - 2 for g in range(0, N, SLOTS))
    free = [(0, b) for b in range(SLOTS)]
    heapq.heapify(free)
    end = 0
    for n in BUDGETS:
        at, slot = heapq.heappop(free)
        at += -(-(n + NQ - 1) // sched_every) * sched_every
        end = max(end, at)
        heapq.heappush(free, (at, slot))
    return batch, end


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sched-every", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "servebench.txt"))
    args = ap.parse_args()
    dev = "cuda:0"
    cfg, seed = synth.FULL_CFG, 1234
    d = cfg["d_model"]
    model, _ = build_model(cfg, seed, dev)
    reqs = [GenRequest(synth.conditioning(seed + i, "servebench.cond", 2, LENGTHS[i], d).to(dev), sampling_params=dict(temperature=0.0), cfg_scale=2.0,
                       max_new_tokens=BUDGETS[i]) for i in range(N)]
    eng = model.engine(SLOTS)
    eng.call("zn_debug_eos_bias", float("-inf"))
    frames = sum(BUDGETS)

    def batch(trace=False):
        steps = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for g in range(0, N, SLOTS):
            tr = {"logits": []} if trace else None
            outs = model.generate_batch(reqs[g:g + SLOTS], ragged_prefix=True, _trace=tr)
            assert [o.shape[2] for o in outs] == BUDGETS[g:g + SLOTS]
            steps += len(tr["logits"]) - 1 if trace else 0
        torch.cuda.synchronize()
        return time.perf_counter() - t0, steps

    def serve(time_admissions=False):
        stats = dict(time_admissions=time_admissions)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = {r.index: r.codes.shape[2] for r in model.serve(iter(reqs), slots=SLOTS, max_prompt=max(LENGTHS), max_new_tokens=max(BUDGETS), guided=True,
                                                              sched_every=args.sched_every, _stats=stats)}
        torch.cuda.synchronize()
        assert [got[i] for i in range(N)] == BUDGETS
        return time.perf_counter() - t0, stats

    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)
    exp_batch, exp_serve = expected_steps(args.sched_every)
    model.generate_batch([GenRequest(r.conditioning, sampling_params=r.sampling_params, cfg_scale=2.0, max_new_tokens=24) for r in reqs[:SLOTS]], ragged_prefix=True)   # warm-up
    _, batch_steps = batch(trace=True)                         # the measured step count (one step per enqueue: not timed)
    serve()                                                    # warm-up of the session's graphs and scratch cache
    tb, tsv, st = [], [], None
    for _ in range(args.reps):                                 # alternated
        tb.append(batch()[0])
        t, st = serve()
        tsv.append(t)
    t_adm, st_adm = serve(time_admissions=True)
    b_ms = sorted(1e3 * t / batch_steps for t in tb)
    s_ms = sorted(1e3 * t / st["steps"] for t in tsv)
    emit(dict(case="batch", calls=N // SLOTS, steps_expected=exp_batch, steps_measured=batch_steps, wall_s_all=[round(t, 4) for t in tb],
              audio_s_per_s=round(frames / FPS / sorted(tb)[len(tb) // 2], 2), ms_per_step_median=round(b_ms[len(b_ms) // 2], 4),
              ms_per_step_all=[round(x, 4) for x in b_ms]))
    emit(dict(case="serve", slots=SLOTS, sched_every=args.sched_every, steps_expected=exp_serve, steps_measured=st["steps"], admissions=st["admissions"],
              wall_s_all=[round(t, 4) for t in tsv], audio_s_per_s=round(frames / FPS / sorted(tsv)[len(tsv) // 2], 2),
              ms_per_step_median=round(s_ms[len(s_ms) // 2], 4), ms_per_step_all=[round(x, 4) for x in s_ms],
              ms_per_admission=round(1e3 * st_adm["admit_seconds"] / st_adm["admissions"], 3),
              ms_per_step_without_admissions=round(1e3 * (t_adm - st_adm["admit_seconds"]) / st_adm["steps"], 4)))
    counters = {f"engine_max_rows_{eng.max_rows}": eng.counters()}
    emit(dict(summary=dict(frames=frames, audio_s=round(frames / FPS, 1), batch_steps=batch_steps, serve_steps=st["steps"],
                           steps_saved=round(1 - st["steps"] / batch_steps, 3), batch_spread_ms_per_step=round(b_ms[-1] - b_ms[0], 4),
                           serve_minus_batch_ms_per_step=round(s_ms[len(s_ms) // 2] - b_ms[len(b_ms) // 2], 4),
                           steps_as_expected=(batch_steps == exp_batch and st["steps"] == exp_serve)), handoff_counters=counters))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# tools/servebench.py --reps {args.reps} --sched-every {args.sched_every}\n" + "\n".join(lines) + "\n")
    return 0 if all(x["handoff_timeouts"] == 0 for x in counters.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
