"""tools/servebench.py's 32 requests of 2 .. 10 s with every second one at cfg_scale = 1, at the Zonos-v0.1 dimensions, EOS suppressed, in one
process:

  (a) mixed    one session of 16 rows, `serve(guided=None)`: an unguided request takes one row, a guided one two
  (b) split    a guided session of 8 slots over the 16 guided requests, then an unguided session of 8 slots over the 16 unguided ones:
               what a server with both kinds of traffic had to run before - here one after the other on one device

Both run 16 rows per decode step while both kinds are present; (b)'s second session runs 8.  The expectation to confirm or refute: (a)
makes fewer passes over the weights, at a sampler tail that is up to twice as wide (one sampler workgroup row per row instead of one per
guided request).  Reported per case: decode steps (measured, and as `SlotScheduler` predicts them), wall time of three alternated
repeats, aggregate audio seconds per second (frames / 86 / median wall), wall time per session step, and the hand-off counters.  One JSON
line per case and a summary line; everything is also written to profiles/mixedbench.txt.

    python tools/mixedbench.py [--reps 3] [--sched-every 8]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))
from servebench import BUDGETS, FPS, LENGTHS, N, NQ  # noqa: E402
from zonos_amd import synth  # noqa: E402
from zonos_amd.model import GenRequest  # noqa: E402
from zonos_amd.serving import SlotScheduler  # noqa: E402
from zonos_amd.testing import build_model  # noqa: E402

ROWS, SLOTS = 16, 8
UNGUIDED = [i % 2 == 1 for i in range(N)]


def expected_steps(indices, slots, sched_every, needs):
    """The session's decode steps as the scheduler alone predicts them (EOS suppressed: a request holds its slots for budget + 9 - 1 steps)."""
    s = SlotScheduler(slots, NQ, sched_every)
    src = iter(indices)
    while True:
        s.pull(src, lambda i: (0, BUDGETS[i], needs[i]))
        if s.finished():
            return s.step
        s.advance()
        for b in s.wants_eos([0 if r is not None and s.own_steps(b) >= r.max_new_tokens + NQ - 1 else 1 for b, r in enumerate(s.rows)]):
            s.set_eos(b, None)
        s.due()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sched-every", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixedbench.txt"))
    args = ap.parse_args()
    dev = "cuda:0"
    cfg, seed = synth.FULL_CFG, 1234
    d = cfg["d_model"]
    model, _ = build_model(cfg, seed, dev)
    reqs = []
    for i in range(N):
        cond = synth.conditioning(seed + i, "servebench.cond", 2, LENGTHS[i], d).to(dev)
        reqs.append(GenRequest(cond[:1].contiguous() if UNGUIDED[i] else cond, sampling_params=dict(temperature=0.0), cfg_scale=1.0 if UNGUIDED[i] else 2.0,
                               max_new_tokens=BUDGETS[i]))
    guided = [i for i in range(N) if not UNGUIDED[i]]
    unguided = [i for i in range(N) if UNGUIDED[i]]
    eng = model.engine(SLOTS)
    eng.call("zn_debug_eos_bias", float("-inf"))
    frames = sum(BUDGETS)

    def session(indices, slots, kind):
        stats = {}
        got = {r.index: r.codes.shape[2] for r in model.serve(iter([reqs[i] for i in indices]), slots=slots, max_prompt=max(LENGTHS), max_new_tokens=max(BUDGETS),
                                                              guided=kind, sched_every=args.sched_every, _stats=stats)}
        assert [got[k] for k in range(len(indices))] == [BUDGETS[i] for i in indices]
        return stats

    def mixed():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = session(list(range(N)), ROWS, None)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, st["steps"], st["admissions"]

    def split():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sg = session(guided, SLOTS, True)
        su = session(unguided, SLOTS, False)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, (sg["steps"], su["steps"]), sg["admissions"] + su["admissions"]

    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)
    needs = [1 if UNGUIDED[i] else 2 for i in range(N)]
    exp_mixed = expected_steps(list(range(N)), ROWS, args.sched_every, needs)
    exp_split = (expected_steps(guided, SLOTS, args.sched_every, [1] * N), expected_steps(unguided, SLOTS, args.sched_every, [1] * N))
    mixed()                                                    # warm-up of each session's graphs and scratch cache
    split()
    tm, tsp, m_steps, s_steps, m_adm, s_adm = [], [], None, None, None, None
    for _ in range(args.reps):                                 # alternated
        t, m_steps, m_adm = mixed()
        tm.append(t)
        t, s_steps, s_adm = split()
        tsp.append(t)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    m_ms = sorted(1e3 * t / m_steps for t in tm)
    s_ms = sorted(1e3 * t / sum(s_steps) for t in tsp)
    emit(dict(case="mixed", rows=ROWS, sched_every=args.sched_every, steps_expected=exp_mixed, steps_measured=m_steps, admissions=m_adm,
              wall_s_all=[round(t, 4) for t in tm], audio_s_per_s=round(frames / FPS / med(tm), 2), ms_per_step_median=round(med(m_ms), 4),
              ms_per_step_all=[round(x, 4) for x in m_ms]))
    emit(dict(case="split", slots=SLOTS, sched_every=args.sched_every, steps_expected=list(exp_split), steps_measured=list(s_steps), admissions=s_adm,
              wall_s_all=[round(t, 4) for t in tsp], audio_s_per_s=round(frames / FPS / med(tsp), 2), ms_per_step_median=round(med(s_ms), 4),
              ms_per_step_all=[round(x, 4) for x in s_ms]))
    counters = {f"engine_max_rows_{eng.max_rows}": eng.counters()}
    emit(dict(summary=dict(frames=frames, audio_s=round(frames / FPS, 1), mixed_steps=m_steps, split_steps=sum(s_steps),
                           weight_passes_saved=round(1 - m_steps / sum(s_steps), 3), wall_ratio_mixed_over_split=round(med(tm) / med(tsp), 4),
                           mixed_minus_split_ms_per_step=round(med(m_ms) - med(s_ms), 4),
                           steps_as_expected=(m_steps == exp_mixed and tuple(s_steps) == exp_split)), handoff_counters=counters))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# tools/mixedbench.py --reps {args.reps} --sched-every {args.sched_every}\n" + "\n".join(lines) + "\n")
    return 0 if all(x["handoff_timeouts"] == 0 for x in counters.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
