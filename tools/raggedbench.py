"""One generate() call over utterances of different prompt lengths (`conditioning_lengths`) against the uniform batch and against solo
runs, in one process, alternated, at the Zonos-v0.1 dimensions, B = 8 guided:

  (a) uniform  eight utterances of L_c = 40 in one call (no lengths: zn_prefill)
  (b) ragged   eight utterances of 16 .. 40 conditioning positions in one call (right-padded: zn_prefill_rows)
  (c) solo     the eight utterances of (b), one generate(batch_size=1) call each, summed

For each case, `--reps` times in turn: ms per decode step = (t(N2) - t(N1)) / (N2 - N1) over two run lengths, everything that is not a
decode step (prefill, setup, read-back) = t(N1) - N1 * ms per step, aggregate audio seconds per second = 8 * N2 / 86.13 / t(N2).  EOS is
suppressed, so every run decodes all its steps.  The expectation checked: (b) costs no more per step than (a) - the same launches over
fewer keys - within the spread of (a) against itself across the repeats; both figures are printed.  One JSON line per case, then one
summary line with the hand-off counters of every engine used (a timeout fails the tool).

    python tools/raggedbench.py [--reps 3] [--n1 16] [--n2 144]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zonos_amd import synth  # noqa: E402
from zonos_amd.conditioning import pad_conditionings  # noqa: E402
from zonos_amd.testing import build_model  # noqa: E402

FRAME_RATE = 44100 / 512
L_UNIFORM = 40
LENGTHS = [16, 19, 23, 26, 30, 33, 37, 40]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n1", type=int, default=16)
    ap.add_argument("--n2", type=int, default=144)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dev = "cuda:0"
    cfg, seed = synth.FULL_CFG, 1234
    d, B = cfg["d_model"], len(LENGTHS)
    model, _ = build_model(cfg, seed, dev)
    engines = {}
    uniform = [synth.conditioning(seed + i, "raggedbench.cond", 2, L_UNIFORM, d) for i in range(B)]
    utts = [u[:, :L].contiguous() for u, L in zip(uniform, LENGTHS)]             # (b), (c): the same utterances cut to their lengths
    cond_a = torch.cat([u[0:1] for u in uniform] + [u[1:2] for u in uniform], 0).to(dev)
    cond_b, lens_b = pad_conditionings(utts, 2.0)
    cond_b = cond_b.to(dev)
    solo = [u.to(dev) for u in utts]

    def gen(cond, b, n, lengths=None):
        eng = model.engine(b)
        engines[id(eng)] = eng
        eng.call("zn_debug_eos_bias", float("-inf"))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.generate(cond, max_new_tokens=n, cfg_scale=2.0, batch_size=b, sampling_params={"temperature": 0.0}, conditioning_lengths=lengths)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    cases = {
        "uniform": lambda n: gen(cond_a, B, n),
        "ragged": lambda n: gen(cond_b, B, n, lens_b),
        "solo": lambda n: sum(gen(c, 1, n) for c in solo),
    }
    for run in cases.values():                         # warm-up: engines, graphs, workspaces
        run(args.n1)
    res = {k: [] for k in cases}
    for _ in range(args.reps):
        for k, run in cases.items():                   # alternated
            res[k].append((run(args.n1), run(args.n2)))
    out = {}
    for k, v in res.items():
        ms = sorted(1e3 * (t2 - t1) / (args.n2 - args.n1) for t1, t2 in v)
        rest = sorted(1e3 * t1 - args.n1 * 1e3 * (t2 - t1) / (args.n2 - args.n1) for t1, t2 in v)
        agg = sorted(B * args.n2 / FRAME_RATE / t2 for _, t2 in v)
        out[k] = dict(case=k, B=B, calls=1 if k != "solo" else B, lengths=[L_UNIFORM] * B if k == "uniform" else LENGTHS,
                      ms_per_step_median=round(ms[len(ms) // 2], 4), ms_per_step_all=[round(x, 4) for x in ms],
                      prefill_and_setup_ms_median=round(rest[len(rest) // 2], 3), prefill_and_setup_ms_all=[round(x, 3) for x in rest],
                      aggregate_audio_s_per_s=round(agg[len(agg) // 2], 3))
        print(json.dumps(out[k]), flush=True)
    a, b, c = out["uniform"], out["ragged"], out["solo"]
    spread = round(a["ms_per_step_all"][-1] - a["ms_per_step_all"][0], 4)
    counters = {f"engine_max_rows_{e.max_rows}": e.counters() for e in engines.values()}
    print(json.dumps(dict(summary=dict(uniform_ms_per_step=a["ms_per_step_median"], ragged_ms_per_step=b["ms_per_step_median"],
                                       uniform_spread_ms=spread, ragged_minus_uniform_ms=round(b["ms_per_step_median"] - a["ms_per_step_median"], 4),
                                       ragged_no_slower_than_uniform_within_spread=b["ms_per_step_median"] <= a["ms_per_step_median"] + spread,
                                       ragged_audio_s_per_s=b["aggregate_audio_s_per_s"], solo_audio_s_per_s=c["aggregate_audio_s_per_s"],
                                       ragged_over_solo=round(b["aggregate_audio_s_per_s"] / c["aggregate_audio_s_per_s"], 3)),
                          handoff_counters=counters)), flush=True)
    return 0 if all(x["handoff_timeouts"] == 0 for x in counters.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
