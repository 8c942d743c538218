"""Eight requests with eight different parameter sets in one `generate_batch()` call against the same eight utterances through
`generate(batch_size=8)` with one shared set, in one process, alternated, at the Zonos-v0.1 dimensions, guided:

  (a) shared    generate(batch_size=8, conditioning_lengths=...): temperature 1.0, min_p 0.1, cfg_scale 2.0 for every row, no table
  (b) requests  generate_batch of eight GenRequests: greedy rows, plain and min_p sampling, top-k / top-p rows (they sort), the unified
                sampler, repetition penalties 1 .. 5 over windows 2 .. 8, cfg_scale 1.5 .. 4, eight seeds (zn_gen_set_rows: every
                sampler workgroup loads its row's 64-byte entry)

Both run every request for the same number of frames (EOS suppressed, one max_new_tokens), so the per-step times compare the sampler
launch with and without the table: ms per decode step = (t(N2) - t(N1)) / (N2 - N1) over two run lengths, `--reps` times in turn.  One
JSON line per case, then a summary line with the measured ratio (b) / (a), the spread of (a) against itself across the repeats and the
hand-off counters (a timeout fails the tool).

    python tools/requestbench.py [--reps 3] [--n1 16] [--n2 144]
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
from zonos_amd.model import GenRequest  # noqa: E402
from zonos_amd.testing import build_model  # noqa: E402

LENGTHS = [16, 19, 23, 26, 30, 33, 37, 40]
SHARED = dict(temperature=1.0, min_p=0.1)
SETS = [
    (dict(temperature=0.0), 2.0),
    (dict(temperature=0.0, repetition_penalty=5.0, repetition_penalty_window=8), 3.0),
    (dict(temperature=1.0, min_p=0.1), 2.0),
    (dict(temperature=0.8, repetition_penalty=1.0), 1.5),
    (dict(temperature=0.9, top_k=40, top_p=0.8), 2.5),
    (dict(temperature=1.1, top_p=0.9, repetition_penalty=2.0, repetition_penalty_window=4), 4.0),
    (dict(temperature=1.2, min_p=0.1, linear=0.7, conf=0.3, quad=0.1), 2.0),
    (dict(temperature=1.3, top_k=100, min_p=0.05, linear=0.5, conf=0.4), 1.75),
]


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
    utts = [synth.conditioning(seed + i, "requestbench.cond", 2, L, d).to(dev) for i, L in enumerate(LENGTHS)]
    cond, lens = pad_conditionings(utts, 2.0)
    eng = model.engine(B)

    def timed(fn):
        eng.call("zn_debug_eos_bias", float("-inf"))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        eng.call("zn_debug_eos_bias", 0.0)
        return time.perf_counter() - t0

    def shared(n):
        return timed(lambda: model.generate(cond, max_new_tokens=n, cfg_scale=2.0, batch_size=B, sampling_params=SHARED, seed=7,
                                            conditioning_lengths=lens))

    def requests(n):
        reqs = [GenRequest(utts[i], sampling_params=sp, seed=100 + i, cfg_scale=scale, max_new_tokens=n) for i, (sp, scale) in enumerate(SETS)]
        return timed(lambda: model.generate_batch(reqs))

    cases = {"shared": shared, "requests": requests}
    for run in cases.values():                         # warm-up: engine, graphs, workspaces
        run(args.n1)
    res = {k: [] for k in cases}
    for _ in range(args.reps):
        for k, run in cases.items():                   # alternated
            res[k].append((run(args.n1), run(args.n2)))
    out = {}
    for k, v in res.items():
        ms = sorted(1e3 * (t2 - t1) / (args.n2 - args.n1) for t1, t2 in v)
        rest = sorted(1e3 * t1 - args.n1 * 1e3 * (t2 - t1) / (args.n2 - args.n1) for t1, t2 in v)
        out[k] = dict(case=k, B=B, lengths=LENGTHS, ms_per_step_median=round(ms[len(ms) // 2], 4), ms_per_step_all=[round(x, 4) for x in ms],
                      prefill_and_setup_ms_median=round(rest[len(rest) // 2], 3))
        print(json.dumps(out[k]), flush=True)
    a, b = out["shared"], out["requests"]
    counters = eng.counters()
    print(json.dumps(dict(summary=dict(shared_ms_per_step=a["ms_per_step_median"], requests_ms_per_step=b["ms_per_step_median"],
                                       requests_over_shared=round(b["ms_per_step_median"] / a["ms_per_step_median"], 4),
                                       shared_spread_ms=round(a["ms_per_step_all"][-1] - a["ms_per_step_all"][0], 4),
                                       requests_spread_ms=round(b["ms_per_step_all"][-1] - b["ms_per_step_all"][0], 4)),
                          handoff_counters=counters)), flush=True)
    return 0 if counters["handoff_timeouts"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
