"""Eight requests with audio prefixes of their own lengths in one `generate_batch(ragged_prefix=True)` call against the same eight
requests with every prefix cut to one shared length on the default path, in one process, alternated, at the Zonos-v0.1 dimensions,
B = 8 guided:

  (a) shared   every prefix cut to PREFIX_SHARED frames: generate_batch(reqs) (the host builds the right-padded prefill rows one by one)
  (b) ragged   prefixes of 0 .. 86 * 3 frames: generate_batch(reqs, ragged_prefix=True) (zn_gen_set_prefix_rows: a column shift per
               row; zn_op_assemble_prefill: the prefill rows in one launch)

For each case, `--reps` times in turn: ms per decode step = (t(N2) - t(N1)) / (N2 - N1) over two run lengths, everything that is not a
decode step (prefill, setup, read-back) = t(N1) - N1 * ms per step.  EOS is suppressed, so every run decodes all its steps.  The
expectations checked against (a) of the same run: (b) costs no more per step than (a) within the spread of (a) against itself across
the repeats (the ragged call attends over more keys in its long rows, fewer in its short ones), and (b)'s time outside the decode steps
is no worse than (a)'s in spite of its longer prefill rows, since one kernel replaces the host's row loop.  One JSON line per case, then one
summary line with the hand-off counters of every engine used (a timeout fails the tool); everything is also written to
profiles/prefixbench.txt.

    python tools/prefixbench.py [--reps 3] [--n1 16] [--n2 144]
"""
import argparse
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

LENGTHS = [16, 19, 23, 26, 30, 33, 37, 40]                # conditioning positions, as tools/raggedbench.py
PREFIXES = [0, 37, 74, 111, 148, 185, 222, 258]           # frames: 0 .. 86 * 3
PREFIX_SHARED = 129                                       # their mean, so that both cases prefill about the same number of valid positions


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n1", type=int, default=16)
    ap.add_argument("--n2", type=int, default=144)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefixbench.txt"))
    args = ap.parse_args()
    dev = "cuda:0"
    cfg, seed = synth.FULL_CFG, 1234
    d, B = cfg["d_model"], len(LENGTHS)
    model, _ = build_model(cfg, seed, dev)
    conds = [synth.conditioning(seed + i, "prefixbench.cond", 2, L, d).to(dev) for i, L in enumerate(LENGTHS)]
    long = [torch.from_numpy(synth.randint(seed + i, "prefixbench.prefix", (1, 9, max(PREFIXES)), 1024)).to(dev) for i in range(B)]

    def requests(prefixes, n):
        return [GenRequest(conds[b], sampling_params=dict(temperature=0.0), cfg_scale=2.0, max_new_tokens=n,
                           audio_prefix_codes=long[b][..., :prefixes[b]] if prefixes[b] else None) for b in range(B)]

    def gen(prefixes, n, ragged):
        reqs = requests(prefixes, n)
        eng = model.engine(B)
        eng.call("zn_debug_eos_bias", float("-inf"))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if ragged:
            model.generate_batch(reqs, ragged_prefix=True)
        else:
            model.generate_batch(reqs)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    cases = {
        "shared": lambda n: gen([PREFIX_SHARED] * B, n, False),
        "ragged": lambda n: gen(PREFIXES, n, True),
    }
    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)
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
        out[k] = dict(case=k, B=B, lengths=LENGTHS, prefixes=PREFIXES if k == "ragged" else [PREFIX_SHARED] * B,
                      ms_per_step_median=round(ms[len(ms) // 2], 4), ms_per_step_all=[round(x, 4) for x in ms],
                      non_step_ms_median=round(rest[len(rest) // 2], 3), non_step_ms_all=[round(x, 3) for x in rest])
        emit(out[k])
    a, b = out["shared"], out["ragged"]
    spread = round(a["ms_per_step_all"][-1] - a["ms_per_step_all"][0], 4)
    eng = model.engine(B)
    counters = {f"engine_max_rows_{eng.max_rows}": eng.counters()}
    emit(dict(summary=dict(shared_ms_per_step=a["ms_per_step_median"], ragged_ms_per_step=b["ms_per_step_median"], shared_spread_ms=spread,
                           ragged_minus_shared_ms=round(b["ms_per_step_median"] - a["ms_per_step_median"], 4),
                           ragged_no_slower_per_step_within_spread=b["ms_per_step_median"] <= a["ms_per_step_median"] + spread,
                           shared_non_step_ms=a["non_step_ms_median"], ragged_non_step_ms=b["non_step_ms_median"],
                           ragged_non_step_no_worse=b["non_step_ms_median"] <= a["non_step_ms_median"]),
              handoff_counters=counters))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(f"# tools/prefixbench.py --reps {args.reps} --n1 {args.n1} --n2 {args.n2}\n" + "\n".join(lines) + "\n")
    return 0 if all(x["handoff_timeouts"] == 0 for x in counters.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
