"""Guided (cfg_scale=2) against unguided (cfg_scale=1) generation in one process, alternated, at the Zonos-v0.1 dimensions.

For each batch size B and context (an audio prefix sets where decoding starts) the two settings are timed in turn, `--reps` times
each: ms per decode step = (t(N2) - t(N1)) / (N2 - N1) over two run lengths (prefill and post-processing cancel), aggregate audio
seconds per second = B * N2 / 86.13 / t(N2), and the path that served the steps (zn_decode_path_detail: 2 = whole-step kernel,
1 = per-block chain, 0 = launches).  EOS is suppressed, so every run decodes all its steps.  The hand-off counters of every engine
the model used are printed at the end.  One JSON line per (B, context, setting), then one summary line.

    python tools/cfg1bench.py [--batches 1,2,8,16] [--prefixes 300,1600,3800] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zonos_amd import synth  # noqa: E402
from zonos_amd.testing import build_model  # noqa: E402

FRAME_RATE = 44100 / 512
L_C = 24


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,8,16")
    ap.add_argument("--prefixes", default="300,1600,3800", help="audio prefix lengths: contexts start at L_c + prefix + 1 keys")
    ap.add_argument("--n1", type=int, default=16)
    ap.add_argument("--n2", type=int, default=144)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dev = "cuda:0"
    cfg, seed = synth.FULL_CFG, 1234
    model, _ = build_model(cfg, seed, dev)
    engines = {}
    rows = []

    def run(B, guided, pre, n):
        c = torch.cat([synth.conditioning(seed + i, "cond", 1, L_C, cfg["d_model"]) for i in range(B)], 0).to(dev)
        cond = torch.cat([c, c], 0) if guided else c
        eng = model.engine((cond.shape[0] + 1) // 2)
        engines[id(eng)] = eng
        eng.call("zn_debug_eos_bias", float("-inf"))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.generate(cond, audio_prefix_codes=pre, max_new_tokens=n, cfg_scale=2.0 if guided else 1.0, batch_size=B,
                       sampling_params={"temperature": 0.0})
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dt, int(eng.lib.zn_decode_path_detail(eng.h))

    for B in [int(x) for x in args.batches.split(",")]:
        for P in [int(x) for x in args.prefixes.split(",")]:
            pre = torch.from_numpy(synth.randint(seed, f"cfg1bench.prefix{P}", (B, 9, P), 1024)).to(dev)
            for guided in (True, False):               # warm-up: engines, graphs, workspaces
                run(B, guided, pre, args.n1)
            res = {True: [], False: []}
            for _ in range(args.reps):
                for guided in (True, False):           # alternated
                    t1, _p = run(B, guided, pre, args.n1)
                    t2, path = run(B, guided, pre, args.n2)
                    res[guided].append((t1, t2, path))
            for guided in (True, False):
                ms = sorted(1e3 * (t2 - t1) / (args.n2 - args.n1) for t1, t2, _ in res[guided])
                agg = sorted(B * args.n2 / FRAME_RATE / t2 for _, t2, _ in res[guided])
                r = dict(B=B, rows=2 * B if guided else B, cfg_scale=2.0 if guided else 1.0, ctx_start=L_C + P + 1,
                         ctx_end=L_C + P + 1 + args.n2 + 8, ms_per_step_median=round(ms[len(ms) // 2], 4), ms_per_step_all=[round(x, 4) for x in ms],
                         aggregate_audio_s_per_s=round(agg[len(agg) // 2], 3), path=res[guided][-1][2])
                rows.append(r)
                print(json.dumps(r), flush=True)
    counters = {f"engine_max_rows_{e.max_rows}": e.counters() for e in engines.values()}
    cmp = []
    for r in rows:
        if r["cfg_scale"] == 1.0:
            g = next(x for x in rows if x["B"] == r["B"] and x["ctx_start"] == r["ctx_start"] and x["cfg_scale"] == 2.0)
            cmp.append(dict(B=r["B"], ctx_start=r["ctx_start"], guided_ms=g["ms_per_step_median"], unguided_ms=r["ms_per_step_median"],
                            unguided_not_slower=r["ms_per_step_median"] <= g["ms_per_step_median"],
                            guided_agg=g["aggregate_audio_s_per_s"], unguided_agg=r["aggregate_audio_s_per_s"]))
    print(json.dumps(dict(summary=cmp, handoff_counters=counters)), flush=True)
    return 0 if all(x["handoff_timeouts"] == 0 for x in counters.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
