"""Weight-only FP8 for fc1 / fc2 (Zonos.quantize_mlp_fp8) against the bf16 stream of the SAME weights, at the Zonos-v0.1
dimensions with seeded synthetic weights, in one process and one quantised model:

  steps     a decode step at 8 utterances (16 rows) and at 4 (8 rows), guided, greedy, EOS suppressed: wall time of generate() at two lengths,
            their difference per step, median over the repetitions - with the stream on, and with zn_debug_tune(ZN_TUNE_MLP_FP8, 2): the same
            build, weights and codes, every launch reading the bf16 copy.  That is the baseline.
  launches  fc1 (LayerNorm from handed-over statistics + SiLU gate) and fc2 (+ residual) at 16 rows, per launch between HIP events, through
            zn_op_linear_fp8 and zn_op_linear_fused, cycling through the 26 layers' weights (1.7 / 0.9 GB: no launch finds its weights cached);
            medians and bytes per launch.
  quality   report only: the largest teacher-forced |dlogit| of the quantised model against its own unquantised copy over the steps of a
            batch-1 generation, beside the reference's own thread-count spread (tests/golden/ref_thread_sensitivity.json).  Synthetic weights:
            this says nothing about audio quality on a real checkpoint.

    python tools/fp8bench.py [--reps 20] [--tf-steps 48]

One JSON line per figure; everything is also written to profiles/fp8bench.txt."""
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


def generate(model, batch, steps, seed=500, hook=None):
    d = model.config.backbone.d_model
    cond = torch.cat([synth.conditioning(seed + i, "fp8bench.cond", 2, 24, d) for i in range(batch)], 0)
    cond = torch.cat([cond[0::2], cond[1::2]], 0).to(DEV)
    tr = {"logits": []} if hook else None
    if hook:
        tr["after_step"] = hook
    t0 = time.perf_counter()
    out = model.generate(cond, max_new_tokens=steps, cfg_scale=2.0, batch_size=batch, sampling_params=GREEDY, _trace=tr)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out, tr


def step_ms(model, batch, reps, short=40, long=168):
    generate(model, batch, short)                       # warm-up: engine, graphs
    generate(model, batch, long)
    per = []
    for _ in range(reps):
        a, b = generate(model, batch, short)[0], generate(model, batch, long)[0]
        per.append((b - a) / (long - short) * 1e3)
    return statistics.median(per), min(per), max(per)


def launch_us(eng, layers, which, fp8, reps):
    """Median microseconds of one fc1 / fc2 launch at 16 rows over reps passes through the layers."""
    d, F, rows = 2048, 8192, 16
    st = _lib.stream_ptr()
    x = synth.conditioning(7, "fp8bench.x", 1, rows, d)[0].to(DEV).contiguous()
    m = synth.conditioning(8, "fp8bench.m", 1, rows, F)[0].to(DEV).contiguous()
    res = x.clone()
    o_fc1 = torch.empty(rows, F, dtype=torch.bfloat16, device=DEV)
    o_x = torch.empty(rows, d, dtype=torch.bfloat16, device=DEV)
    o_fc2 = torch.empty(rows, d, dtype=torch.bfloat16, device=DEV)
    l0 = layers[0]
    # fc1 normalises from the statistics the projection in front of it leaves: run that projection once (as zn_bench_kernel does)
    pre = _lib.zn_linear_op(pro=0, epi=1, rows=rows, N=d, K=d, target_blocks=512, want_ln_stats_out=1, x=x.data_ptr(), W=l0.mixer.out_proj.weight.data_ptr(),
                            resid=res.data_ptr(), out=o_x.data_ptr())
    eng.call("zn_op_linear_fused", C.byref(pre), st)
    assert pre.plan_dict()["writes_ln_stats"] == 1
    times, plan = [], None
    # the launches are enqueued behind ~0.1 s of matrix products, so that the device never waits for the host between two events
    big = torch.empty(8192, 8192, dtype=torch.bfloat16, device=DEV).normal_()
    for _ in range(64):
        big @ big
    for rep in range(reps + 2):
        for blk in layers:
            if which == "fc1":
                op = _lib.zn_linear_op(pro=1, epi=2, rows=rows, N=2 * F, K=d, target_blocks=512, ln_stats_in=1, x=o_x.data_ptr(), W=blk.mlp.fc1.weight.data_ptr(),
                                       ln_w=blk.norm2.weight.data_ptr(), ln_b=blk.norm2.bias.data_ptr(), out=o_fc1.data_ptr())
                qe = (blk.mlp.fc1_q, blk.mlp.fc1_exp)
            else:
                op = _lib.zn_linear_op(pro=0, epi=1, rows=rows, N=d, K=F, target_blocks=1024, x=m.data_ptr(), W=blk.mlp.fc2.weight.data_ptr(), resid=res.data_ptr(),
                                       out=o_fc2.data_ptr())
                qe = (blk.mlp.fc2_q, blk.mlp.fc2_exp)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if fp8:
                eng.call("zn_op_linear_fp8", C.byref(op), qe[0].data_ptr(), qe[1].data_ptr(), st)
            else:
                eng.call("zn_op_linear_fused", C.byref(op), st)
            e1.record()
            if rep >= 2:                                  # two warm-up passes
                times.append((e0, e1))
            plan = op.plan_dict()
    torch.cuda.synchronize()
    us = [a.elapsed_time(b) * 1e3 for a, b in times]
    assert plan["kernel"] == "GEMM16S" and plan["w8"] == int(fp8), plan
    return statistics.median(us), min(us), len(us), plan


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tf-steps", type=int, default=48)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8bench.txt"))
    args = ap.parse_args()
    lines = []

    def emit(**kw):
        s = json.dumps(kw)
        print(s, flush=True)
        lines.append(s)
    model, _ = build_model(synth.FULL_CFG, 1234, DEV)
    layers = list(model.backbone.layers)
    # ---- quality (report only): the unquantised model's own trajectory first, then the quantised model forced along it
    rec = {}

    def record(step_idx, delayed, col):
        rec[step_idx] = delayed[:, :, col].clone()
    eng1 = model.engine(1)
    eng1.call("zn_debug_eos_bias", float("-inf"))
    _, _, tr_u = generate(model, 1, args.tf_steps, hook=record)
    before = layers[0].mlp.fc1.weight.data.float().clone()
    model.quantize_mlp_fp8()
    after = layers[0].mlp.fc1.weight.data.float()
    scale = torch.exp2(layers[0].mlp.fc1_exp.float())[:, None]
    normal = before.abs() >= 2.0 ** -6 * scale                        # scaled magnitudes in E4M3's normal range: the 2^-4 |w| bound is theirs
    rel = ((after - before).abs() / before.abs().clamp(min=1e-30))[normal].max().item()
    sub = ((after - before).abs() / scale)[~normal].max().item()

    def force(step_idx, delayed, col):
        if step_idx in rec:
            delayed[:, :, col] = rec[step_idx]
    eng1 = model.engine(1)
    eng1.call("zn_debug_eos_bias", float("-inf"))
    _, _, tr_q = generate(model, 1, args.tf_steps, hook=force)
    n = min(len(tr_u["logits"]), len(tr_q["logits"]))
    dl = [float((tr_u["logits"][i].float() - tr_q["logits"][i].float()).abs().max()) for i in range(n)]
    with open(os.path.join(ROOT, "tests", "golden", "ref_thread_sensitivity.json")) as f:
        spread = float(json.load(f)["heads"]["gaussian"]["largest_tf_abs_dlogit"])
    emit(figure="quality_report_only", teacher_forced_steps=n, max_abs_dlogit_fp8_vs_own_unquantised=max(dl), prefill_abs_dlogit=dl[0],
         reference_thread_count_spread_max_abs_dlogit=spread, layer0_fc1_max_rel_weight_error_normal_range=rel, bound=2.0 ** -4,
         layer0_fc1_max_abs_error_over_row_scale_subnormal_range=sub, bound_subnormal=2.0 ** -10,
         note="synthetic weights; no audio-quality claim")
    # ---- steps
    for batch in (8, 4):
        eng = model.engine(batch)
        eng.call("zn_debug_eos_bias", float("-inf"))
        for mode, tune in (("fp8", 1), ("bf16", 2)):
            eng.call("zn_debug_tune", _lib.ZN_TUNE_MLP_FP8, tune)
            plan = eng.mlp_fp8_plan(2 * batch)
            med, lo, hi = step_ms(model, batch, args.reps)
            emit(figure="step", utterances=batch, rows=2 * batch, mlp_stream=mode, reads_fp8=plan, ms_per_step_median=round(med, 4), min=round(lo, 4), max=round(hi, 4),
                 reps=args.reps)
        eng.call("zn_debug_tune", _lib.ZN_TUNE_MLP_FP8, 1)
    # ---- launches
    eng = model.engine(8)
    for which, nbytes in (("fc1", 2 * 8192 * 2048), ("fc2", 2048 * 8192)):
        for fp8 in (True, False):
            med, lo, cnt, plan = launch_us(eng, layers, which, fp8, args.reps)
            wbytes = nbytes * (1 if fp8 else 2) + (nbytes // (2048 if which == "fc1" else 8192) if fp8 else 0)
            emit(figure="launch", op=which, rows=16, stream="fp8" if fp8 else "bf16", us_median=round(med, 2), us_min=round(lo, 2), launches=cnt, weight_bytes=wbytes,
                 tb_per_s=round(wbytes / med / 1e6, 3), nwv=plan["nwv"], groups=plan["groups"], ksplit=plan["ksplit"], lnp=plan["lnp"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("python tools/fp8bench.py --reps %d --tf-steps %d\n" % (args.reps, args.tf_steps) + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
