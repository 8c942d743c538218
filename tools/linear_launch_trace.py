"""The ordered kernel launches of the small-M linear dispatch (zn_linear_plan.h), for comparing two builds of the library.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/linear_launch_trace.py
    python tools/linear_launch_trace.py list DIR OUT.txt      # DIR's kernel trace -> one "name grid=(..) wg=(..)" line per launch of this library (argument types dropped), in start order, repeated blocks folded

Without arguments: a few greedy frames with one launch per op (ZN_TUNE_PERSISTENT = 2) at Zonos-v0.1 dimensions - batch 1 guided (2 rows)
and unguided (1 row), batch 3 (6 rows, 48-row prefill), batch 8 (16 rows, 64-row prefill), batch 17 (34 rows: the wide plan), prefills of 120 and 400
rows - then the same row counts on the tiny hybrid model and on the d_model 512 chain model; a two-layer transformer of the same widths with quantize_mlp_fp8() at
6 rows, and at 2 rows with set_fp8_small_rows(True); the two-layer full-width hybrid of tests/test_gpu_mamba_fp8.py, plain and with quantize_mamba_fp8(), at 2, 6
and 34 rows.  Every transformer engine applies out_proj twice (double_out_proj), so each transformer case traces that linear too.  ZONOS_HIP_LIB selects the library."""
import csv
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(cfg, seed, cases, prepare=None, label=""):
    import torch
    from zonos_amd import _lib, synth
    from zonos_amd.testing import build_model
    model, _ = build_model(cfg, seed, "cuda:0")
    if prepare:
        prepare(model)      # (quantising drops the cached engines: before the one below exists)
    model.engine(max(8, max(B for B, _, _ in cases))).call("zn_debug_tune", _lib.ZN_TUNE_PERSISTENT, 2)
    for B, scale, S in cases:
        rows = B if scale == 1.0 else 2 * B
        cond = synth.conditioning(seed, "cond%d_%d" % (rows, S), rows, S, cfg["d_model"]).to("cuda:0")
        out = model.generate(cond, max_new_tokens=10, cfg_scale=scale, batch_size=B, sampling_params={"temperature": 0.0})
        torch.cuda.synchronize()
        print("case", label, "d_model", cfg["d_model"], "batch", B, "cfg_scale", scale, "conditioning", S, "-> codes checksum", int(out.sum()), flush=True)


def listing(d, out):
    fs = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    assert len(fs) == 1, fs
    rows = list(csv.DictReader(open(fs[0])))
    rows.sort(key=lambda r: (int(r["Start_Timestamp"]), int(r.get("Dispatch_Id", 0))))
    gk = [k for k in rows[0] if k.startswith("Grid_Size")]
    wk = [k for k in rows[0] if k.startswith("Workgroup_Size")]
    # this library's launches only (PyTorch's and the runtime's copy / fill kernels say nothing about the dispatch)
    rows = [r for r in rows if "at::" not in r["Kernel_Name"] and not r["Kernel_Name"].startswith("__amd_rocclr")]
    lines = ["%s grid=(%s) wg=(%s)" % (re.sub(r"\(.*\)$", "", r["Kernel_Name"].replace("void ", "", 1)), ",".join(r[k] for k in gk), ",".join(r[k] for k in wk)) for r in rows]

    def fold(seq):      # blocks repeated back to back (the layers of a step, the steps of a run) are written once: "repeat K {" ... "}", nested
        out_, i = [], 0
        while i < len(seq):
            best_l, best_k = 1, 1
            for l in range(1, 600):
                k = 1
                while seq[i + k * l:i + (k + 1) * l] == seq[i:i + l]:
                    k += 1
                if k > 1 and l * k > best_l * best_k:
                    best_l, best_k = l, k
            block = seq[i:i + best_l]
            if best_k > 1:
                inner = fold(block) if best_l > 1 else block
                out_.append("repeat %d {\n%s\n}" % (best_k, "\n".join("  " + x for y in inner for x in y.split("\n"))))
            else:
                out_ += block
            i += best_l * best_k
        return out_
    with open(out, "w") as f:
        f.write("\n".join(fold(lines)) + "\n")
    print(out, len(rows), "launches")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "list":
        listing(sys.argv[2], sys.argv[3])
    else:
        from zonos_amd import synth
        run(synth.FULL_CFG, 1, [(1, 2.0, 6), (1, 1.0, 6), (3, 2.0, 8), (8, 2.0, 4), (17, 2.0, 3), (1, 2.0, 60), (1, 2.0, 200)], label="full")
        run(synth.HYBRID_TINY_CFG, 3, [(1, 2.0, 6), (3, 2.0, 5), (8, 2.0, 4)], label="hybrid tiny")
        run(synth.CHAIN_CFG, 5, [(1, 2.0, 6), (3, 2.0, 8), (8, 2.0, 4)], label="chain")
        two = dict(synth.FULL_CFG, n_layer=2)
        run(two, 7, [(3, 2.0, 8)], lambda m: m.quantize_mlp_fp8(), "fp8 mlp")
        run(two, 7, [(1, 2.0, 6)], lambda m: m.quantize_mlp_fp8(small_rows=True), "fp8 mlp, small rows")
        wide = dict(synth.HYBRID_FULL_CFG, n_layer=2, attn_layer_idx=[1])
        run(wide, 9, [(1, 2.0, 6), (3, 2.0, 5), (17, 2.0, 3)], label="hybrid wide")
        run(wide, 9, [(1, 2.0, 6), (3, 2.0, 5), (17, 2.0, 3)], lambda m: m.quantize_mamba_fp8(), "hybrid wide, fp8 mamba")
