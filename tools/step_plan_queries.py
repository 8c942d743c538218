"""Every output of the six plan queries (zn_mlp_fp8_plan, zn_mamba_fp8_plan, zn_decode_rows_plan, zn_hybrid_rows_plan, zn_kv_fp8_plan, zn_kv_cache_plan), for
comparing two builds of the library: the two outputs must be equal line for line.

    python tools/step_plan_queries.py > RAW.txt
    python tools/step_plan_queries.py fold RAW.txt OUT.txt      # one line per (handle, rows); settings and row counts that answer alike are written once

Handles: a two-layer transformer of Zonos-v0.1 widths and the two-layer full-width hybrid of tests/test_gpu_mamba_fp8.py, each plain and with its FP8 streams
attached (quantize_mlp_fp8 / quantize_mamba_fp8).  Rows 1, 2, 4, 5, 16, 17, 33, 64.  Settings: a fresh engine per line group - the defaults, each of
ZN_TUNE_FP8_SMALL_ROWS 2 / 3, ZN_TUNE_WIDE_ROWS 1, ZN_TUNE_WIDE_HYBRID 1 / 2 / 3, ZN_TUNE_FC1_LN_LAUNCH 2, ZN_TUNE_MLP_FP8 2, ZN_TUNE_MAMBA_FP8 2 alone, some of
them together, and the KV cache modes (zn_set_kv_fp8, zn_set_kv_fp8_only, ZN_TUNE_KV_FP8 2).  A query that refuses prints its error class.  ZONOS_HIP_LIB selects
the library."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS = (1, 2, 4, 5, 16, 17, 33, 64)
QUERIES = (("zn_mlp_fp8_plan", 2), ("zn_mamba_fp8_plan", 2), ("zn_decode_rows_plan", 5), ("zn_hybrid_rows_plan", 7), ("zn_kv_fp8_plan", 2), ("zn_kv_cache_plan", 3))


def settings(L):
    one = [{}, {L.ZN_TUNE_FP8_SMALL_ROWS: 2}, {L.ZN_TUNE_FP8_SMALL_ROWS: 3}, {L.ZN_TUNE_WIDE_ROWS: 1}, {L.ZN_TUNE_WIDE_HYBRID: 1}, {L.ZN_TUNE_WIDE_HYBRID: 2},
           {L.ZN_TUNE_WIDE_HYBRID: 3}, {L.ZN_TUNE_FC1_LN_LAUNCH: 2}, {L.ZN_TUNE_MLP_FP8: 2}, {L.ZN_TUNE_MAMBA_FP8: 2},
           {L.ZN_TUNE_FP8_SMALL_ROWS: 2, L.ZN_TUNE_WIDE_ROWS: 1, L.ZN_TUNE_FC1_LN_LAUNCH: 2}, {L.ZN_TUNE_WIDE_ROWS: 1, L.ZN_TUNE_WIDE_HYBRID: 3},
           {L.ZN_TUNE_FP8_SMALL_ROWS: 2, L.ZN_TUNE_MLP_FP8: 2, L.ZN_TUNE_MAMBA_FP8: 2}]
    out = [(t, (0, 0)) for t in one]
    out += [({}, (1, 0)), ({}, (1, 1)), ({}, (0, 1)), ({L.ZN_TUNE_KV_FP8: 2}, (1, 0)), ({L.ZN_TUNE_KV_FP8: 2}, (1, 1))]
    return out


def dump(name, model):
    from zonos_amd import _lib
    for tune, (kv, kv_only) in settings(_lib):
        eng = model._new_engine(32)
        for k, v in tune.items():
            eng.call("zn_debug_tune", k, v)
        mode = []
        for fn, on in (("zn_set_kv_fp8", kv), ("zn_set_kv_fp8_only", kv_only)):
            if on:
                try:
                    eng.call(fn, 1)
                    mode.append(fn)
                except _lib.ZonosHipError:
                    mode.append(fn + " refused")
        for rows in ROWS:
            got = []
            for q, n in QUERIES:
                out = (C.c_int32 * n)()
                try:
                    eng.call(q, rows, out)
                    got.append("%s %s" % (q[3:], list(out)))
                except _lib.ZonosHipError:
                    got.append("%s refused" % q[3:])
            print(name, "tune", sorted(tune.items()), " ".join(mode), "rows", rows, "|", "; ".join(got), flush=True)


def fold(raw, out):
    blocks = {}      # (handle, the rows' answers) -> settings
    per = {}
    for line in open(raw):
        head, answers = line.rstrip("\n").split(" | ")
        name, rest = head.split(" tune ")
        setting, rows = rest.rsplit(" rows ", 1)
        per.setdefault((name, setting.strip()), []).append((rows, answers.replace("_plan", "").replace(", ", ",")))
    for (name, setting), rows in per.items():
        blocks.setdefault((name, tuple(rows)), []).append(setting)
    with open(out, "w") as f:
        for (name, rows), settings in blocks.items():
            f.write("%s: tune %s\n" % (name, " | ".join(settings)))
            alike = {}
            for r, a in rows:
                alike.setdefault(a, []).append(r)
            for a, rs in alike.items():
                f.write("  rows %s: %s\n" % (" ".join(rs), a))
    print(out, sum(len(v) for v in per.values()), "answers")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "fold":
        fold(sys.argv[2], sys.argv[3])
        sys.exit(0)
    from zonos_amd import synth
    from zonos_amd.testing import build_model
    two = dict(synth.FULL_CFG, n_layer=2)
    wide = dict(synth.HYBRID_FULL_CFG, n_layer=2, attn_layer_idx=[1])
    for name, cfg, quantize in (("transformer", two, None), ("transformer+fp8", two, "quantize_mlp_fp8"), ("hybrid", wide, None), ("hybrid+fp8", wide, "quantize_mamba_fp8")):
        model, _ = build_model(cfg, 7, "cuda:0")
        if quantize:
            getattr(model, quantize)()
        dump(name, model)
