"""Decode steps of 17..64 rows read every weight matrix once per step (the wide plan: ZN_TUNE_WIDE_ROWS) and compute the bits of the
grouped path, which streams the weights once per 16 rows.  The bar is equality of the raw bits - int16 / int32 views, torch.equal - between
zn_debug_tune(ZN_TUNE_WIDE_ROWS, 2) (per op) or the default (generation) and ZN_TUNE_WIDE_ROWS = 1:
  1. gemm16w_kernel against gemm16s_kernel in groups of 16 over linear_cases_gemm16s()'s shapes (one slice and split-K 2 / 8 / 16, the statistics
     orders of 32- and 64-row workgroups, the clamped edges N = 96 and N = 16416), residual and SiLU gate, at row counts around every row-block
     count and past 64 (65 = 64 + 1, 80 = 64 + 16: the last group is planned by its own size);
  2. out_proj leaving LayerNorm statistics through gemm16k_kernel's row groups, then fc1 normalising from them ahead of the wide kernel;
  3. the FP8 stream, wide against grouped and against the bf16 launch on the dequantised weights;
  4. gemm16k_kernel's row groups in a decode step: split + RoPE + KV append (positions 0, capacity - 1 and capacity; the cache's canary row) and
     the fp32 epilogue of the heads, a LayerNorm launch and the LayerNorm prologue in front;
  5. generate(), generate_batch() and a mixed serve() session on a two-block model of the production widths, bf16 and FP8;
  6. zn_decode_rows_plan: the step really is planned wide."""
import ctypes as C

import pytest
import torch

from zonos_amd import _lib, synth
from zonos_amd import testing as T
from zonos_amd.backbone import HipEngine
from zonos_amd.model import GenRequest
from zonos_amd.testing import LF_F32, LF_PRO_LN, LF_PRO_NONE, LF_RESID, LF_ROPE_KV, LF_SILU, LF_STORE, LinearCase, build_model, linear_case_tensors

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD, CANARY = 2, 768.0
bf = torch.bfloat16
E2E_CFG = dict(d_model=2048, n_layer=2, num_heads=16, num_heads_kv=4, d_ff=8192)
GROUPED, WIDE = 1, 2
ROWS = (17, 31, 32, 33, 48, 49, 64, 65, 80)


def bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def tiles_of(rows):
    return (min(rows, 64) + 15) // 16


@pytest.fixture(scope="module")
def eng():
    model, _ = build_model(dict(d_model=2048, n_layer=1, num_heads=16, num_heads_kv=4, d_ff=256), 31, DEV)
    e = HipEngine(model.backbone, max_rows=128)
    e._model = model
    return e


class Guarded:
    """[PAD canary rows | rows x cols of NaN | PAD canary rows]"""

    def __init__(self, rows, cols, dtype=bf):
        self.buf = torch.full((rows + 2 * PAD, cols), CANARY, dtype=dtype, device=DEV)
        self.view = self.buf[PAD:PAD + rows]
        self.view.fill_(float("nan"))

    def check(self, label):
        b = self.buf.float().cpu()
        assert bool((b[:PAD] == CANARY).all()) and bool((b[-PAD:] == CANARY).all()), f"{label}: a canary row was overwritten"
        assert bool(torch.isfinite(b[PAD:-PAD]).all()), f"{label}: elements never written (or not finite)"
        return self.view.cpu()


def run_op(eng, c: LinearCase, mode, dev, W=None, fp8=None, want_stats=False, stats_in=False, kv=None, lengths=None):
    """The case through zn_op_linear_fused (fp8 = (q, exp): zn_op_linear_fp8) under ZN_TUNE_WIDE_ROWS = mode: ({name: output rows on the CPU}, plan)."""
    op = _lib.zn_linear_op(pro=c.pro, epi=c.epi, rows=c.rows, N=c.N, K=c.K, target_blocks=4, want_ln_stats_out=int(want_stats), ln_stats_in=int(stats_in))
    for k in ("x", "W", "ln_w", "ln_b", "resid"):
        if k in dev:
            setattr(op, k, dev[k].data_ptr())
    if W is not None:
        op.W = W.data_ptr()
    outs = {}
    if c.epi in (LF_STORE, LF_RESID, LF_SILU):
        outs["out"] = Guarded(c.rows, c.N // 2 if c.epi == LF_SILU else c.N)
        op.out = outs["out"].view.data_ptr()
    if c.epi == LF_F32:
        outs["out_f32"] = Guarded(c.rows, c.N, torch.float32)
        op.out_f32 = outs["out_f32"].view.data_ptr()
    if c.epi == LF_ROPE_KV:
        outs["q_out"] = Guarded(c.rows, 2048)
        op.kv, op.q_out, op.max_len, op.lengths = kv.data_ptr(), outs["q_out"].view.data_ptr(), T.LF_MAX_LEN, lengths.data_ptr()
    try:
        for key, val in c.tune:
            eng.call("zn_debug_tune", getattr(_lib, key), val)
        eng.call("zn_debug_tune", _lib.ZN_TUNE_WIDE_ROWS, mode)
        for _ in range(2 if c.twice else 1):                       # split-K twice on one handle: the arrival tickets must be back at zero
            for g in outs.values():
                g.view.fill_(float("nan"))
            if fp8 is not None:
                eng.call("zn_op_linear_fp8", C.byref(op), fp8[0].data_ptr(), fp8[1].data_ptr(), _lib.stream_ptr())
            else:
                eng.call("zn_op_linear_fused", C.byref(op), _lib.stream_ptr())
            torch.cuda.synchronize()
    finally:
        for key, _ in c.tune:
            eng.call("zn_debug_tune", getattr(_lib, key), 1)
        eng.call("zn_debug_tune", _lib.ZN_TUNE_WIDE_ROWS, GROUPED)
    plan = op.plan_dict()
    assert plan["err"] == 0, (c.label, plan)
    for k, v in c.expect:
        assert plan[k] == v, f"{c.label}: plan {k} = {plan[k]}, the case is about {v} ({plan})"
    return {k: g.check(f"{c.label} mode {mode}") for k, g in outs.items()}, plan


def check_plans(c, pg, pw, wide_form=True):
    """Grouped: 16 rows per launch, one row tile.  Wide: 64 and ceil(min(rows, 64) / 16); every other field unchanged."""
    assert pg["row_tiles"] == 1 and pg["rows_per_launch"] == 16, (c.label, pg)
    if wide_form:
        assert pw["row_tiles"] == tiles_of(c.rows) and pw["rows_per_launch"] == 64, (c.label, pw)
    else:
        assert pw["row_tiles"] == 1 and pw["rows_per_launch"] == 16, (c.label, pw)
    skip = ("row_tiles", "rows_per_launch")
    assert {k: v for k, v in pg.items() if k not in skip} == {k: v for k, v in pw.items() if k not in skip}, (c.label, pg, pw)


def same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        bad = bits(a[k]) != bits(b[k])
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements of {k} differ; first at {bad.nonzero()[0].tolist()}"


def to_dev(t):
    return {k: v.to(DEV).contiguous() for k, v in t.items()}


def gemm16s_cases(rows):
    out = [c._replace(rows=rows) for c in T.linear_cases_gemm16s() if c.rows == 5 and c.pro == LF_PRO_NONE and c.epi in (LF_RESID, LF_SILU)]
    assert len(out) == 12 and {dict(c.expect)["nwv"] for c in out} == {2, 4} and {dict(c.expect)["ksplit"] for c in out} == {1, 2, 8, 16}
    assert {c.N for c in out} >= {96, 16416}
    return out


# ---------------------------------------------------------------------------------------------- 1. per op: the wide kernel against groups of 16
@pytest.mark.parametrize("rows", ROWS)
def test_wide_kernel_equals_groups_of_16(eng, rows):
    for c in gemm16s_cases(rows):
        t = linear_case_tensors(c)
        x = t["x"].float()
        assert len({tuple(r[:8].tolist()) for r in x}) == rows and float(x[-1].std()) > 2 * float(x[0].std()), "activation rows: pairwise distinct, row-scaled"
        dev = to_dev(t)
        og, pg = run_op(eng, c, GROUPED, dev)
        ow, pw = run_op(eng, c, WIDE, dev)
        check_plans(c, pg, pw)
        same_bits(og, ow, c.label)


# ---------------------------------------------------------------------------------------------- 2. the statistics hand-over
@pytest.mark.parametrize("rows", [24, 33, 64])
def test_fc1_behind_statistics_left_through_row_groups(eng, rows):
    orders = set()
    for N, nwv, _, _ in T.LF_PAIR_FC1:
        out, fc1 = T.linear_cases_pair(rows, N)
        d_out = to_dev(linear_case_tensors(out))
        res = {}
        for mode in (GROUPED, WIDE):
            x1, p_out = run_op(eng, out, mode, d_out, want_stats=True)
            y, p_fc1 = run_op(eng, fc1, mode, to_dev(linear_case_tensors(fc1, x=x1["out"])), stats_in=True)
            res[mode] = (x1, p_out, y, p_fc1)
        check_plans(out, res[GROUPED][1], res[WIDE][1])
        check_plans(fc1, res[GROUPED][3], res[WIDE][3])
        assert res[WIDE][3]["lnp"] == 1 and res[WIDE][3]["reads_ln_stats"] == 1 and res[WIDE][1]["writes_ln_stats"] == 1
        same_bits(res[GROUPED][0], res[WIDE][0], out.label)
        same_bits(res[GROUPED][2], res[WIDE][2], fc1.label)
        orders.add(nwv)
    assert orders == {2, 4}, "both orders of the tile statistics"


# ---------------------------------------------------------------------------------------------- 3. the FP8 stream
def dev_quantize(eng, W):
    N, K = W.shape
    q = torch.empty((N, K), dtype=torch.uint8, device=DEV)
    e = torch.empty((N,), dtype=torch.int8, device=DEV)
    Wdq = torch.empty_like(W)
    eng.call("zn_op_fp8_quantize_rows", W.data_ptr(), N, K, q.data_ptr(), e.data_ptr(), _lib.stream_ptr())
    eng.call("zn_op_fp8_dequant_rows", q.data_ptr(), e.data_ptr(), N, K, Wdq.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return q, e, Wdq


@pytest.mark.parametrize("rows", [17, 33, 64])
def test_fp8_wide_equals_grouped_and_the_bf16_launch(eng, rows):
    for c in gemm16s_cases(rows):
        dev = to_dev(linear_case_tensors(c))
        # rows of one amax binade would all carry one exponent: scale them by row-dependent powers of two (exact), as tests/test_gpu_fp8.py does
        q, e, Wdq = dev_quantize(eng, dev["W"] * torch.exp2(T.fp8_row_shifts(c.N).float()).to(bf).to(DEV)[:, None])
        assert len(set(e.cpu().tolist())) >= 4 and int(e[0]) != int(e[1]) and int(e[c.N - 1]) != int(e[c.N - 2]), c.label
        o8g, p8g = run_op(eng, c, GROUPED, dev, W=Wdq, fp8=(q, e))
        o8w, p8w = run_op(eng, c, WIDE, dev, W=Wdq, fp8=(q, e))
        obw, pbw = run_op(eng, c, WIDE, dev, W=Wdq)
        assert p8g["w8"] == 1 and p8w["w8"] == 1 and pbw["w8"] == 0
        check_plans(c, p8g, p8w)
        assert {k: v for k, v in p8w.items() if k != "w8"} == {k: v for k, v in pbw.items() if k != "w8"}
        same_bits(o8g, o8w, c.label + " fp8 wide vs grouped")
        same_bits(obw, o8w, c.label + " fp8 wide vs bf16 wide on the dequantised weights")
        del q, e, Wdq


# ---------------------------------------------------------------------------------------------- 4. gemm16k_kernel's row groups in a decode step
@pytest.mark.parametrize("rows", [17, 33, 64])
def test_gemm16k_row_groups_in_decode(eng, rows):
    L = T.LF_MAX_LEN
    lens = tuple((0, 5, L - 1, L)[r % 4] if r < rows - 1 else L for r in range(rows))     # the last row is at capacity: a broken guard writes into the canary row
    assert {0, L - 1, L} <= set(lens)
    for pro in (LF_PRO_LN, LF_PRO_NONE):
        c = LinearCase("rope", pro, LF_ROPE_KV, rows, 3072, 2048, (("kernel", "GEMM16K"), ("nch", 2), ("ln_pro", int(pro == LF_PRO_LN)), ("ln_launch", 0)), lengths=lens)
        dev = to_dev(linear_case_tensors(c))
        kv0 = torch.from_numpy(synth.normal(T.LF_SEED, f"lf.kv.{rows}.{L}.128", (rows + 1, L, 2, 512))).to(bf)       # (+ 1: the canary row of the cache)
        lengths = torch.tensor(lens, dtype=torch.int32, device=DEV)
        res = {}
        for mode in (GROUPED, WIDE):
            kv = kv0.to(DEV)
            o, p = run_op(eng, c, mode, dev, kv=kv, lengths=lengths)
            res[mode] = (o, p, kv.cpu())
        check_plans(c, res[GROUPED][1], res[WIDE][1])
        same_bits(res[GROUPED][0], res[WIDE][0], c.label)
        kg, kw = res[GROUPED][2], res[WIDE][2]
        assert torch.equal(bits(kg), bits(kw)), f"{c.label}: the caches differ"
        assert torch.equal(bits(kw[rows]), bits(kv0[rows])), f"{c.label}: the canary row of the cache was written"
        changed = (bits(kw[:rows]) != bits(kv0[:rows])).flatten(2).any(-1)                # [rows, L]
        want = torch.zeros(rows, L, dtype=torch.bool)
        for r, p_ in enumerate(lens):
            if p_ < L:
                want[r, p_] = True
        assert torch.equal(changed, want), f"{c.label}: positions other than the appended ones changed, or an append is missing"
    # the other row-pair epilogues through row groups: fp32 (the heads: LayerNorm as a launch at K = 4096, as the prologue at K = 2048; an odd N), residual, store
    for pro, epi, N, K, ex in ((LF_PRO_LN, LF_F32, 72, 4096, (("ln_launch", 1), ("ln_pro", 0))), (LF_PRO_LN, LF_F32, 1025, 2048, (("ln_launch", 0), ("ln_pro", 1))),
                               (LF_PRO_NONE, LF_F32, 72, 2048, ()), (LF_PRO_NONE, LF_RESID, 72, 4096, ()), (LF_PRO_LN, LF_STORE, 16, 2048, (("ln_pro", 1),))):
        c = LinearCase("gemm16k", pro, epi, rows, N, K, (("kernel", "GEMM16K"), ("nch", K // 1024)) + ex)
        dev = to_dev(linear_case_tensors(c))
        og, pg = run_op(eng, c, GROUPED, dev)
        ow, pw = run_op(eng, c, WIDE, dev)
        check_plans(c, pg, pw)
        same_bits(og, ow, c.label)


def test_what_has_no_wide_form_stays_per_16(eng):
    """Store and fp32 on the LDS-staged kernel, and the direct-fragment kernel: groups of 16 under ZN_TUNE_WIDE_ROWS = 2, and the same bits."""
    for c in (LinearCase("gemm16s", LF_PRO_NONE, LF_STORE, 33, 7168, 1024, (("kernel", "GEMM16S"),)), LinearCase("gemm16s", LF_PRO_NONE, LF_F32, 33, 2048, 8192, (("kernel", "GEMM16S"),)),
              LinearCase("gemm16", LF_PRO_NONE, LF_RESID, 33, 100, 384, (("kernel", "GEMM16"),))):
        dev = to_dev(linear_case_tensors(c))
        og, pg = run_op(eng, c, GROUPED, dev)
        ow, pw = run_op(eng, c, WIDE, dev)
        check_plans(c, pg, pw, wide_form=False)
        same_bits(og, ow, c.label)


# ---------------------------------------------------------------------------------------------- 5. end to end
@pytest.fixture(scope="module")
def models():
    plain, _ = build_model(E2E_CFG, 53, DEV)
    q8, _ = build_model(E2E_CFG, 53, DEV)
    for blk in q8.backbone.layers:
        for lin in (blk.mlp.fc1, blk.mlp.fc2):
            lin.weight.data.mul_(torch.exp2(T.fp8_row_shifts(lin.weight.shape[0]).float()).to(bf).to(DEV)[:, None])
    q8.quantize_mlp_fp8()
    return {"bf16": plain, "fp8": q8}


def fresh_engine(model, kind):
    """A new handle (ZN_TUNE_WIDE_ROWS unset: zn_debug_tune cannot unset a key) of 32 rows, which every case below then runs on."""
    with model._spare_guard:
        model._engine = model._spare = None
    eng = model.engine(16)
    eng.call("zn_debug_eos_bias", float("-inf"))
    assert eng.mlp_fp8_plan(18) == ([1, 1] if kind == "fp8" else [0, 0])
    return eng


def run_generate(model, seed):
    d = E2E_CFG["d_model"]
    cond = torch.cat([synth.conditioning(700 + i, "wide.e2e", 2, 6, d) for i in range(9)], 0)
    cond = torch.cat([cond[0::2], cond[1::2]], 0).to(DEV)                           # [cond rows | uncond rows]
    tr = {"logits": []}
    sp = dict(temperature=0.0) if seed is None else dict(temperature=1.0, min_p=0.1)
    out = model.generate(cond, max_new_tokens=12, cfg_scale=2.0, batch_size=9, sampling_params=sp, seed=seed, _trace=tr)
    torch.cuda.synchronize()
    return [out.cpu()], [l.cpu() for l in tr["logits"]]


def run_batch(model):
    d = E2E_CFG["d_model"]
    reqs = [GenRequest(synth.conditioning(800 + i, "wide.batch", 2, 3 + i % 4, d).to(DEV), sampling_params=dict(temperature=0.0, repetition_penalty=1.0 + 0.5 * (i % 3)) if i % 2 else
                       dict(temperature=0.9, min_p=0.05 * (1 + i % 3)), seed=None if i % 2 else 40 + i, cfg_scale=[2.0, 1.5, 3.0][i % 3], max_new_tokens=12 - i % 3) for i in range(16)]
    tr = {"logits": []}
    outs = model.generate_batch(reqs, _trace=tr)
    torch.cuda.synchronize()
    assert tr["logits"][0].shape[0] == 16
    return [o.cpu() for o in outs], [l.cpu() for l in tr["logits"]]


def run_serve(model):
    d = E2E_CFG["d_model"]
    reqs = []
    for i in range(20):
        guided = i % 3 != 2
        reqs.append(GenRequest(synth.conditioning(900 + i, "wide.serve", 2 if guided else 1, 4 + i % 3, d).to(DEV), sampling_params=dict(temperature=0.0) if i % 2 else
                               dict(temperature=0.8, min_p=0.1), seed=None if i % 2 else 60 + i, cfg_scale=[2.0, 1.5][i % 2] if guided else 1.0, max_new_tokens=8 + i % 5))
    tr = {}
    out = {r.index: r for r in model.serve(iter(reqs), slots=24, max_prompt=8, max_new_tokens=12, guided=None, sched_every=4, _trace=tr)}
    torch.cuda.synchronize()
    assert sorted(out) == list(range(20)) and all(r.error is None for r in out.values())
    assert tr["logits"][-1].shape[0] == 24
    return [out[i].codes.cpu() for i in range(20)], [l.cpu() for l in tr["logits"]]


CASES = {"generate.greedy": lambda m: run_generate(m, None), "generate.seeded": lambda m: run_generate(m, 1234), "generate_batch": run_batch, "serve": run_serve}
CASE_ROWS = {"generate.greedy": 18, "generate.seeded": 18, "generate_batch": 32, "serve": 24}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_generation_by_default_equals_groups_of_16(models, kind, case):
    model = models[kind]
    eng = fresh_engine(model, kind)
    try:
        rows = CASE_ROWS[case]
        assert list(eng.decode_rows_plan(rows).values()) == [64] * 5
        wide = CASES[case](model)
        assert model.engine(16) is eng
        eng.call("zn_debug_tune", _lib.ZN_TUNE_WIDE_ROWS, GROUPED)
        assert list(eng.decode_rows_plan(rows).values()) == [16] * 5
        grouped = CASES[case](model)
        assert model.engine(16) is eng
    finally:
        eng.call("zn_debug_eos_bias", 0.0)
    assert len(wide[0]) == len(grouped[0])
    for i, (a, b) in enumerate(zip(wide[0], grouped[0])):
        assert a.shape == b.shape and torch.equal(a, b), f"{kind} {case}: codes of result {i} differ"
    assert len(wide[1]) == len(grouped[1]) >= 10
    for i, (a, b) in enumerate(zip(wide[1], grouped[1])):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{kind} {case}: logits of step {i} differ"


def test_hybrid_stack_by_default_equals_groups_of_16():
    """The attention block of a hybrid stack at the real widths (in_proj, out_proj on gemm16k_kernel's row groups, fc1 without a prologue on the
    wide kernel) between Mamba2 layers, whose projections stay per 16: generate(batch_size=9), 18 rows."""
    cfg = dict(synth.HYBRID_FULL_CFG, n_layer=2, attn_layer_idx=[1])
    model, _ = build_model(cfg, 11, DEV)
    eng = model.engine(16)
    eng.call("zn_debug_eos_bias", float("-inf"))
    cond = torch.cat([synth.conditioning(700 + i, "wide.hybrid", 2, 6, cfg["d_model"]) for i in range(9)], 0)
    cond = torch.cat([cond[0::2], cond[1::2]], 0).to(DEV)

    def run():
        tr = {"logits": []}
        out = model.generate(cond, max_new_tokens=12, cfg_scale=2.0, batch_size=9, sampling_params=dict(temperature=0.0), _trace=tr)
        torch.cuda.synchronize()
        assert model.engine(16) is eng
        return out.cpu(), [l.cpu() for l in tr["logits"]]
    try:
        assert eng.decode_rows_plan(18)["fc1"] == 64
        wide = run()
        eng.call("zn_debug_tune", _lib.ZN_TUNE_WIDE_ROWS, GROUPED)
        assert eng.decode_rows_plan(18)["fc1"] == 16
        grouped = run()
    finally:
        eng.call("zn_debug_eos_bias", 0.0)
    assert torch.equal(wide[0], grouped[0]), "hybrid: codes differ"
    assert len(wide[1]) == len(grouped[1]) >= 10
    for i, (a, b) in enumerate(zip(wide[1], grouped[1])):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"hybrid: logits of step {i} differ"


# ---------------------------------------------------------------------------------------------- 6. the step really is wide
def test_decode_rows_plan(models):
    assert hasattr(_lib.load(), "zn_decode_rows_plan") and _lib.ZN_TUNE_WIDE_ROWS == 21
    for kind in ("bf16", "fp8"):
        eng = fresh_engine(models[kind], kind)
        names = ["in_proj", "out_proj", "fc1", "fc2", "heads"]
        assert list(eng.decode_rows_plan(18)) == names
        for rows in (18, 32):
            assert list(eng.decode_rows_plan(rows).values()) == [64] * 5, (kind, rows)
        assert list(eng.decode_rows_plan(16).values()) == [16] * 5 and list(eng.decode_rows_plan(5).values()) == [16] * 5 and list(eng.decode_rows_plan(2).values()) == [4] * 5
        eng.call("zn_debug_tune", _lib.ZN_TUNE_WIDE_ROWS, GROUPED)
        for rows in (16, 18, 32):
            assert list(eng.decode_rows_plan(rows).values()) == [16] * 5, (kind, rows)
        eng.call("zn_debug_tune", _lib.ZN_TUNE_WIDE_ROWS, WIDE)
        assert list(eng.decode_rows_plan(32).values()) == [64] * 5 and list(eng.decode_rows_plan(16).values()) == [16] * 5
    # 64 rows: a handle of its own (the plan does not depend on the handle's row capacity, the statistics buffer does)
    big = HipEngine(models["bf16"].backbone, max_rows=64)
    assert list(big.decode_rows_plan(64).values()) == [64] * 5 and list(big.decode_rows_plan(18).values()) == [64] * 5
    big.call("zn_debug_tune", _lib.ZN_TUNE_WIDE_ROWS, GROUPED)
    assert list(big.decode_rows_plan(64).values()) == [16] * 5
