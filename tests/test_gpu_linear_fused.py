"""Every fused linear prologue and epilogue as a single op, per kernel family and variant: zn_op_linear_fused runs plan_linear and the
production launcher on caller-chosen shapes, the test asserts the plan it reports (which kernel, which variant) and then holds every output
element to the float64 interval of zonos_amd.testing.linear_fused_reference - no tolerance constant, no exempted element
(tests/test_linear_compare_cpu.py shows on the CPU that the reference's own fp32 form stays inside it on every case here, and that seven
subtly wrong kernels do not).  Output buffers sit between canary rows, are NaN-filled before the call, K/V caches have a canary row behind them
and every cache position other than the appended one must come back unchanged."""
import ctypes as C

import pytest
import torch

from zonos_amd import _lib, synth
from zonos_amd import testing as T
from zonos_amd.backbone import HipEngine
from zonos_amd.testing import (LF_F32, LF_PRO_LN, LF_PRO_NONE, LF_RESID, LF_ROPE_KV, LF_SILU, LF_STORE, LinearCase, build_model, linear_case_positions,
                               linear_case_reference, linear_case_tensors, linear_fused_compare)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD, CANARY = 2, 768.0                 # canary rows in front of and behind every output; their value (exact in bf16)
TUNE_DEFAULT = {"ZN_TUNE_SMALL_M_LDS": 2, "ZN_TUNE_FC1_LN_LAUNCH": 1}
bf = torch.bfloat16


def _engine(heads, heads_kv, max_rows=64):
    model, _ = build_model(dict(d_model=2048, n_layer=1, num_heads=heads, num_heads_kv=heads_kv, d_ff=256), 31, DEV)
    eng = HipEngine(model.backbone, max_rows=max_rows)
    eng._model = model
    return eng


@pytest.fixture(scope="module")
def engines():
    return {128: _engine(16, 4), 64: _engine(32, 8)}


class Guarded:
    """[PAD canary rows | rows x cols of NaN | PAD canary rows]"""

    def __init__(self, rows, cols, dtype=bf):
        self.buf = torch.full((rows + 2 * PAD, cols), CANARY, dtype=dtype, device=DEV)
        self.view = self.buf[PAD:PAD + rows]
        self.view.fill_(float("nan"))

    def refill(self):
        self.view.fill_(float("nan"))

    def ptr(self):
        return self.view.data_ptr()

    def check(self, label, written=True):
        b = self.buf.float().cpu()
        assert bool((b[:PAD] == CANARY).all()) and bool((b[-PAD:] == CANARY).all()), f"{label}: a canary row was overwritten"
        inner = b[PAD:-PAD]
        if written:
            assert bool(torch.isfinite(inner).all()), f"{label}: {int((~torch.isfinite(inner)).sum())} elements never written (or not finite)"
        else:
            assert bool(torch.isnan(inner).all()), f"{label}: a buffer the plan does not use was written"
        return self.view.cpu()


def run_case(eng, c: LinearCase, x=None, ref=None, want_stats=False, stats_in=False):
    """One case: returns (output rows on the CPU, reference).  x: activations to use (fc1 behind a real out_proj); ref: an interval computed before."""
    lib, st = eng.lib, _lib.stream_ptr()
    t = linear_case_tensors(c, x=x)
    dev = {k: v.to(DEV).contiguous() for k, v in t.items()}
    nq, nk = 2048, 512
    op = _lib.zn_linear_op(pro=c.pro, epi=c.epi, rows=c.rows, N=c.N, K=c.K, prefill=c.prefill, target_blocks=4, want_ln_stats_out=int(want_stats),
                           ln_stats_in=int(stats_in))
    for k in ("x", "W", "ln_w", "ln_b", "gv", "bias", "resid"):
        if k in dev:
            setattr(op, k, dev[k].data_ptr())
    outs = {}
    if c.epi in (LF_STORE, LF_RESID, LF_SILU) or (c.epi == LF_ROPE_KV and c.prefill):
        outs["out"] = Guarded(c.rows, c.N // 2 if c.epi == LF_SILU else c.N)
        op.out = outs["out"].ptr()
    if c.epi == LF_F32:
        outs["out_f32"] = Guarded(c.rows, c.N, torch.float32)
        op.out_f32 = outs["out_f32"].ptr()
    kv = kv0 = lengths = None
    if c.epi == LF_ROPE_KV:
        cr, pos = linear_case_positions(c)
        n_cache = int(cr.max()) + 1
        max_len = c.pf_base + c.pf_S + 3 if c.prefill else T.LF_MAX_LEN
        kv0 = torch.from_numpy(synth.normal(T.LF_SEED, f"lf.kv.{n_cache}.{max_len}.{c.hd}", (n_cache + 1, max_len, 2, nk))).to(bf)   # (+ 1: a canary row of the cache)
        kv = kv0.to(DEV)
        outs["q_out"] = Guarded(c.rows, nq)
        op.kv, op.q_out, op.max_len, op.pf_S, op.pf_base = kv.data_ptr(), outs["q_out"].ptr(), max_len, c.pf_S, c.pf_base
        if not c.prefill:
            lengths = torch.tensor(c.lengths, dtype=torch.int32, device=DEV)
            op.lengths = lengths.data_ptr()
    try:
        for key, val in c.tune:
            eng.call("zn_debug_tune", getattr(_lib, key), val)
        for _ in range(2 if c.twice else 1):             # split-K twice in a row: the arrival tickets must be back at zero
            for g in outs.values():
                g.refill()
            eng.call("zn_op_linear_fused", C.byref(op), st)
            torch.cuda.synchronize()
    finally:
        for key, _ in c.tune:
            eng.call("zn_debug_tune", getattr(_lib, key), TUNE_DEFAULT[key])
    plan = op.plan_dict()
    assert plan["err"] == 0, (c.label, plan)
    for k, v in c.expect:
        assert plan[k] == v, f"{c.label}: plan {k} = {plan[k]}, the case is about {v} ({plan})"
    if ref is None:
        ref = linear_case_reference(c, t, eng.zc.norm_eps, eng.rope.cpu() if c.epi == LF_ROPE_KV else None, eng.zc.rope_positions)
    desc = f"{c.label} [{plan['kernel']} ks{plan['ks']} nch{plan['nch']} full{plan['full']} nw{plan['nw']} tile8={plan['tile8']} nwv{plan['nwv']} groups{plan['groups']} " \
           f"ksplit{plan['ksplit']} lnp{plan['lnp']} ln_pro{plan['ln_pro']} ln_launch{plan['ln_launch']} stats w{plan['writes_ln_stats']} r{plan['reads_ln_stats']}]"
    period = {"GEMV": 2 * max(1, plan["upw"]), "GEMM16S": 16 * max(1, plan["nwv"]), "GEMM64S": 64, "GEMM_TILED": 128}.get(plan["kernel"], 0)
    if c.epi != LF_ROPE_KV:
        got = outs["out_f32" if c.epi == LF_F32 else "out"].check(c.label)
        res = linear_fused_compare(got, ref, desc, period)
        assert res.ok, (c.label, res)
        return got, ref
    # split + RoPE + KV append: q compact, k / v at (cache row, position) - nothing when the position is the capacity
    if c.prefill:
        assert plan["rope_done"] == 1
        outs["out"].check(c.label, written=False)
    q = outs["q_out"].check(c.label)
    res = linear_fused_compare(q, ref, desc + " q", columns=slice(0, nq))
    assert res.ok, (c.label, res)
    kv1 = kv.cpu()
    fits = pos < max_len
    assert int(fits.sum()) >= (1 if c.rows > 1 or c.prefill else 0)
    expect_same = torch.ones(kv0.shape[:2], dtype=torch.bool)
    expect_same[cr[fits], pos[fits]] = False
    assert torch.equal(kv1.view(torch.int16)[expect_same], kv0.view(torch.int16)[expect_same]), f"{c.label}: a cache position other than the appended one changed"
    if bool(fits.any()):
        app = kv1[cr[fits], pos[fits]].reshape(int(fits.sum()), 2 * nk)          # [k | v] of every appended row
        assert bool(torch.isfinite(app.float()).all())
        sub = ref._replace(lo=ref.lo[fits], hi=ref.hi[fits], mid=ref.mid[fits])
        res = linear_fused_compare(app, sub, desc + " k|v", columns=slice(nq, nq + 2 * nk))
        assert res.ok, (c.label, res)
    return q, ref


@pytest.mark.parametrize("K", list(T._GEMV_KS_NCH))
def test_gemv_every_form(engines, K):
    """ks 1 at nch 1 / 2 / 4 / 8 and ks 4 at nch 2 / 4 / 8, each mask-free (N = 72; rows 2 and 4) and masked (odd N, a unit tail, K short of
    the chunks, 1 and 3 rows), with every epilogue and prologue the decode step fuses into it."""
    for c in T.linear_cases_gemv(K):
        run_case(engines[128], c)


@pytest.mark.parametrize("hd", [128, 64])
def test_split_rope_kv_append(engines, hd):
    for c in T.linear_cases_rope(hd):
        run_case(engines[hd], c)


def test_gemm16k_tiles_prologues_and_row_groups(engines):
    for c in T.linear_cases_gemm16k():
        run_case(engines[128], c)


@pytest.mark.parametrize("rows", [5, 16])
def test_gemm16s_split_k_and_group_shapes(engines, rows):
    for c in T.linear_cases_gemm16s():
        if c.rows == rows:
            run_case(engines[128], c)


def test_gemm16_direct_fragment_forms(engines):
    for c in T.linear_cases_gemm16():
        run_case(engines[128], c)


def test_prefill_gemm64s_and_tiled(engines):
    for c in T.linear_cases_prefill():
        run_case(engines[128], c)


@pytest.mark.parametrize("rows", T.LF_PAIR_ROWS)
def test_layernorm_statistics_handoff_pair(engines, rows):
    """out_proj + residual leaves per-tile LayerNorm statistics, fc1 normalises from them: fc1's reference takes the out kernel's own bf16
    output as x, so only fc1 is on trial; then the launch form (ZN_TUNE_FC1_LN_LAUNCH = 2) against the same interval."""
    eng = engines[128]
    for k_out, Ns in ((2048, [f[0] for f in T.LF_PAIR_FC1]), (4096, [2560])):
        for N in Ns:
            out, fc1 = T.linear_cases_pair(rows, N, k_out)
            x1, _ = run_case(eng, out, want_stats=True)
            _, ref = run_case(eng, fc1, x=x1, stats_in=True)
            print(f"[linear fused {fc1.label}] ambiguous share of a row at most {ref.ambiguous:.4f}")
            out2, fc1b = T.linear_cases_pair(rows, N, k_out, launch=True)
            x1b, _ = run_case(eng, out2, want_stats=True)
            assert torch.equal(x1b.view(torch.int16), x1.view(torch.int16)), "the projection's output must not depend on whether it leaves statistics"
            run_case(eng, fc1b, x=x1, ref=ref)


def test_workspace_overruns_and_unserved_pairs_are_refused():
    """A LayerNorm launch over rows x K beyond the handle's buffer (the latent overrun of zn_op_linear with ln_w at rows > 4 on a small handle),
    statistics for more rows than the handle has, a K the tiled GEMM would read past, and (prologue, epilogue) pairs production never
    instantiates: a status and a message, plan[] filled, nothing launched."""
    model, _ = build_model(synth.TINY_CFG, 77, DEV)
    eng = HipEngine(model.backbone, max_rows=2)
    st = _lib.stream_ptr()
    rows, N, K = 5, 96, 256                                   # 5 x 256 > 2 x 128
    x = torch.zeros(rows, K, dtype=bf, device=DEV)
    W = torch.zeros(N, K, dtype=bf, device=DEV)
    ln = torch.ones(K, dtype=bf, device=DEV)
    out = Guarded(rows, N)

    def call(**kw):
        op = _lib.zn_linear_op(rows=rows, N=N, K=K, target_blocks=4, x=x.data_ptr(), W=W.data_ptr(), ln_w=ln.data_ptr(), ln_b=ln.data_ptr(),
                               out=out.ptr(), resid=x.data_ptr())
        for k, v in kw.items():
            setattr(op, k, v)
        with torch.cuda.device(eng.device):
            rc = eng.lib.zn_op_linear_fused(eng.h, C.byref(op), st)
        return rc, op.plan_dict(), eng.lib.zn_last_error(eng.h).decode()
    rc, plan, msg = call(pro=LF_PRO_LN, epi=LF_STORE)
    assert rc == -1 and plan["err"] == -1 and plan["ln_launch"] == 1 and "LayerNorm launch" in msg, (rc, plan, msg)
    with torch.cuda.device(eng.device):
        rc = eng.lib.zn_op_linear(eng.h, x.data_ptr(), ln.data_ptr(), ln.data_ptr(), W.data_ptr(), out.ptr(), rows, N, K, st)
    assert rc == -1 and "LayerNorm launch" in eng.lib.zn_last_error(eng.h).decode()
    rc, plan, msg = call(pro=LF_PRO_NONE, epi=LF_RESID, N=2048, K=2048, want_ln_stats_out=1)        # (refused before any operand is read)
    assert rc == -1 and plan["writes_ln_stats"] == 1 and "statistics" in msg, (rc, plan, msg)
    rc, plan, msg = call(pro=LF_PRO_NONE, epi=LF_STORE, prefill=1, rows=65, N=200, K=136)
    assert rc == -4 and plan["err"] == -4 and "multiple of 32" in msg, (rc, plan, msg)
    for pro, epi in ((2, LF_RESID), (2, LF_SILU), (0, 5), (1, 5)):
        rc, plan, msg = call(pro=pro, epi=epi, rows=2)
        assert rc == -4 and plan["err"] == -4, (pro, epi, rc, msg)
    rc, plan, msg = call(pro=LF_PRO_LN, epi=LF_STORE, prefill=1, rows=17)
    assert rc == -4 and "not served" in msg, (rc, msg)
    torch.cuda.synchronize()
    out.check("refused calls", written=False)
    rc, plan, msg = call(pro=LF_PRO_NONE, epi=LF_STORE)       # and the handle still serves what fits
    assert rc == 0 and plan["kernel"] == "GEMM16S" and plan["err"] == 0, (rc, plan, msg)
    torch.cuda.synchronize()
    assert bool((out.check("zeros") == 0).all())
