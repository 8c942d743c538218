"""Weight-only FP8 for fc1 / fc2 on the device (zonos_amd/quant.py is the specification).  The acceptance bar is equality, not
a tolerance: the dequantiser must reproduce the CPU table for every finite code in every byte position, the quantiser the specification's codes
and exponents, and a launch that reads the FP8 stream every output bit of the bf16 launch on the dequantised weights - per op over
linear_cases_gemm16s()'s shapes and the LayerNorm-statistics pair, and end to end through generate() and serve()."""
import ctypes as C

import pytest
import torch

from zonos_amd import _lib, synth
from zonos_amd import quant as Q
from zonos_amd import testing as T
from zonos_amd.backbone import HipEngine
from zonos_amd.model import GenRequest
from zonos_amd.testing import LF_PRO_LN, LF_PRO_NONE, LF_RESID, LF_SILU, LF_STORE, LinearCase, build_model, linear_case_reference, linear_case_tensors, linear_fused_compare

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD, CANARY = 2, 768.0
bf = torch.bfloat16
E2E_CFG = dict(d_model=2048, n_layer=2, num_heads=16, num_heads_kv=4, d_ff=8192)


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture(scope="module")
def eng():
    model, _ = build_model(dict(d_model=2048, n_layer=1, num_heads=16, num_heads_kv=4, d_ff=256), 31, DEV)
    e = HipEngine(model.backbone, max_rows=64)
    e._model = model
    return e


def dev_quantize(eng, W):
    """(q, exp, Wdq) of a device matrix through the two device ops."""
    N, K = W.shape
    q = torch.empty((N, K), dtype=torch.uint8, device=DEV)
    e = torch.empty((N,), dtype=torch.int8, device=DEV)
    Wdq = torch.empty_like(W)
    eng.call("zn_op_fp8_quantize_rows", W.data_ptr(), N, K, q.data_ptr(), e.data_ptr(), _lib.stream_ptr())
    eng.call("zn_op_fp8_dequant_rows", q.data_ptr(), e.data_ptr(), N, K, Wdq.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    return q, e, Wdq


# ---------------------------------------------------------------------------------------------- 1. the dequantiser, exhaustively
def test_dequant_every_finite_code_in_every_byte_position(eng):
    tab = Q.e4m3_value_table()
    finite = torch.tensor([c for c in range(256) if not bool(torch.isnan(tab[c]))], dtype=torch.uint8)
    assert finite.numel() == 254
    exps = [-100, -17, -1, 0, 1, 17, 100]
    # row r, column j carries finite[(r + j) % 254]: within 254 rows each code meets each of the 4 byte positions of a word (and each of the 16
    # of a piece); one such block per exponent
    j = torch.arange(256)
    block = finite[(torch.arange(254)[:, None] + j[None, :]) % 254]
    q = block.repeat(len(exps), 1).contiguous()
    e = torch.tensor(exps, dtype=torch.int8).repeat_interleave(254)
    for pos in range(4):
        assert set(q[:254, pos::4].flatten().tolist()) == set(finite.tolist())
    want = Q.dequantize_rows_fp8(q, e)
    assert torch.equal(want.double(), tab[q.long()] * torch.exp2(e.double())[:, None])
    out = torch.full(q.shape, float("nan"), dtype=bf, device=DEV)
    qd, ed = q.to(DEV), e.to(DEV)
    eng.call("zn_op_fp8_dequant_rows", qd.data_ptr(), ed.data_ptr(), q.shape[0], q.shape[1], out.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    got = out.cpu()
    bad = bits(got) != bits(want)
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} differ; first: row {int(bad.nonzero()[0][0])} col {int(bad.nonzero()[0][1])}"


# ---------------------------------------------------------------------------------------------- 2. the quantiser
@pytest.mark.parametrize("which", ["96x256", "64x8192", "adversarial"])
def test_quantiser_matches_the_specification(eng, which):
    W = T.fp8_adversarial_rows()[0] if which == "adversarial" else T.fp8_seeded_matrix(*T.FP8_MATRIX_SHAPES[0 if which == "96x256" else 1])
    q_ref, e_ref, w_ref = Q.quantize_rows_fp8(W)
    q, e, Wdq = dev_quantize(eng, W.to(DEV))
    assert torch.equal(e.cpu(), e_ref), f"exponents differ in rows {(e.cpu() != e_ref).nonzero().flatten().tolist()[:8]}"
    bad = q.cpu() != q_ref
    assert not bool(bad.any()), f"{int(bad.sum())} codes differ; first at {bad.nonzero()[0].tolist()}"
    assert torch.equal(bits(Wdq.cpu()), bits(w_ref))


# ---------------------------------------------------------------------------------------------- 3. the kernel, bit for bit
class Guarded:
    def __init__(self, rows, cols):
        self.buf = torch.full((rows + 2 * PAD, cols), CANARY, dtype=bf, device=DEV)
        self.view = self.buf[PAD:PAD + rows]
        self.view.fill_(float("nan"))

    def check(self, label):
        b = self.buf.float().cpu()
        assert bool((b[:PAD] == CANARY).all()) and bool((b[-PAD:] == CANARY).all()), f"{label}: a canary row was overwritten"
        assert bool(torch.isfinite(b[PAD:-PAD]).all()), f"{label}: elements never written (or not finite)"
        return self.view.cpu()


_QCACHE: dict = {}


def check_exponents_differ(e, c):
    """The per-row scale lookup is on trial only if the rows' exponents differ where a wrong index would land: inside every 16-row tile of the
    first workgroup, between value row u and gate row N / 2 + u, and between the last row (the one a clamped edge group repeats) and its
    neighbour."""
    N, F = c.N, c.N // 2
    assert len(set(e.tolist())) >= 4, (c.label, sorted(set(e.tolist())))
    for t0 in range(0, min(N, 64), 16):
        assert len(set(e[t0:t0 + 16].tolist())) > 1, (c.label, t0)
    assert int(e[0]) != int(e[1]) and int(e[N - 1]) != int(e[N - 2]), c.label
    if c.epi == LF_SILU:
        assert bool((e[:16] != e[F:F + 16]).all()) and float((e[:F] != e[F:]).float().mean()) > 0.5, c.label


def run_both(eng, c: LinearCase, x=None, want_stats=False, stats_in=False, fp8=True, interval=False):
    """The case through zn_op_linear_fused on the dequantised weights and (fp8) through zn_op_linear_fp8 on the stream: outputs and plans."""
    t = linear_case_tensors(c, x=x)
    dev = {k: v.to(DEV).contiguous() for k, v in t.items()}
    if (c.N, c.K) not in _QCACHE:
        _QCACHE.clear()                                            # one matrix at a time: the largest is 67 MB as bf16
        # the synthetic rows all have one amax binade: scale them by row-dependent powers of two (exact in bf16), or the launch would meet one
        # exponent in all rows and could read any row's scale
        # (the projection in front of fc1, which only ever runs as bf16 here, keeps its rows)
        W = dev["W"] * torch.exp2(T.fp8_row_shifts(c.N).float()).to(bf).to(DEV)[:, None] if fp8 else dev["W"]
        _QCACHE[(c.N, c.K)] = dev_quantize(eng, W)
    q, e, Wdq = _QCACHE[(c.N, c.K)]
    if fp8:
        check_exponents_differ(e.cpu(), c)
    res = []
    try:
        for key, val in c.tune:
            eng.call("zn_debug_tune", getattr(_lib, key), val)
        for use8 in ((False, True) if fp8 else (False,)):
            op = _lib.zn_linear_op(pro=c.pro, epi=c.epi, rows=c.rows, N=c.N, K=c.K, target_blocks=4, want_ln_stats_out=int(want_stats), ln_stats_in=int(stats_in))
            for k in ("x", "ln_w", "ln_b", "resid"):
                if k in dev:
                    setattr(op, k, dev[k].data_ptr())
            op.W = Wdq.data_ptr()
            g = Guarded(c.rows, c.N // 2 if c.epi == LF_SILU else c.N)
            op.out = g.view.data_ptr()
            for _ in range(2 if c.twice else 1):                   # split-K twice in a row: the arrival tickets must be back at zero
                g.view.fill_(float("nan"))
                if use8:
                    eng.call("zn_op_linear_fp8", C.byref(op), q.data_ptr(), e.data_ptr(), _lib.stream_ptr())
                else:
                    eng.call("zn_op_linear_fused", C.byref(op), _lib.stream_ptr())
                torch.cuda.synchronize()
            res.append((g.check(c.label + (" fp8" if use8 else " bf16")), op.plan_dict()))
    finally:
        for key, _ in c.tune:
            eng.call("zn_debug_tune", getattr(_lib, key), 1)
    (out_a, plan_a) = res[0]
    for k, v in c.expect:
        assert plan_a[k] == v, f"{c.label}: plan {k} = {plan_a[k]}, the case is about {v}"
    assert plan_a["w8"] == 0 and plan_a["err"] == 0
    if fp8:
        out_b, plan_b = res[1]
        assert plan_b["w8"] == 1, (c.label, plan_b)
        assert {k: v for k, v in plan_b.items() if k != "w8"} == {k: v for k, v in plan_a.items() if k != "w8"}, (c.label, plan_a, plan_b)
        bad = bits(out_a) != bits(out_b)
        assert not bool(bad.any()), f"{c.label}: {int(bad.sum())} of {bad.numel()} output elements differ between the FP8 and the bf16 launch; first at {bad.nonzero()[0].tolist()}"
        if interval:
            ref = linear_case_reference(c, dict(t, W=Wdq.cpu()), eng.zc.norm_eps, None, eng.zc.rope_positions)
            assert linear_fused_compare(out_b, ref, c.label + " fp8 vs float64 interval").ok
    return out_a


@pytest.mark.parametrize("rows", [5, 16, 24])
def test_fp8_launch_equals_bf16_launch_on_gemm16s_shapes(eng, rows):
    """One slice, split-K 2 / 8 / 16, 32- and 64-row workgroups, the clamped edge group 513; none x residual and none x SiLU gate."""
    n = 0
    for c in T.linear_cases_gemm16s():
        if c.rows != 5 or c.pro != LF_PRO_NONE or c.epi not in (LF_RESID, LF_SILU):
            continue
        run_both(eng, c._replace(rows=rows), interval=(rows == 16 and c.N == 2048 and c.epi == LF_RESID))      # fc2's shape also against the float64 interval
        n += 1
    assert n == 12


@pytest.mark.parametrize("rows", [5, 16, 24])
def test_fp8_fc1_behind_handed_over_statistics(eng, rows):
    """out_proj leaves LayerNorm statistics, fc1 normalises from them (LNP) - and under ZN_TUNE_FC1_LN_LAUNCH = 2 from a LayerNorm launch."""
    for N in (2560, 16384, 32736):
        out, fc1 = T.linear_cases_pair(rows, N)
        x1 = run_both(eng, out, want_stats=True, fp8=False)
        run_both(eng, fc1, x=x1, stats_in=True)
        out2, fc1b = T.linear_cases_pair(rows, N, launch=True)
        x1b = run_both(eng, out2, want_stats=True, fp8=False)
        assert torch.equal(bits(x1b), bits(x1))
        run_both(eng, fc1b, x=x1)


# ---------------------------------------------------------------------------------------------- 4. refusals, before any launch
def test_refusals_launch_nothing(eng):
    rows, N, K = 5, 96, 256
    x = torch.zeros(rows, K, dtype=bf, device=DEV)
    W = torch.zeros(N, 264, dtype=bf, device=DEV)
    q = torch.zeros(N, 264, dtype=torch.uint8, device=DEV)
    e = torch.zeros(N, dtype=torch.int8, device=DEV)
    ln = torch.ones(264, dtype=bf, device=DEV)
    out = torch.full((64, N), float("nan"), dtype=bf, device=DEV)

    def call(**kw):
        op = _lib.zn_linear_op(rows=rows, N=N, K=K, target_blocks=4, x=x.data_ptr(), W=W.data_ptr(), ln_w=ln.data_ptr(), ln_b=ln.data_ptr(), out=out.data_ptr(), resid=x.data_ptr())
        for k, v in kw.items():
            setattr(op, k, v)
        with torch.cuda.device(eng.device):
            rc = eng.lib.zn_op_linear_fp8(eng.h, C.byref(op), q.data_ptr(), e.data_ptr(), _lib.stream_ptr())
        return rc, op.plan_dict(), eng.lib.zn_last_error(eng.h).decode()
    rc, plan, msg = call(pro=LF_PRO_LN, epi=LF_STORE)
    assert rc == -4 and plan["err"] == -4 and "no FP8 kernel" in msg, (rc, plan, msg)
    rc, plan, msg = call(pro=LF_PRO_NONE, epi=LF_RESID, K=264)
    assert rc == -4 and plan["err"] == -4 and "multiple of 256" in msg, (rc, plan, msg)
    rc, plan, msg = call(pro=LF_PRO_NONE, epi=LF_RESID, prefill=1, rows=17)
    assert rc == -4 and plan["err"] == -4 and "prefill" in msg, (rc, plan, msg)
    rc, plan, msg = call(pro=LF_PRO_NONE, epi=LF_RESID, rows=2)                      # the GEMV reads bf16: the op would not read the stream
    assert rc == -4 and plan["w8"] == 0 and "would not read" in msg, (rc, plan, msg)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.float()).all()), "a refused call wrote its output"
    rc, plan, msg = call(pro=LF_PRO_NONE, epi=LF_RESID)                              # and what is served still runs
    assert rc == 0 and plan["w8"] == 1 and plan["kernel"] == "GEMM16S", (rc, plan, msg)
    torch.cuda.synchronize()
    # zn_set_mlp_fp8: a hybrid handle; a model whose d_model is no multiple of 256
    for cfg, seed, what in ((synth.HYBRID_TINY_CFG, 23, "hybrid"), (synth.TINY_CFG, 77, "multiples of 256")):
        m, _ = build_model(cfg, seed, DEV)
        h = HipEngine(m.backbone, max_rows=2)
        with torch.cuda.device(h.device):
            rc = h.lib.zn_set_mlp_fp8(h.h, 0, q.data_ptr(), e.data_ptr(), q.data_ptr(), e.data_ptr())
        assert rc == -4 and what in h.lib.zn_last_error(h.h).decode(), (rc, h.lib.zn_last_error(h.h).decode())
        out2 = (C.c_int32 * 2)(7, 7)
        assert h.lib.zn_mlp_fp8_plan(h.h, 8, out2) == 0 and list(out2) == [0, 0]
    with pytest.raises(_lib.ZonosHipError, match="hybrid"):
        build_model(synth.HYBRID_TINY_CFG, 23, DEV)[0].quantize_mlp_fp8()


def _e2e_pair():
    """A: quantize_mlp_fp8() applied.  B: a plain bf16 model holding A's dequantised weights."""
    A, _ = build_model(E2E_CFG, 53, DEV)
    # the synthetic rows of a matrix all share one amax binade: scale them by row-dependent powers of two (exact), so that every workgroup, and
    # the value and gate halves of fc1, meet different scale exponents
    for blk in A.backbone.layers:
        for lin in (blk.mlp.fc1, blk.mlp.fc2):
            lin.weight.data.mul_(torch.exp2(T.fp8_row_shifts(lin.weight.shape[0]).float()).to(bf).to(DEV)[:, None])
    before = [bits(b.mlp.fc1.weight.data).clone() for b in A.backbone.layers]
    assert A.mlp_weights == "bf16"
    A.quantize_mlp_fp8()
    assert A.mlp_weights == "fp8"
    for blk in A.backbone.layers:
        for name, epi in (("fc1", LF_SILU), ("fc2", LF_RESID)):
            e = getattr(blk.mlp, name + "_exp").cpu()
            check_exponents_differ(e, LinearCase("e2e." + name, LF_PRO_NONE, epi, 16, e.numel(), 0))
    assert any(not torch.equal(x, bits(b.mlp.fc1.weight.data)) for x, b in zip(before, A.backbone.layers)), "quantisation must change the weights (it is lossy)"
    B, _ = build_model(E2E_CFG, 53, DEV)
    for a, b in zip(A.backbone.layers, B.backbone.layers):
        b.mlp.fc1.weight.data.copy_(a.mlp.fc1.weight.data)
        b.mlp.fc2.weight.data.copy_(a.mlp.fc2.weight.data)
    assert B.mlp_weights == "bf16" and not hasattr(B.backbone.layers[0].mlp, "fc1_q")
    return A, B


@pytest.fixture(scope="module")
def e2e():
    return _e2e_pair()


def test_set_mlp_fp8_state_and_verification(e2e, monkeypatch):
    A, _ = e2e
    mlp = A.backbone.layers[1].mlp
    ptrs = [t.data_ptr() for t in (mlp.fc1_q, mlp.fc1_exp, mlp.fc2_q, mlp.fc2_exp)]
    h = A.engine(4)
    # the specification on the model's own weights: the device codes dequantise to the bf16 parameters (the contract of zn_set_mlp_fp8)
    assert torch.equal(bits(Q.dequantize_rows_fp8(mlp.fc2_q[:64].cpu(), mlp.fc2_exp[:64].cpu())), bits(mlp.fc2.weight.data[:64].cpu()))
    monkeypatch.setenv("ZN_FP8_VERIFY", "1")
    h.call("zn_set_mlp_fp8", 1, *ptrs)                                                # the contract holds: accepted
    flipped = mlp.fc1_q.clone()
    flipped[1234, 77] ^= 0x01
    torch.cuda.synchronize()
    with torch.cuda.device(h.device):
        rc = h.lib.zn_set_mlp_fp8(h.h, 1, flipped.data_ptr(), *ptrs[1:])
    assert rc == -1 and "not the dequantised stream" in h.lib.zn_last_error(h.h).decode()
    monkeypatch.delenv("ZN_FP8_VERIFY")
    assert h.mlp_fp8_plan(8) == [1, 1], "a refused stream must leave the attached one in place"
    with torch.cuda.device(h.device):
        assert h.lib.zn_set_mlp_fp8(h.h, 1, ptrs[0], None, ptrs[2], ptrs[3]) == -1    # some but not all
        assert h.lib.zn_set_mlp_fp8(h.h, 2, *ptrs) == -1                              # layer out of range
    # inside a generation
    d = E2E_CFG["d_model"]
    reqs = [GenRequest(synth.conditioning(900 + i, "fp8.state", 2, 4, d).to(DEV), sampling_params=dict(temperature=0.0), cfg_scale=2.0, max_new_tokens=4) for i in range(2)]
    gen = A.serve(iter(reqs), slots=4, max_prompt=8, max_new_tokens=4, guided=True)
    next(gen)
    with torch.cuda.device(h.device):
        rc = h.lib.zn_set_mlp_fp8(h.h, 1, *ptrs)
    assert rc == -3 and "inside a generation" in h.lib.zn_last_error(h.h).decode()
    gen.close()
    h.call("zn_set_mlp_fp8", 1, *ptrs)
    # detach and attach again
    h.call("zn_set_mlp_fp8", 0, None, None, None, None)
    assert h.mlp_fp8_plan(8) == [0, 0]
    m0 = A.backbone.layers[0].mlp
    h.call("zn_set_mlp_fp8", 0, m0.fc1_q.data_ptr(), m0.fc1_exp.data_ptr(), m0.fc2_q.data_ptr(), m0.fc2_exp.data_ptr())
    assert h.mlp_fp8_plan(8) == [1, 1]


# ---------------------------------------------------------------------------------------------- 5. end to end
def _generate(model, batch, steps=12):
    d = E2E_CFG["d_model"]
    cond = torch.cat([synth.conditioning(700 + i, "fp8.e2e", 2, 6, d) for i in range(batch)], 0)
    cond = torch.cat([cond[0::2], cond[1::2]], 0).to(DEV)                           # [cond rows ‖ uncond rows]
    tr = {"logits": []}
    eng = model.engine(batch)
    eng.call("zn_debug_eos_bias", float("-inf"))
    try:
        out = model.generate(cond, max_new_tokens=steps, cfg_scale=2.0, batch_size=batch, sampling_params=dict(temperature=0.0), _trace=tr)
    finally:
        eng.call("zn_debug_eos_bias", 0.0)
    torch.cuda.synchronize()
    return out.cpu(), [l.cpu() for l in tr["logits"]]


def _same_run(a, b, what):
    assert torch.equal(a[0], b[0]), f"{what}: codes differ"
    assert len(a[1]) == len(b[1]) >= 10
    for i, (x, y) in enumerate(zip(a[1], b[1])):
        assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{what}: logits of step {i} differ"


def test_generate_equals_the_bf16_model_on_the_dequantised_weights(e2e):
    A, B = e2e
    assert A.engine(4).mlp_fp8_plan(8) == [1, 1] and A.engine(4).mlp_fp8_plan(2) == [0, 0] and A.engine(4).mlp_fp8_plan(16) == [1, 1]
    assert B.engine(4).mlp_fp8_plan(8) == [0, 0]
    ref8, ref2 = _generate(B, 4), _generate(B, 1)
    _same_run(_generate(A, 4), ref8, "8 rows (FP8 stream)")
    _same_run(_generate(A, 1), ref2, "2 rows (the whole-step kernel reads the bf16 copy)")
    eng = A.engine(4)
    eng.call("zn_debug_tune", _lib.ZN_TUNE_MLP_FP8, 2)
    try:
        assert eng.mlp_fp8_plan(8) == [0, 0]
        _same_run(_generate(A, 4), ref8, "8 rows, ZN_TUNE_MLP_FP8 = 2")
    finally:
        eng.call("zn_debug_tune", _lib.ZN_TUNE_MLP_FP8, 1)
    assert eng.mlp_fp8_plan(8) == [1, 1]


def test_serve_session_equals_the_bf16_model(e2e):
    A, B = e2e
    d = E2E_CFG["d_model"]

    def session(model):
        reqs = [GenRequest(synth.conditioning(800 + i, "fp8.serve", 2, 4 + i % 3, d).to(DEV), sampling_params=dict(temperature=0.0), cfg_scale=[2.0, 1.5, 3.0][i % 3],
                           max_new_tokens=6 + i % 4) for i in range(10)]
        tr = {}
        out = {r.index: r for r in model.serve(iter(reqs), slots=8, max_prompt=8, max_new_tokens=10, guided=True, sched_every=4, _trace=tr)}
        assert sorted(out) == list(range(10)) and all(r.error is None for r in out.values())
        return out, tr
    assert A.engine(8).mlp_fp8_plan(16) == [1, 1]
    (oa, ta), (ob, tb) = session(A), session(B)
    for i in range(10):
        assert torch.equal(oa[i].codes.cpu(), ob[i].codes.cpu()), f"request {i}: codes differ"
    assert len(ta["logits"]) == len(tb["logits"]) > 0
    for i, (x, y) in enumerate(zip(ta["logits"], tb["logits"])):
        assert torch.equal(x.cpu().view(torch.int32), y.cpu().view(torch.int32)), f"session logits {i} differ"


def test_bf16_mode_leaves_the_parameters_untouched(tmp_path):
    """from_local(mlp_weights="bf16") - the default - loads the checkpoint's bits; "fp8" replaces fc1 / fc2 by their dequantised values and
    nothing else; any other value is refused."""
    import json
    from safetensors.torch import save_file
    from zonos_amd.model import Zonos
    cfg = dict(d_model=256, n_layer=1, num_heads=2, num_heads_kv=1, d_ff=512)
    ck = {k: v.clone() for k, v in synth.zonos_state_dict(cfg, 11).items()}
    ck["prefix_conditioner.norm.weight"] = torch.ones(cfg["d_model"], dtype=bf)
    ck["prefix_conditioner.norm.bias"] = torch.zeros(cfg["d_model"], dtype=bf)
    save_file(ck, str(tmp_path / "model.safetensors"))
    conf = {"backbone": {"d_model": cfg["d_model"], "n_layer": cfg["n_layer"], "attn_mlp_d_intermediate": cfg["d_ff"], "d_intermediate": 0, "ssm_cfg": {},
                         "attn_layer_idx": list(range(cfg["n_layer"])), "attn_cfg": {"num_heads": cfg["num_heads"], "num_heads_kv": cfg["num_heads_kv"], "causal": True},
                         "rms_norm": False, "residual_in_fp32": False, "norm_epsilon": 1e-5},
            "prefix_conditioner": {"conditioners": [], "projection": "none"}, "eos_token_id": 1024, "masked_token_id": 1025, "pad_vocab_to_multiple_of": 8}
    (tmp_path / "config.json").write_text(json.dumps(conf))
    plain = Zonos.from_local(str(tmp_path / "config.json"), str(tmp_path / "model.safetensors"), DEV)
    same = Zonos.from_local(str(tmp_path / "config.json"), str(tmp_path / "model.safetensors"), DEV, mlp_weights="bf16")
    f8 = Zonos.from_local(str(tmp_path / "config.json"), str(tmp_path / "model.safetensors"), DEV, mlp_weights="fp8")
    assert plain.mlp_weights == same.mlp_weights == "bf16" and f8.mlp_weights == "fp8"
    ps, ss, fs = plain.state_dict(), same.state_dict(), f8.state_dict()
    assert set(ps) == set(ss) == set(fs), "the codes and exponents are not part of the state dict"
    for k in ps:
        assert torch.equal(bits(ps[k]), bits(ss[k])), k
        if ".mlp.fc" in k:
            assert torch.equal(bits(fs[k].cpu()), bits(Q.quantize_rows_fp8(ps[k])[2])), k
        else:
            assert torch.equal(bits(ps[k]), bits(fs[k])), k
    with pytest.raises(_lib.ZonosHipError, match="mlp_weights"):
        Zonos.from_local(str(tmp_path / "config.json"), str(tmp_path / "model.safetensors"), DEV, mlp_weights="int8")
