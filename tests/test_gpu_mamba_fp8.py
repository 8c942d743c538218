"""The Mamba2 in_proj and out_proj of a hybrid model read as an FP8 stream (Zonos.quantize_mamba_fp8, zn_set_mamba_fp8, zn_mamba_fp8_kernels.h).
The mode is lossy with respect to the checkpoint and EXACT with respect to its own dequantised weights, so the bar everywhere is equality of the raw bits
(int16 / int32 views, torch.equal) between three engines: (a) the quantised model with the stream attached and read, (b) the same model under
ZN_TUNE_MAMBA_FP8 = 2, (c) a plain bf16 model built from the dequantised weights that was never quantised.
Test weights: weight row n of both projections is multiplied by 2^-(n mod 16) before quantising (exact), so that the 16 rows of every weight tile carry 16
different scale exponents - a kernel that applied another row's scale would not pass.
  1. per op through zn_op_mamba_step on layer 0 of two two-layer models of the production widths (d_state 128 / one group, d_state 64 / two groups): 5 .. 80 rows,
     three consecutive tokens from per-row random states, state and output between canaries, the output pre-filled with NaN; at 33 and 64 rows (a) again under
     ZN_TUNE_WIDE_HYBRID 1, 2 and 3;
  2. zn_set_mamba_fp8: refusals, ZN_FP8_VERIFY, detach;
  3. generate() at 3 and 9 utterances, a 16-request generate_batch(), a mixed serve() session of 24 rows, and generate() at 1 and 2 utterances (the bf16 copy):
     codes and per-step logits of (a) against (c);
  4. a hybrid model of other widths (synth.HYBRID_TINY_CFG): quantize_mamba_fp8() raises ZonosHipError naming the widths and changes nothing - the behaviour chosen
     over carrying a stream that no decode step would read;
  5. mamba_weights="bf16" leaves every parameter's bits untouched; a transformer model refuses."""
import ctypes as C

import pytest
import torch

from zonos_amd import _lib, quant as Q, synth
from zonos_amd.backbone import HipEngine
from zonos_amd.backbone._hip import mamba2_dims
from zonos_amd.model import GenRequest
from zonos_amd.testing import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
bf = torch.bfloat16
PAD, CANARY, SPAD = 2, 768.0, 4096
WIDE_CFG = dict(synth.HYBRID_FULL_CFG, n_layer=2, attn_layer_idx=[1])
GROUPS_CFG = dict(WIDE_CFG, ssm_cfg={"layer": "Mamba2", "d_state": 64, "ngroups": 2})
CFGS = {"wide": WIDE_CFG, "groups": GROUPS_CFG}
ROWS = (5, 16, 17, 33, 64, 65, 80)
HAS_FEATURE = hasattr(_lib, "ZN_TUNE_MAMBA_FP8") and "zn_set_mamba_fp8" in _lib.SIGNATURES


def tune_key():
    assert HAS_FEATURE, "this library has no ZN_TUNE_MAMBA_FP8 / zn_set_mamba_fp8"
    return _lib.ZN_TUNE_MAMBA_FP8


def bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def mamba_mixers(model):
    return [blk.mixer for blk in model.backbone.layers if blk.is_mamba]


def rescale_rows(model):
    """weight row n of in_proj and out_proj *= 2^-(n mod 16): exact (a power of two, far from the denormals), and asserted to be."""
    for mx in mamba_mixers(model):
        for lin in (mx.in_proj, mx.out_proj):
            W = lin.weight.data
            f = torch.exp2(-(torch.arange(W.shape[0], device=W.device) % 16).float())[:, None]
            want = W.float() * f
            W.mul_(f.to(bf))
            assert torch.equal(W.float(), want) and bool(torch.isfinite(W.float()).all()) and bool((W.float().abs().amax(1) > 0).all())


def quantised_pair(cfg, seed):
    """A: rows rescaled, then quantize_mamba_fp8().  Cm: a plain bf16 model holding A's dequantised weights, never quantised."""
    tune_key()
    A, _ = build_model(cfg, seed, DEV)
    rescale_rows(A)
    before = {k: v.clone() for k, v in A.state_dict().items()}
    assert A.mamba_weights == "bf16" and A.mamba_fp8_plan(8) == {"in_proj": False, "out_proj": False}
    A.quantize_mamba_fp8()
    assert A.mamba_weights == "fp8"
    after = A.state_dict()
    assert set(after) == set(before), "the codes and exponents are not part of the state dict"
    changed = sorted(k for k in before if not torch.equal(bits(before[k]), bits(after[k])))
    assert changed == sorted("backbone.layers.%d.mixer.%s.weight" % (i, n) for i, blk in enumerate(A.backbone.layers) if blk.is_mamba for n in ("in_proj", "out_proj")), changed
    for mx in mamba_mixers(A):
        for name in ("in_proj", "out_proj"):
            q, e, W = getattr(mx, name + "_q"), getattr(mx, name + "_exp"), getattr(mx, name).weight.data
            assert q.dtype == torch.uint8 and e.dtype == torch.int8 and q.shape == W.shape and e.shape == (W.shape[0],)
            tiles = e.cpu().view(-1, 16).to(torch.int64)
            assert bool((tiles.sort(1).values.diff(dim=1) != 0).all()), f"{name}: a 16-row tile repeats a scale exponent"
            # the specification on a few tiles: the device's codes, exponents and dequantised values are quant.py's
            rows = slice(W.shape[0] - 48, W.shape[0])
            key = "backbone.layers.0.mixer.%s.weight" % name
            cq, ce, cw = Q.quantize_rows_fp8(before[key][rows].cpu())
            assert torch.equal(cq, q[rows].cpu()) and torch.equal(ce, e[rows].cpu()) and torch.equal(bits(cw), bits(W[rows].cpu())), name
    Cm, _ = build_model(cfg, seed, DEV)
    Cm.load_state_dict(A.state_dict(), strict=True)
    assert Cm.mamba_weights == "bf16" and not hasattr(mamba_mixers(Cm)[0], "in_proj_q")
    return A, Cm


_BUILT = {}


def get_built():
    """The models and per-op handles, built once on first use (inside a test, behind tune_key(): without the feature every test FAILS, none errors or skips)."""
    tune_key()
    out = _BUILT
    for name, cfg in CFGS.items():
        if name in out:
            continue
        A, Cm = quantised_pair(cfg, 11)
        # per-op handles of 80 rows: (a) stream read, (b) the same model ignoring it, (c) the plain model, and one more of (a) whose ZN_TUNE_WIDE_HYBRID the cases set
        a, b, c, forms = (HipEngine(A.backbone, max_rows=80), HipEngine(A.backbone, max_rows=80), HipEngine(Cm.backbone, max_rows=80), HipEngine(A.backbone, max_rows=80))
        b.call("zn_debug_tune", tune_key(), 2)
        out[name] = dict(A=A, C=Cm, m=mamba2_dims(A.config.backbone), a=a, b=b, c=c, forms=forms)
    return out


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _BUILT.clear()


class State:
    """[SPAD canary elements | conv window [rows][conv_dim][4] | SSM state [rows][heads][headdim][d_state] | SPAD canary elements], and the output rows
    [PAD canary rows | rows x d of NaN | PAD canary rows]"""

    def __init__(self, eng, m, rows, d, seed):
        gen = torch.Generator(device=DEV).manual_seed(seed)
        self.n_conv, n_ssm = rows * m["conv_dim"] * m["d_conv"], rows * m["nheads"] * m["headdim"] * m["d_state"]
        assert (self.n_conv + n_ssm) * 2 == eng.lib.zn_mamba_state_bytes_per_layer(C.byref(eng.zc), rows, None)
        self.buf = torch.full((2 * SPAD + self.n_conv + n_ssm,), CANARY, dtype=bf, device=DEV)
        self.state = self.buf[SPAD:-SPAD]
        self.state.copy_(torch.randn(self.state.numel(), generator=gen, device=DEV, dtype=torch.float32).to(bf))      # every row its own window and state
        self.out = torch.full((rows + 2 * PAD, d), CANARY, dtype=bf, device=DEV)
        self.rows = rows

    def step(self, eng, x):
        self.out[PAD:-PAD].fill_(float("nan"))
        eng.call("zn_op_mamba_step", 0, x.data_ptr(), self.state.data_ptr(), self.out[PAD:-PAD].data_ptr(), self.rows, _lib.stream_ptr())
        torch.cuda.synchronize()

    def check(self, label):
        assert bool((self.buf[:SPAD] == CANARY).all()) and bool((self.buf[-SPAD:] == CANARY).all()), f"{label}: the state buffer's canary was overwritten"
        assert bool((self.out[:PAD] == CANARY).all()) and bool((self.out[-PAD:] == CANARY).all()), f"{label}: a canary row of the output was overwritten"
        assert bool(torch.isfinite(self.out[PAD:-PAD].float()).all()), f"{label}: output elements never written (or not finite)"
        assert bool(torch.isfinite(self.state.float()).all()), f"{label}: state not finite"


def three_tokens(eng, m, rows, d, xs, label):
    st = State(eng, m, rows, d, seed=900 + rows)
    snaps = []
    for t, x in enumerate(xs):
        st.step(eng, x)
        st.check(f"{label} token {t}")
        snaps.append((st.out[PAD:-PAD].clone(), st.state.clone()))
    return snaps, st.n_conv


# ---------------------------------------------------------------------------------------------- 1. per op
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("cfg_name", list(CFGS))
def test_mamba_step_bits_equal_across_the_three_engines(cfg_name, rows):
    key = tune_key()
    B = get_built()[cfg_name]
    m, d = B["m"], CFGS[cfg_name]["d_model"]
    gen = torch.Generator(device=DEV).manual_seed(500 + rows)
    xs = [torch.randn((rows, d), generator=gen, device=DEV, dtype=torch.float32).to(bf) for _ in range(3)]
    assert B["a"].mamba_fp8_plan(rows) == [1, 1] and B["b"].mamba_fp8_plan(rows) == [0, 0] and B["c"].mamba_fp8_plan(rows) == [0, 0]
    runs = {}
    for which in ("c", "a", "b"):                    # the plain model first: what the others are compared with
        runs[which], nc = three_tokens(B[which], m, rows, d, xs, f"{cfg_name} rows {rows} engine ({which})")
    if rows in (33, 64):                             # every wide form of the in_proj reads the stream, and agrees
        for form in (1, 2, 3):
            B["forms"].call("zn_debug_tune", _lib.ZN_TUNE_WIDE_HYBRID, form)
            assert B["forms"].mamba_fp8_plan(rows) == [1, 1], form
            plan = B["forms"].hybrid_rows_plan(rows)
            assert plan["mamba_in_proj"] == (16 if form == 1 else 64) and plan["mamba_out_proj"] == 64, (form, plan)
            runs[f"a, ZN_TUNE_WIDE_HYBRID {form}"], _ = three_tokens(B["forms"], m, rows, d, xs, f"{cfg_name} rows {rows} form {form}")
    ref = runs.pop("c")
    for which, snaps in runs.items():
        for t in range(3):
            assert torch.equal(bits(snaps[t][0]), bits(ref[t][0])), f"{cfg_name} rows {rows}: output of engine ({which}) differs from the plain bf16 model at token {t}"
            assert torch.equal(bits(snaps[t][1][:nc]), bits(ref[t][1][:nc])), f"{cfg_name} rows {rows}: conv window of engine ({which}) differs at token {t}"
            assert torch.equal(bits(snaps[t][1][nc:]), bits(ref[t][1][nc:])), f"{cfg_name} rows {rows}: SSM state of engine ({which}) differs at token {t}"
    # the tokens moved the state, and the rows differ
    assert not torch.equal(ref[0][1], ref[2][1]) and not torch.equal(ref[2][0][0], ref[2][0][rows - 1])
    assert key == 23


# ---------------------------------------------------------------------------------------------- 2. zn_set_mamba_fp8
def test_set_mamba_fp8_state_and_refusals(monkeypatch):
    tune_key()
    A = get_built()["wide"]["A"]
    mx = A.backbone.layers[0].mixer
    ts = (mx.in_proj_q, mx.in_proj_exp, mx.out_proj_q, mx.out_proj_exp)
    ptrs = [t.data_ptr() for t in ts]
    h = A.engine(4)
    assert h.mamba_fp8_plan(8) == [1, 1] and h.mamba_fp8_plan(4) == [0, 0] and h.mamba_fp8_plan(5) == [1, 1]

    def refused(eng, rc_want, text, layer, *p):
        with torch.cuda.device(eng.device):
            rc = eng.lib.zn_set_mamba_fp8(eng.h, layer, *p)
        msg = eng.lib.zn_last_error(eng.h).decode()
        assert rc == rc_want and text in msg, (rc, msg)

    # ZN_FP8_VERIFY=1 is set throughout: a refusal comes before the verification launches, and attaches nothing
    monkeypatch.setenv("ZN_FP8_VERIFY", "1")
    plain, _ = build_model(synth.TINY_CFG, 5, DEV)
    pe = HipEngine(plain.backbone, max_rows=8)
    refused(pe, -4, "transformer", 0, *ptrs)
    assert pe.mamba_fp8_plan(8) == [0, 0]
    fresh = HipEngine(A.backbone, max_rows=8)
    fresh.call("zn_set_mamba_fp8", 0, None, None, None, None)
    assert fresh.mamba_fp8_plan(8) == [0, 0]
    refused(fresh, -4, "attention layer", 1, *ptrs)
    refused(fresh, -1, "all four pointers", 0, ptrs[0], None, ptrs[2], ptrs[3])
    refused(fresh, -1, "out of range", 2, *ptrs)
    refused(fresh, -1, "out of range", -1, *ptrs)
    assert fresh.mamba_fp8_plan(8) == [0, 0], "a refused call attached something"
    # the contract holds on the model's own weights: accepted; one flipped code: ZN_ERR_ARG, and nothing is attached
    flipped = mx.in_proj_q.clone()
    flipped[8511, 2047] ^= 0x01
    torch.cuda.synchronize()
    refused(fresh, -1, "not the dequantised stream", 0, flipped.data_ptr(), *ptrs[1:])
    assert fresh.mamba_fp8_plan(8) == [0, 0]
    flipped_out = mx.out_proj_q.clone()
    flipped_out[0, 0] ^= 0x01
    torch.cuda.synchronize()
    refused(fresh, -1, "not the dequantised stream", 0, ptrs[0], ptrs[1], flipped_out.data_ptr(), ptrs[3])
    assert fresh.mamba_fp8_plan(8) == [0, 0]
    fresh.call("zn_set_mamba_fp8", 0, *ptrs)
    assert fresh.mamba_fp8_plan(8) == [1, 1]
    monkeypatch.delenv("ZN_FP8_VERIFY")
    # inside a generation
    d = WIDE_CFG["d_model"]
    reqs = [GenRequest(synth.conditioning(900 + i, "mfp8.state", 2, 4, d).to(DEV), sampling_params=dict(temperature=0.0), cfg_scale=2.0, max_new_tokens=4) for i in range(2)]
    gen = A.serve(iter(reqs), slots=4, max_prompt=8, max_new_tokens=4, guided=True)
    next(gen)
    assert A.engine(4) is h
    refused(h, -3, "inside a generation", 0, *ptrs)
    refused(h, -3, "inside a generation", 0, None, None, None, None)
    gen.close()
    assert h.mamba_fp8_plan(8) == [1, 1]
    # detach, attach again; the tune key
    h.call("zn_set_mamba_fp8", 0, None, None, None, None)
    assert h.mamba_fp8_plan(8) == [0, 0] and A.mamba_fp8_plan(8) == {"in_proj": False, "out_proj": False}
    h.call("zn_set_mamba_fp8", 0, *ptrs)
    assert h.mamba_fp8_plan(8) == [1, 1] and A.mamba_fp8_plan(8) == {"in_proj": True, "out_proj": True}
    h.call("zn_debug_tune", tune_key(), 2)
    assert h.mamba_fp8_plan(8) == [0, 0]
    h.call("zn_debug_tune", tune_key(), 1)
    assert h.mamba_fp8_plan(8) == [1, 1] and h.mamba_fp8_plan(64) == [1, 1]
    out2 = (C.c_int32 * 2)(7, 7)
    assert h.lib.zn_mamba_fp8_plan(h.h, 0, out2) == -1


# ---------------------------------------------------------------------------------------------- 3. end to end
STEPS = 8


def run_generate(model, B):
    d = WIDE_CFG["d_model"]
    cond = torch.cat([synth.conditioning(700 + i, "mfp8.e2e", 2, 6, d) for i in range(B)], 0)
    cond = torch.cat([cond[0::2], cond[1::2]], 0).to(DEV)                           # [cond rows | uncond rows]
    tr = {"logits": []}
    out = model.generate(cond, max_new_tokens=STEPS, cfg_scale=2.0, batch_size=B, sampling_params=dict(temperature=0.0), _trace=tr)
    torch.cuda.synchronize()
    return [out.cpu()], [l.cpu() for l in tr["logits"]]


def run_batch(model):
    d = WIDE_CFG["d_model"]
    reqs = [GenRequest(synth.conditioning(800 + i, "mfp8.batch", 2, 3 + i % 4, d).to(DEV), sampling_params=dict(temperature=0.0, repetition_penalty=1.0 + 0.5 * (i % 3)) if i % 2 else
                       dict(temperature=0.9, min_p=0.05 * (1 + i % 3)), seed=None if i % 2 else 40 + i, cfg_scale=[2.0, 1.5, 3.0][i % 3], max_new_tokens=8 - i % 3) for i in range(16)]
    tr = {"logits": []}
    outs = model.generate_batch(reqs, _trace=tr)
    torch.cuda.synchronize()
    assert tr["logits"][0].shape[0] == 16
    return [o.cpu() for o in outs], [l.cpu() for l in tr["logits"]]


def run_serve(model):
    d = WIDE_CFG["d_model"]
    reqs = []
    for i in range(16):
        guided = i % 3 != 2
        reqs.append(GenRequest(synth.conditioning(900 + i, "mfp8.serve", 2 if guided else 1, 4 + i % 3, d).to(DEV), sampling_params=dict(temperature=0.0) if i % 2 else
                               dict(temperature=0.8, min_p=0.1), seed=None if i % 2 else 60 + i, cfg_scale=[2.0, 1.5][i % 2] if guided else 1.0, max_new_tokens=5 + i % 5))
    tr = {}
    out = {r.index: r for r in model.serve(iter(reqs), slots=24, max_prompt=8, max_new_tokens=10, guided=None, sched_every=3, _trace=tr)}
    torch.cuda.synchronize()
    assert sorted(out) == list(range(16)) and all(r.error is None for r in out.values())
    assert tr["logits"][-1].shape[0] == 24
    return [out[i].codes.cpu() for i in range(16)], [l.cpu() for l in tr["logits"]]


CASES = {"generate.1": lambda m: run_generate(m, 1), "generate.2": lambda m: run_generate(m, 2), "generate.3": lambda m: run_generate(m, 3), "generate.9": lambda m: run_generate(m, 9),
         "generate_batch": run_batch, "serve": run_serve}
CASE_ROWS = {"generate.1": 2, "generate.2": 4, "generate.3": 6, "generate.9": 18, "generate_batch": 32, "serve": 24}


@pytest.mark.parametrize("case", list(CASES))
def test_generation_equals_the_bf16_model_on_the_dequantised_weights(case):
    tune_key()
    A, Cm = get_built()["wide"]["A"], get_built()["wide"]["C"]
    rows = CASE_ROWS[case]
    runs = {}
    for name, model in (("a", A), ("c", Cm)):
        eng = model.engine(16)
        reads = rows > 4 and name == "a"
        assert eng.mamba_fp8_plan(rows) == ([1, 1] if reads else [0, 0]), (case, name)
        assert model.mamba_fp8_plan(rows) == {"in_proj": reads, "out_proj": reads}
        eng.call("zn_debug_eos_bias", float("-inf"))
        try:
            runs[name] = CASES[case](model)
        finally:
            eng.call("zn_debug_eos_bias", 0.0)
        c = eng.counters()
        assert c["handoff_timeouts"] == 0 and c["demoted"] == 0, c
    got, ref = runs["a"], runs["c"]
    assert len(got[0]) == len(ref[0]) and len(got[1]) == len(ref[1]) and len(ref[1]) >= 5
    for i, (x, y) in enumerate(zip(got[0], ref[0])):
        assert x.shape == y.shape and torch.equal(x, y), f"{case}: codes of result {i} differ from the plain bf16 model"
    for i, (x, y) in enumerate(zip(got[1], ref[1])):
        assert x.shape == y.shape and torch.equal(bits(x), bits(y)), f"{case}: logits of step {i} differ from the plain bf16 model"


# ---------------------------------------------------------------------------------------------- 4. other widths
def test_other_widths_are_refused_and_nothing_changes():
    tune_key()
    tiny, _ = build_model(synth.HYBRID_TINY_CFG, 23, DEV)
    before = {k: v.clone() for k, v in tiny.state_dict().items()}
    with pytest.raises(_lib.ZonosHipError, match="d_model 2048 and d_inner 4096"):
        tiny.quantize_mamba_fp8()
    assert tiny.mamba_weights == "bf16" and not hasattr(mamba_mixers(tiny)[0], "in_proj_q")
    after = tiny.state_dict()
    assert all(torch.equal(bits(before[k]), bits(after[k])) for k in before)
    assert tiny.mamba_fp8_plan(8) == {"in_proj": False, "out_proj": False}
    # the library's own refusal
    h = HipEngine(tiny.backbone, max_rows=8)
    mx = mamba_mixers(tiny)[0]
    q1, q2 = torch.zeros(mx.in_proj.weight.shape, dtype=torch.uint8, device=DEV), torch.zeros(mx.out_proj.weight.shape, dtype=torch.uint8, device=DEV)
    e1, e2 = torch.zeros(q1.shape[0], dtype=torch.int8, device=DEV), torch.zeros(q2.shape[0], dtype=torch.int8, device=DEV)
    with torch.cuda.device(h.device):
        rc = h.lib.zn_set_mamba_fp8(h.h, 0, q1.data_ptr(), e1.data_ptr(), q2.data_ptr(), e2.data_ptr())
    assert rc == -4 and "d_model 2048 and d_inner 4096" in h.lib.zn_last_error(h.h).decode()
    assert h.mamba_fp8_plan(8) == [0, 0]


# ---------------------------------------------------------------------------------------------- 5. the default changes nothing
def test_bf16_mode_leaves_the_parameters_untouched(tmp_path):
    """from_local(mamba_weights="bf16") - the default - loads the checkpoint's bits; on a transformer checkpoint "fp8" and quantize_mamba_fp8() raise; any other
    value is refused."""
    tune_key()
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
    paths = (str(tmp_path / "config.json"), str(tmp_path / "model.safetensors"))
    plain = Zonos.from_local(*paths, DEV)
    same = Zonos.from_local(*paths, DEV, mamba_weights="bf16")
    assert plain.mamba_weights == same.mamba_weights == "bf16"
    ps, ss = plain.state_dict(), same.state_dict()
    assert set(ps) == set(ss)
    for k in ps:
        assert torch.equal(bits(ps[k]), bits(ss[k])), k
    with pytest.raises(_lib.ZonosHipError, match="transformer"):
        Zonos.from_local(*paths, DEV, mamba_weights="fp8")
    with pytest.raises(_lib.ZonosHipError, match="transformer"):
        same.quantize_mamba_fp8()
    assert same.mamba_weights == "bf16" and all(torch.equal(bits(ps[k]), bits(v)) for k, v in same.state_dict().items())
    with pytest.raises(_lib.ZonosHipError, match="mamba_weights"):
        Zonos.from_local(*paths, DEV, mamba_weights="int8")
