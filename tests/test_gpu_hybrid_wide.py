"""The Mamba2 in_proj of a hybrid decode step of 17..64 rows reads its weights once per step (ZN_TUNE_WIDE_HYBRID): row groups on the
grid of gemm16k_kernel (= 2) or the row-tile loop gemm16k_rows_kernel (= 3), against groups of 16 rows (= 1).  The bar between the forms is equality
of the raw bits (int16 / int32 views, torch.equal):
  1. per op through zn_op_mamba_step on layer 0 of a two-layer model of the production widths (N = 8512) and of one with d_state 64 and two groups
     (N = 8384, the gated norm over two groups): 17 .. 80 rows, three consecutive tokens from random states that differ from row to row, the state
     buffer between canary regions, the output between canary rows and pre-filled with NaN; = 1, 2, 3 and the key unset;
  2. one anchor outside HIP against HIP: a token at 33 rows under the default against oracle.zonos_oracle.mamba2_step, at the bars of
     tests/test_gpu_hybrid.py::test_mamba2_step_vs_oracle;
  3. generate() at 18 and 34 rows, a 16-request generate_batch() and a mixed serve() session of 24 rows: codes and per-step logits;
  4. zn_hybrid_rows_plan: the step really is planned that way."""
import ctypes as C

import pytest
import torch

from oracle import zonos_oracle as zo
from zonos_amd import _lib, synth
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
ROWS = (17, 32, 33, 48, 64, 65, 80)
FORMS = (1, 2, 3)
HAS_FEATURE = hasattr(_lib, "ZN_TUNE_WIDE_HYBRID")


def tune_key():
    assert HAS_FEATURE, "this library has no ZN_TUNE_WIDE_HYBRID"
    return _lib.ZN_TUNE_WIDE_HYBRID


def bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


@pytest.fixture(scope="module")
def built():
    out = {}
    for name, cfg in CFGS.items():
        model, sd = build_model(cfg, 11, DEV)
        # two handles of 80 rows for the per-op cases: one whose key is never set (zn_debug_tune cannot unset a key), one the cases set to 1, 2 and 3
        model._op_engines = (HipEngine(model.backbone, max_rows=80), HipEngine(model.backbone, max_rows=80))
        out[name] = (model, sd, mamba2_dims(model.config.backbone))
    return out


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


# ---------------------------------------------------------------------------------------------- 1. per op
@pytest.mark.parametrize("rows", ROWS + (5, 16))
@pytest.mark.parametrize("cfg_name", list(CFGS))
def test_mamba_step_bits_equal_across_forms(built, cfg_name, rows):
    """= 1, 2, 3 and the key unset (a handle of its own): output, conv window and SSM state bit-equal after every one of
    three tokens; at 5 and 16 rows the key changes nothing."""
    key = tune_key()
    model, _, m = built[cfg_name]
    d = CFGS[cfg_name]["d_model"]
    unset, tuned = model._op_engines
    gen = torch.Generator(device=DEV).manual_seed(500 + rows)
    xs = [torch.randn((rows, d), generator=gen, device=DEV, dtype=torch.float32).to(bf) for _ in range(3)]
    ref = None
    for form in (1, None, 2, 3):                     # groups of 16 first: what every other form is compared with
        eng = unset if form is None else tuned
        if form is not None:
            eng.call("zn_debug_tune", key, form)
        plan = eng.hybrid_rows_plan(rows)
        assert plan["mamba_in_proj"] == (16 if rows <= 16 or form == 1 else 64) and plan["mamba_out_proj"] == (64 if rows > 16 else 16), (form, rows, plan)
        st = State(eng, m, rows, d, seed=900 + rows)
        snaps = []
        for t, x in enumerate(xs):
            st.step(eng, x)
            st.check(f"{cfg_name} rows {rows} form {form} token {t}")
            snaps.append((st.out[PAD:-PAD].clone(), st.state.clone()))
        if ref is None:
            ref = snaps
            continue
        nc = st.n_conv
        for t in range(3):
            assert torch.equal(bits(snaps[t][0]), bits(ref[t][0])), f"{cfg_name} rows {rows}: output of form {form} differs from groups of 16 at token {t}"
            assert torch.equal(bits(snaps[t][1][:nc]), bits(ref[t][1][:nc])), f"{cfg_name} rows {rows}: conv window of form {form} differs at token {t}"
            assert torch.equal(bits(snaps[t][1][nc:]), bits(ref[t][1][nc:])), f"{cfg_name} rows {rows}: SSM state of form {form} differs at token {t}"
    # the tokens moved the state, and the rows differ (a row group served from another group's window would show above only if they do)
    assert not torch.equal(ref[0][1], ref[2][1]) and not torch.equal(ref[2][0][0], ref[2][0][rows - 1])


# ---------------------------------------------------------------------------------------------- 2. the anchor outside HIP against HIP
def test_mamba_step_33_rows_default_vs_oracle(built):
    """One token at 33 rows (three row tiles, the last of one row) under the default form against the CPU restatement, at the bars of
    tests/test_gpu_hybrid.py::test_mamba2_step_vs_oracle: bit-equal fractions > 0.98 (window, state) / > 0.8 (output), max |diff| <= 2^-6 of the output scale."""
    tune_key()
    model, sd, m = built["wide"]
    eng = HipEngine(model.backbone, max_rows=34)
    assert eng.hybrid_rows_plan(33)["mamba_in_proj"] == 64
    R, d = 33, WIDE_CFG["d_model"]
    conv = torch.from_numpy(synth.normal(11, "hw.conv0", (R, m["conv_dim"], m["d_conv"]))).to(bf)
    ssm = torch.from_numpy(synth.normal(11, "hw.ssm0", (R, m["nheads"], m["headdim"], m["d_state"]))).to(bf)
    n_conv = conv.numel()
    buf = torch.cat([conv.flatten(), ssm.flatten()]).to(DEV)
    x = torch.from_numpy(synth.normal(11, "hw.x0", (R, d))).to(bf)
    ref = zo.mamba2_step(sd, "backbone.layers.0.mixer.", x, conv, ssm, zo.mamba2_dims(dict(WIDE_CFG)))      # conv, ssm: advanced in place
    xd = x.to(DEV)
    out = torch.empty_like(xd)
    eng.call("zn_op_mamba_step", 0, xd.data_ptr(), buf.data_ptr(), out.data_ptr(), R, _lib.stream_ptr())
    torch.cuda.synchronize()
    got, gconv, gssm = out.cpu(), buf[:n_conv].cpu().view_as(conv), buf[n_conv:].cpu().view_as(ssm)
    eq = float((bits(got) == bits(ref)).float().mean())
    ceq = float((bits(gconv) == bits(conv)).float().mean())
    seq = float((bits(gssm) == bits(ssm)).float().mean())
    md = (got.float() - ref.float()).abs().max().item()
    print(f"\n[mamba2 33 rows, default form] out bit-equal {eq:.4f} max|d| {md:.3g} (|ref| max {ref.float().abs().max():.3g}); window bit-equal {ceq:.5f}; state bit-equal {seq:.5f}")
    assert ceq > 0.98 and seq > 0.98 and eq > 0.8, (ceq, seq, eq)
    assert md <= 2.0 ** -6 * max(1.0, ref.float().abs().max().item())


# ---------------------------------------------------------------------------------------------- 3. end to end
def run_generate(model, B):
    d = WIDE_CFG["d_model"]
    cond = torch.cat([synth.conditioning(700 + i, "hw.e2e", 2, 6, d) for i in range(B)], 0)
    cond = torch.cat([cond[0::2], cond[1::2]], 0).to(DEV)                           # [cond rows | uncond rows]
    tr = {"logits": []}
    out = model.generate(cond, max_new_tokens=6, cfg_scale=2.0, batch_size=B, sampling_params=dict(temperature=0.0), _trace=tr)
    torch.cuda.synchronize()
    return [out.cpu()], [l.cpu() for l in tr["logits"]]


def run_batch(model):
    d = WIDE_CFG["d_model"]
    reqs = [GenRequest(synth.conditioning(800 + i, "hw.batch", 2, 3 + i % 4, d).to(DEV), sampling_params=dict(temperature=0.0, repetition_penalty=1.0 + 0.5 * (i % 3)) if i % 2 else
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
        reqs.append(GenRequest(synth.conditioning(900 + i, "hw.serve", 2 if guided else 1, 4 + i % 3, d).to(DEV), sampling_params=dict(temperature=0.0) if i % 2 else
                               dict(temperature=0.8, min_p=0.1), seed=None if i % 2 else 60 + i, cfg_scale=[2.0, 1.5][i % 2] if guided else 1.0, max_new_tokens=5 + i % 5))
    tr = {}
    out = {r.index: r for r in model.serve(iter(reqs), slots=24, max_prompt=8, max_new_tokens=10, guided=None, sched_every=3, _trace=tr)}
    torch.cuda.synchronize()
    assert sorted(out) == list(range(16)) and all(r.error is None for r in out.values())
    assert tr["logits"][-1].shape[0] == 24
    return [out[i].codes.cpu() for i in range(16)], [l.cpu() for l in tr["logits"]]


CASES = {"generate.9": lambda m: run_generate(m, 9), "generate.17": lambda m: run_generate(m, 17), "generate_batch": run_batch, "serve": run_serve}
CASE_ROWS = {"generate.9": 18, "generate.17": 34, "generate_batch": 32, "serve": 24}


@pytest.mark.parametrize("case", list(CASES))
def test_generation_equal_across_forms(built, case):
    """The default (a new handle), then ZN_TUNE_WIDE_HYBRID = 1, 2 and 3 on it: codes and per-step logits."""
    key = tune_key()
    model = built["wide"][0]
    with model._spare_guard:
        model._engine = model._spare = None
    eng = model.engine(17)
    eng.call("zn_debug_eos_bias", float("-inf"))
    rows = CASE_ROWS[case]
    runs = {}
    try:
        for form in (None,) + FORMS:
            if form is not None:
                eng.call("zn_debug_tune", key, form)
            assert eng.hybrid_rows_plan(rows)["mamba_in_proj"] == (16 if form == 1 else 64), (case, form)
            runs[form] = CASES[case](model)
            assert model.engine(17) is eng
    finally:
        eng.call("zn_debug_eos_bias", 0.0)
    ref = runs[1]
    assert len(ref[1]) >= 6
    for form in (None, 2, 3):
        got = runs[form]
        assert len(got[0]) == len(ref[0]) and len(got[1]) == len(ref[1])
        for i, (a, b) in enumerate(zip(got[0], ref[0])):
            assert a.shape == b.shape and torch.equal(a, b), f"{case} form {form}: codes of result {i} differ from groups of 16"
        for i, (a, b) in enumerate(zip(got[1], ref[1])):
            assert a.shape == b.shape and torch.equal(bits(a), bits(b)), f"{case} form {form}: logits of step {i} differ from groups of 16"
    c = eng.counters()
    assert c["handoff_timeouts"] == 0 and c["demoted"] == 0, c


# ---------------------------------------------------------------------------------------------- 4. the plan report
def test_hybrid_rows_plan(built):
    assert hasattr(_lib.load(), "zn_hybrid_rows_plan") and tune_key() == 22
    model = built["wide"][0]
    eng = HipEngine(model.backbone, max_rows=64)
    names = ["mamba_in_proj", "mamba_out_proj", "in_proj", "out_proj", "fc1", "fc2", "heads"]
    for rows in (32, 64):
        p = eng.hybrid_rows_plan(rows)
        assert list(p) == names
        assert p["mamba_in_proj"] == 64 and p["mamba_out_proj"] == 64 and p["fc2"] == 16, (rows, p)       # (fc2 of the attention layers: store on the LDS-staged kernel, per 16)
        assert p["in_proj"] == 64 and p["out_proj"] == 64 and p["fc1"] == 64 and p["heads"] == 64, (rows, p)
    assert list(eng.hybrid_rows_plan(16).values()) == [16] * 7
    assert list(eng.hybrid_rows_plan(2).values()) == [4] * 7
    eng.call("zn_debug_tune", tune_key(), 1)
    for rows in (32, 64):
        p = eng.hybrid_rows_plan(rows)
        assert p["mamba_in_proj"] == 16 and p["mamba_out_proj"] == 64, (rows, p)
    for form in (2, 3):
        eng.call("zn_debug_tune", tune_key(), form)
        assert eng.hybrid_rows_plan(32)["mamba_in_proj"] == 64 and eng.hybrid_rows_plan(16)["mamba_in_proj"] == 16
    eng.call("zn_debug_tune", _lib.ZN_TUNE_WIDE_ROWS, 1)
    assert list(eng.hybrid_rows_plan(64).values()) == [16] * 7
    # the same through the model; a transformer model has no such report
    assert model.hybrid_rows_plan(32)["mamba_in_proj"] == 64
    plain, _ = build_model(synth.TINY_CFG, 5, DEV)
    with pytest.raises(_lib.ZonosHipError):
        plain.hybrid_rows_plan(32)
