"""The FP8 KV cache (Zonos.set_kv_cache("fp8"), zn_set_kv_fp8) on the device, bit for bit:
  1. the appends, per op: with a code cache bound, zn_op_linear_fused's RoPE + KV epilogue (decode at 5, 16, 17 and 64 rows, prefill) and
     rope_kv_rows_kernel leave kv_round_e4m3 of what they leave without it in the bf16 cache and its codes in the code cache, q untouched, nothing
     at a position equal to max_len, guard bytes around both caches intact; the inputs reach beyond +-448 and below 2^-9;
  2. the attention, per op: the FP8 form equals the bf16 form reading the dequantised cache at every head size and group the attention is
     instantiated for, rows 5 / 16 / 17 / 64, contexts 1 .. max_len, both launch shapes, both column splits, rows of different lengths in one call,
     large finite garbage past every row's length in both caches - and stays inside the float64 interval of zonos_amd.testing.attention_reference
     on the dequantised K/V (the operands are identical, so the bound of tests/test_gpu_attention.py applies unchanged);
  3. end to end on a tiny transformer: codes and per-step logits with the mode on equal the same model under ZN_TUNE_KV_FP8 = 2 (the attention
     reads the bf16 cache) through generate(), generate_batch(), serve() and serve_stream(); one and two utterances equal the mode-off model;
  4. a negative control: with codes that differ from the bf16 cache the mode-on output follows the codes and the = 2 output the bf16 cache."""
import ctypes as C

import pytest
import torch

from zonos_amd import _lib, synth
from zonos_amd import quant as Q
from zonos_amd import testing as T
from zonos_amd.autoencoder import DACAutoencoder
from zonos_amd.backbone import HipEngine
from zonos_amd.model import GenRequest
from zonos_amd.testing import LF_PRO_LN, LF_PRO_NONE, LF_ROPE_KV, attention_compare, attention_reference, build_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
bf = torch.bfloat16
PAD = 4096                       # guard elements in front of and behind each cache
KV_CANARY, CODE_CANARY = 768.0, 0xA5


def bits(t):
    return t.view(torch.int16)


# ---------------------------------------------------------------------------------------------- 1. the appends
NQ, NK, NQKV, KIN = 2048, 512, 3072, 2048


@pytest.fixture(scope="module")
def lin_engines():
    out = {}
    for hd, (h, hkv) in {128: (16, 4), 64: (32, 8)}.items():
        model, _ = build_model(dict(d_model=2048, n_layer=1, num_heads=h, num_heads_kv=hkv, d_ff=256), 31, DEV)
        out[hd] = HipEngine(model.backbone, max_rows=64)
        out[hd]._model = model
    return out


@pytest.fixture(scope="module")
def lin_weights():
    """in_proj-shaped weights whose output features come in pairs of scale 1, 1, 4096 and 2^-10: K and V beyond +-448 and below 2^-9 in every row."""
    W = torch.from_numpy(synth.uniform(61, "kv8.w", (NQKV, KIN), 1.0 / KIN ** 0.5))
    s = torch.tensor([1.0, 1.0, 4096.0, 2.0 ** -10])[(torch.arange(NQKV) // 2) % 4]
    t = dict(W=(W * s[:, None]).to(bf), ln_w=(1.0 + torch.from_numpy(synth.uniform(61, "kv8.lnw", (KIN,), 0.3))).to(bf),
             ln_b=torch.from_numpy(synth.uniform(61, "kv8.lnb", (KIN,), 0.2)).to(bf))
    return {k: v.to(DEV).contiguous() for k, v in t.items()}


class GuardedCache:
    """A bf16 cache [rows][max_len][2][NK] of seeded finite values and its code cache, each between PAD guard elements."""

    def __init__(self, rows, max_len, tag):
        n = rows * max_len * 2 * NK
        self.shape = (rows, max_len, 2, NK)
        self.kv0 = torch.from_numpy(synth.normal(62, f"kv8.cache.{tag}.{rows}.{max_len}", self.shape)).to(bf).to(DEV)
        self.kvbuf = torch.full((n + 2 * PAD,), KV_CANARY, dtype=bf, device=DEV)
        self.cbuf = torch.full((n + 2 * PAD,), CODE_CANARY, dtype=torch.uint8, device=DEV)
        self.kv, self.codes = self.kvbuf[PAD:PAD + n].view(self.shape), self.cbuf[PAD:PAD + n].view(self.shape)
        self.reset()

    def reset(self):
        self.kv.copy_(self.kv0)
        self.codes.fill_(CODE_CANARY)

    def guards_intact(self, label):
        assert bool((self.kvbuf[:PAD] == KV_CANARY).all()) and bool((self.kvbuf[-PAD:] == KV_CANARY).all()), f"{label}: a guard of the bf16 cache was written"
        assert bool((self.cbuf[:PAD] == CODE_CANARY).all()) and bool((self.cbuf[-PAD:] == CODE_CANARY).all()), f"{label}: a guard of the code cache was written"


def check_append(cache, kv_off, kv_on, codes_on, cr, pos, label):
    """kv_off / kv_on: the bf16 cache after the op without / with the code cache bound (CPU); (cr, pos): cache row and position per activation row."""
    max_len = cache.shape[1]
    fits = pos < max_len
    assert bool((~fits).any()) and bool(fits.any()), f"{label}: the case must append somewhere and meet the capacity somewhere"
    touched = torch.zeros(cache.shape[:2], dtype=torch.bool)
    touched[cr[fits], pos[fits]] = True
    kv0 = cache.kv0.cpu()
    assert torch.equal(bits(kv_off)[~touched], bits(kv0)[~touched]) and torch.equal(bits(kv_on)[~touched], bits(kv0)[~touched]), f"{label}: a position that was not appended changed"
    assert bool((codes_on[~touched] == CODE_CANARY).all()), f"{label}: codes were written at a position that was not appended"
    app = kv_off[touched]
    assert bool(torch.isfinite(app.float()).all()) and float(app.float().abs().max()) > 448 and float(app.float().abs()[app != 0].min()) < 2.0 ** -9, label
    q, dq = Q.kv_round_e4m3(app)
    assert not torch.equal(bits(dq), bits(app)), f"{label}: the rounding must change something (it is lossy)"
    assert torch.equal(bits(kv_on[touched]), bits(dq)), f"{label}: the bf16 cache is not kv_round_e4m3 of the mode-off cache"
    assert torch.equal(codes_on[touched], q), f"{label}: the code cache does not hold the codes"


def run_linear(eng, w, cache, pro, rows, x, lengths=None, prefill=0, pf_S=0, pf_base=0, bound=True, out=None):
    st = _lib.stream_ptr()
    q_out = torch.full((rows, NQ), float("nan"), dtype=bf, device=DEV)
    op = _lib.zn_linear_op(pro=pro, epi=LF_ROPE_KV, rows=rows, N=NQKV, K=KIN, prefill=prefill, target_blocks=4, max_len=cache.shape[1], pf_S=pf_S, pf_base=pf_base)
    op.x, op.W, op.kv, op.q_out = x.data_ptr(), w["W"].data_ptr(), cache.kv.data_ptr(), q_out.data_ptr()
    if pro == LF_PRO_LN:
        op.ln_w, op.ln_b = w["ln_w"].data_ptr(), w["ln_b"].data_ptr()
    if lengths is not None:
        op.lengths = lengths.data_ptr()
    if out is not None:
        op.out = out.data_ptr()
    eng.call("zn_op_bind_kv_fp8", cache.codes.data_ptr() if bound else None)
    try:
        eng.call("zn_op_linear_fused", C.byref(op), st)
        torch.cuda.synchronize()
    finally:
        eng.call("zn_op_bind_kv_fp8", None)
    assert op.plan_dict()["err"] == 0
    return q_out.cpu(), op.plan_dict()


def _x(rows, tag):
    scale = torch.linspace(0.5, 3.0, rows)[:, None]
    return (torch.from_numpy(synth.normal(63, f"kv8.x.{tag}.{rows}", (rows, KIN))) * scale).to(bf).to(DEV)


@pytest.mark.parametrize("rows,wide", [(5, 0), (16, 0), (17, 0), (17, 1), (64, 0), (64, 1)])
def test_decode_append_rounds_and_writes_both_caches(lin_engines, lin_weights, rows, wide):
    """gemv_epilogue<EPI_ROPE_KV> as the 5..64-row projection kernels use it: groups of 16 rows (17 = 16 + a one-row GEMV launch), and up to 64 rows per
    weight pass (ZN_TUNE_WIDE_ROWS = 2: the row groups on the grid), with and without the LayerNorm prologue, at both head sizes."""
    L = 16
    lens = torch.tensor([(0, 5, L - 1)[r % 3] if r < rows - 1 else L for r in range(rows)])           # the last row sits at the capacity
    cr = torch.arange(rows)
    for hd in (128, 64) if rows in (5, 17) else (128,):
        eng = lin_engines[hd]
        if wide:
            eng.call("zn_debug_tune", _lib.ZN_TUNE_WIDE_ROWS, 2)
        try:
            for pro in (LF_PRO_LN, LF_PRO_NONE):
                label = f"decode hd{hd} rows {rows} wide {wide} pro {pro}"
                cache, x, ld = GuardedCache(rows + 1, L, "d"), _x(rows, "d"), lens.to(torch.int32).to(DEV)
                q_off, plan = run_linear(eng, lin_weights, cache, pro, rows, x, lengths=ld, bound=False)
                kv_off = cache.kv.cpu()
                assert bool((cache.codes == CODE_CANARY).all()), f"{label}: codes written without a code cache bound"
                cache.guards_intact(label)
                cache.reset()
                q_on, plan_on = run_linear(eng, lin_weights, cache, pro, rows, x, lengths=ld, bound=True)
                assert plan_on == plan and (rows <= 16 or plan["rows_per_launch"] == (64 if wide else 16)), (label, plan)
                cache.guards_intact(label)
                assert bool(torch.isfinite(q_off.float()).all()) and torch.equal(bits(q_on), bits(q_off)), f"{label}: q must not change"
                check_append(cache, kv_off, cache.kv.cpu(), cache.codes.cpu(), cr, lens, label)
        finally:
            if wide:
                eng.call("zn_debug_tune", _lib.ZN_TUNE_WIDE_ROWS, 1)


@pytest.mark.parametrize("rows,S,base", [(34, 17, 3), (64, 32, 0)])
def test_prefill_append_in_the_epilogue_and_in_rope_kv_rows(lin_engines, lin_weights, rows, S, base):
    """The prefill appends: gemm16k_kernel<EPI_ROPE_KV> over the rows of a short prefill, then the plain projection followed by rope_kv_rows_kernel
    (ZN_TUNE_NO_PREFILL_GEMM16K = 2 sends the projection to the kernels that leave RoPE to it), whose last positions lie at or past max_len."""
    eng, st, R = lin_engines[128], _lib.stream_ptr(), rows // S
    x = _x(rows, "p")
    m = torch.arange(rows)
    cr = m // S
    # 1. in the epilogue (the entry point wants base + S <= max_len: the capacity is met in form 2)
    cache = GuardedCache(R + 1, base + S + 3, "p")
    out = torch.full((rows, NQKV), float("nan"), dtype=bf, device=DEV)
    q_off, plan = run_linear(eng, lin_weights, cache, LF_PRO_NONE, rows, x, prefill=1, pf_S=S, pf_base=base, bound=False, out=out)
    assert plan["rope_done"] == 1 and plan["kernel"] == "GEMM16K", plan
    kv_off = cache.kv.cpu()
    cache.reset()
    q_on, _ = run_linear(eng, lin_weights, cache, LF_PRO_NONE, rows, x, prefill=1, pf_S=S, pf_base=base, bound=True, out=out)
    cache.guards_intact("prefill epilogue")
    assert torch.equal(bits(q_on), bits(q_off))
    pos = base + m % S
    touched = torch.zeros(cache.shape[:2], dtype=torch.bool)
    touched[cr, pos] = True
    app = kv_off[touched]
    q, dq = Q.kv_round_e4m3(app)
    assert float(app.float().abs().max()) > 448 and torch.equal(bits(cache.kv.cpu()[touched]), bits(dq)) and torch.equal(cache.codes.cpu()[touched], q)
    assert torch.equal(bits(cache.kv.cpu()[~touched]), bits(cache.kv0.cpu()[~touched])) and bool((cache.codes.cpu()[~touched] == CODE_CANARY).all())
    # 2. projection, then rope_kv_rows_kernel; max_len = base + S - 2: the last two positions of every row write nothing
    eng.call("zn_debug_tune", _lib.ZN_TUNE_NO_PREFILL_GEMM16K, 2)
    try:
        cache = GuardedCache(R + 1, base + S + 3, "p2")
        _, plan = run_linear(eng, lin_weights, cache, LF_PRO_NONE, rows, x, prefill=1, pf_S=S, pf_base=base, bound=True, out=out)
    finally:
        eng.call("zn_debug_tune", _lib.ZN_TUNE_NO_PREFILL_GEMM16K, 1)
    assert plan["rope_done"] == 0 and bool(torch.isfinite(out.float()).all()), plan
    assert torch.equal(bits(cache.kv), bits(cache.kv0)) and bool((cache.codes == CODE_CANARY).all()), "a plan that leaves RoPE to a later kernel appends nothing"
    max_len = base + S - 2
    cache = GuardedCache(R + 1, max_len, "p3")
    qkv_off, qkv_on = out.clone(), out.clone()
    eng.call("zn_op_rope_kv_rows", qkv_off.data_ptr(), cache.kv.data_ptr(), max_len, S, base, R, st)
    torch.cuda.synchronize()
    kv_off = cache.kv.cpu()
    assert bool((cache.codes == CODE_CANARY).all())
    cache.reset()
    eng.call("zn_op_bind_kv_fp8", cache.codes.data_ptr())
    try:
        eng.call("zn_op_rope_kv_rows", qkv_on.data_ptr(), cache.kv.data_ptr(), max_len, S, base, R, st)
        torch.cuda.synchronize()
    finally:
        eng.call("zn_op_bind_kv_fp8", None)
    cache.guards_intact("rope_kv_rows")
    assert torch.equal(bits(qkv_on), bits(qkv_off)) and not torch.equal(bits(qkv_on[:, :NQ]), bits(out[:, :NQ])), "q is rotated in place, the same with and without the code cache"
    check_append(cache, kv_off, cache.kv.cpu(), cache.codes.cpu(), cr, pos, "rope_kv_rows")


# ---------------------------------------------------------------------------------------------- 2. the attention
AT_ROWS = 64
LENS_512 = (1, 15, 16, 17, 63, 64, 65, 511, 512, 300, 2, 449, 128)                 # keys per row; 511 = max_len - 1, 512 = max_len
LENS_1032 = (1, 15, 16, 17, 63, 64, 65, 511, 512, 513, 1025, 1031, 1032)            # ... 1031 = max_len - 1: the second and third key blocks
WINDOWS = ((5, 0), (5, 5), (5, 8), (16, 0), (17, 3), (64, 0))                       # (rows, first row): between them the 5-row calls meet all 13 contexts


def _pool():
    """bf16 values on the E4M3 grid and their codes: N(0, 1) draws rounded by the specification."""
    x = torch.from_numpy(synth.normal(64, "kv8.pool", (1 << 16,))).to(bf)
    q, dq = Q.kv_round_e4m3(x)
    return q, dq


class AttnOperands:
    """One geometry at one capacity: 64 rows of q, a dequantised K/V cache with its codes (garbage past every row's length in both), the float64
    interval on the dequantised values, and a second, different cache for the negative control."""

    def __init__(self, hd, G, cap, lens13, pool):
        hq, hkv = T.AT_GEOM[(hd, G)]
        self.hd, self.G, self.cap, self.hq, self.hkv = hd, G, cap, hq, hkv
        self.lens = torch.tensor([lens13[r % len(lens13)] for r in range(AT_ROWS)])
        g = torch.Generator().manual_seed(65 + hd + G + cap)
        pq, pdq = pool
        self.q = torch.randn(AT_ROWS, hq * hd, generator=g).to(bf)

        def draw():
            idx = torch.randint(0, pq.numel(), (AT_ROWS, cap, 2, hkv, hd), generator=g)
            return pq[idx], pdq[idx]
        self.codes, self.kv = draw()
        self.codes2, self.kv2 = draw()
        tt = torch.arange(cap)
        past = tt[None, :] >= self.lens[:, None]                                  # [rows][cap]
        k, v = self.kv[:, :, 0].permute(0, 2, 1, 3), self.kv[:, :, 1].permute(0, 2, 1, 3)
        self.ref = attention_reference(self.q.view(AT_ROWS, hq, 1, hd), k, v, 1.0 / hd ** 0.5, ~past[:, None, :])
        # large finite garbage past each row's length, different in the two caches
        bits(self.kv)[past] = torch.where(torch.arange(hd) % 2 == 0, 0x7F7F, -129).to(torch.int16)          # +-3.39e38
        self.codes[past] = torch.where(torch.arange(hd) % 3 == 0, 0x7E, 0xFE).to(torch.uint8)               # +-448
        self.dev = {k: getattr(self, k).to(DEV).contiguous() for k in ("q", "kv", "codes", "kv2", "codes2")}
        self.lengths = (self.lens - 1).to(torch.int32).to(DEV)

    def run(self, eng, rows, r0, kv="kv", codes=None):
        out = torch.full((rows + 2, self.hq * self.hd), KV_CANARY, dtype=bf, device=DEV)
        eng.call("zn_op_bind_kv_fp8", None if codes is None else self.dev[codes][r0:].data_ptr())
        try:
            for _ in range(2):                                 # twice: the split pass's tickets must be back at zero
                out[1:-1].fill_(float("nan"))
                eng.call("zn_op_attn_decode", self.dev["q"][r0:].data_ptr(), self.dev[kv][r0:].data_ptr(), self.cap, self.lengths[r0:].data_ptr(), None,
                         out[1:-1].data_ptr(), rows, _lib.stream_ptr())
            torch.cuda.synchronize()
        finally:
            eng.call("zn_op_bind_kv_fp8", None)
        assert bool((out[0] == KV_CANARY).all()) and bool((out[-1] == KV_CANARY).all())
        return out[1:-1].cpu()

    def sub_ref(self, rows, r0):
        return self.ref._replace(**{f: getattr(self.ref, f)[r0:r0 + rows] for f in self.ref._fields})


@pytest.fixture(scope="module")
def attn_pool():
    return _pool()


@pytest.mark.parametrize("hd,G", list(T.AT_GEOM))
def test_fp8_attention_equals_bf16_attention_on_the_dequantised_cache(attn_pool, hd, G):
    hq, hkv = T.AT_GEOM[(hd, G)]
    model, _ = build_model(dict(d_model=hq * hd, n_layer=1, num_heads=hq, num_heads_kv=hkv, d_ff=256), 31, DEV)
    eng = HipEngine(model.backbone, max_rows=AT_ROWS)
    launches = 0
    # (capacity, ZN_TUNE_ATTN_FUSED_MAX_KEYS): one block fused; the split shape at short contexts; scores + blocks with a second and a third key block
    for cap, lens13, fused_max in ((512, LENS_512, 512), (512, LENS_512, 1), (1032, LENS_1032, 512)):
        ops = AttnOperands(hd, G, cap, lens13, attn_pool)
        eng.call("zn_debug_tune", _lib.ZN_TUNE_ATTN_FUSED_MAX_KEYS, fused_max)
        try:
            for split_cols in (1, 2):
                eng.call("zn_debug_tune", _lib.ZN_TUNE_ATTN_SPLIT_COLS, split_cols)
                for rows, r0 in WINDOWS:
                    label = f"d{hd}g{G} cap{cap} fused_max={fused_max} split_cols={split_cols} rows {rows}+{r0}"
                    got8 = ops.run(eng, rows, r0, codes="codes")
                    got16 = ops.run(eng, rows, r0)
                    assert bool(torch.isfinite(got8.float()).all()), label
                    assert torch.equal(bits(got8), bits(got16)), f"{label}: the FP8 form differs from the bf16 form on the dequantised cache"
                    res = attention_compare(got8.view(rows, hq, 1, hd), ops.sub_ref(rows, r0), label, quiet=True)
                    assert res.ok and res.outside == 0 and res.nonfinite == 0, res.line(label)
                    launches += 1
                    if (rows, r0) == (16, 0):
                        # negative control: other codes under the same bf16 cache - the FP8 form follows the codes, ZN_TUNE_KV_FP8 = 2 the bf16 cache
                        other = ops.run(eng, rows, r0, kv="kv2")
                        assert not torch.equal(bits(other), bits(got16))
                        assert torch.equal(bits(ops.run(eng, rows, r0, kv="kv", codes="codes2")), bits(other)), f"{label}: the FP8 form did not read the codes"
                        eng.call("zn_debug_tune", _lib.ZN_TUNE_KV_FP8, 2)
                        try:
                            assert torch.equal(bits(ops.run(eng, rows, r0, kv="kv", codes="codes2")), bits(got16)), f"{label}: ZN_TUNE_KV_FP8 = 2 must read the bf16 cache"
                        finally:
                            eng.call("zn_debug_tune", _lib.ZN_TUNE_KV_FP8, 1)
        finally:
            eng.call("zn_debug_tune", _lib.ZN_TUNE_ATTN_FUSED_MAX_KEYS, 512)
            eng.call("zn_debug_tune", _lib.ZN_TUNE_ATTN_SPLIT_COLS, 3)
        for k in ("q", "kv", "codes"):
            assert torch.equal(ops.dev[k].cpu().view(torch.uint8), getattr(ops, k).contiguous().view(torch.uint8)), f"d{hd}g{G} cap{cap}: {k} was written"
    assert launches == 36
    print(f"[kv fp8 attention d{hd}g{G}] {launches} launch settings: FP8 form == bf16 form, inside the float64 interval")


def test_fewer_than_five_rows_read_the_bf16_cache(attn_pool):
    """The per-op entry follows the plan: at 4 rows the bound codes are ignored (here they differ from the cache, so reading them would show)."""
    model, _ = build_model(dict(d_model=8 * 128, n_layer=1, num_heads=8, num_heads_kv=2, d_ff=256), 31, DEV)
    eng = HipEngine(model.backbone, max_rows=AT_ROWS)
    ops = AttnOperands(128, 4, 512, LENS_512, attn_pool)
    assert torch.equal(bits(ops.run(eng, 4, 0, kv="kv", codes="codes2")), bits(ops.run(eng, 4, 0)))
    assert not torch.equal(bits(ops.run(eng, 5, 0, kv="kv", codes="codes2")), bits(ops.run(eng, 5, 0)))


# ---------------------------------------------------------------------------------------------- 3. end to end
NQB = 9


@pytest.fixture(scope="module")
def tiny():
    """A: the mode on.  B: the same weights, the mode off."""
    dac = DACAutoencoder(synth.dac_state_dict(4321, encoder=False), device=DEV)
    A, _ = build_model(synth.TINY_CFG, 77, DEV, dac=dac, peaky=True)
    B, _ = build_model(synth.TINY_CFG, 77, DEV, dac=dac, peaky=True)
    assert A.kv_cache == "bf16" and A.set_kv_cache("fp8").kv_cache == "fp8" and B.kv_cache == "bf16"
    A.engine(16)                                   # one engine for every call below (a tune key lives on the engine)
    return A, B


class reads_bf16:
    """ZN_TUNE_KV_FP8 = 2 on the model's engine for the length of the block."""

    def __init__(self, model):
        self.eng = model.engine(16)

    def __enter__(self):
        self.eng.call("zn_debug_tune", _lib.ZN_TUNE_KV_FP8, 2)

    def __exit__(self, *a):
        self.eng.call("zn_debug_tune", _lib.ZN_TUNE_KV_FP8, 1)


def _cond(i, L, halves=2):
    return synth.conditioning(500 + i, "kv8.e2e", halves, L, synth.TINY_CFG["d_model"]).to(DEV)


def _generate(model, batch, steps=12):
    cond = torch.cat([_cond(i, 6) for i in range(batch)], 0)
    cond = torch.cat([cond[0::2], cond[1::2]], 0)
    tr = {"logits": []}
    eng = model.engine(16)
    eng.call("zn_debug_eos_bias", float("-inf"))
    try:
        out = model.generate(cond, max_new_tokens=steps, cfg_scale=2.0, batch_size=batch, sampling_params=dict(temperature=0.0), _trace=tr)
    finally:
        eng.call("zn_debug_eos_bias", 0.0)
    torch.cuda.synchronize()
    return [out.cpu()], [l.cpu() for l in tr["logits"]]


def _same_run(a, b, what, differ=False):
    assert len(a[0]) == len(b[0]) and len(a[1]) == len(b[1]) >= 8, what
    codes = [i for i, (x, y) in enumerate(zip(a[0], b[0])) if not torch.equal(x, y)]
    logits = [i for i, (x, y) in enumerate(zip(a[1], b[1])) if x.shape != y.shape or not torch.equal(x.view(torch.int32), y.view(torch.int32))]
    if differ:
        assert logits, f"{what}: every per-step logit is equal"
    else:
        assert not codes and not logits, f"{what}: codes of results {codes} and logits of records {logits} differ"


@pytest.mark.parametrize("batch", [3, 9])
def test_generate_equals_the_bf16_reads_of_the_same_rounded_cache(tiny, batch):
    A, B = tiny
    assert A.kv_fp8_plan(2 * batch) == {"rounded": True, "attention_reads": "fp8"}
    on = _generate(A, batch)
    with reads_bf16(A):
        assert A.kv_fp8_plan(2 * batch) == {"rounded": True, "attention_reads": "bf16"}
        off = _generate(A, batch)
    _same_run(on, off, f"generate(batch_size={batch})")
    _same_run(on, _generate(B, batch), f"generate(batch_size={batch}) against the mode-off model: the rounding must show", differ=True)


@pytest.mark.parametrize("batch", [1, 2])
def test_the_mode_is_inert_below_five_rows(tiny, batch):
    A, B = tiny
    assert A.kv_fp8_plan(2 * batch) == {"rounded": False, "attention_reads": "bf16"}
    _same_run(_generate(A, batch), _generate(B, batch), f"generate(batch_size={batch})")


def _batch(model, ragged, mixed):
    reqs = []
    for i in range(6):
        guided = not (mixed and i % 2)
        pre = torch.from_numpy(synth.randint(66, f"kv8.prefix.{i}", (1, NQB, (0, 3, 1, 4, 2, 0)[i]), 1024)).to(DEV) if ragged and (0, 3, 1, 4, 2, 0)[i] else None
        reqs.append(GenRequest(_cond(20 + i, 4 + i % 3, 2 if guided else 1), sampling_params=dict(temperature=0.0), cfg_scale=(2.0, 1.5, 3.0)[i % 3] if guided else 1.0,
                               max_new_tokens=8 + i % 4, audio_prefix_codes=pre))
    tr = {"logits": []}
    out = model.generate_batch(reqs, ragged_prefix=ragged, mixed_guidance=mixed, _trace=tr)
    torch.cuda.synchronize()
    return [o.cpu() for o in out], [l.cpu() for l in tr["logits"]]


@pytest.mark.parametrize("ragged,mixed", [(True, False), (False, True)])
def test_generate_batch_ragged_prefixes_and_mixed_guidance(tiny, ragged, mixed):
    A, _ = tiny
    on = _batch(A, ragged, mixed)
    with reads_bf16(A):
        off = _batch(A, ragged, mixed)
    _same_run(on, off, f"generate_batch(ragged_prefix={ragged}, mixed_guidance={mixed})")


def _requests(n):
    return [GenRequest(_cond(40 + i, 4 + i % 3), sampling_params=dict(temperature=0.0), cfg_scale=(2.0, 1.5, 3.0)[i % 3], max_new_tokens=6 + i % 4) for i in range(n)]


def test_serve_session_in_which_requests_join_late(tiny):
    A, _ = tiny

    def session():
        src = _requests(5) + [None, None] + _requests(12)[5:]                  # 12 requests for 8 slots; some arrive while the session runs
        tr = {}
        out = {r.index: r for r in A.serve(iter(src), slots=8, max_prompt=8, max_new_tokens=10, guided=True, sched_every=4, _trace=tr)}
        assert sorted(out) == list(range(12)) and all(r.error is None for r in out.values())
        assert any(kind == "admit" and step > 0 for kind, step, _ in tr["slots"]), "no request joined the running session"
        # (the logits of a slot nobody holds are workspace: they follow what the engine ran before the session)
        held = [[b for b, who in enumerate(holders) if who is not None] for _, _, holders in tr["slots"]]
        return [out[i].codes.cpu() for i in range(12)], [l.cpu()[rows] for l, rows in zip(tr["logits"], held)], tr["slots"]
    on = session()
    with reads_bf16(A):
        off = session()
    assert on[2] == off[2], "the two sessions must schedule alike"
    _same_run(on, off, "serve(slots=8)")


def test_serve_stream(tiny):
    A, _ = tiny

    def session():
        codes, wavs = {}, {}
        for ch in A.serve_stream(iter(_requests(10)), slots=8, max_prompt=8, max_new_tokens=10, guided=True, sched_every=4, chunk_frames=4):
            assert ch.error is None
            codes.setdefault(ch.index, []).append(ch.codes.cpu())
            wavs.setdefault(ch.index, []).append(ch.wav.cpu())
        return [torch.cat(codes[i], 2) for i in range(10)], [torch.cat(wavs[i], 2) for i in range(10)]
    on = session()
    with reads_bf16(A):
        off = session()
    assert all(torch.equal(x, y) for x, y in zip(on[0], off[0])), "serve_stream: codes differ"
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(on[1], off[1])), "serve_stream: samples differ"


def test_state_refusals_and_the_unbound_generation(tiny):
    A, _ = tiny
    eng = A.engine(16)
    out = (C.c_int32 * 2)()
    eng.call("zn_kv_fp8_plan", 16, out)
    assert list(out) == [1, 1]
    gen = A.serve(iter(_requests(2)), slots=4, max_prompt=8, max_new_tokens=10, guided=True)
    next(gen)
    with torch.cuda.device(eng.device):
        rc = eng.lib.zn_set_kv_fp8(eng.h, 0)
    assert rc == -3 and "inside a generation" in eng.lib.zn_last_error(eng.h).decode()
    gen.close()
    eng.call("zn_set_kv_fp8", 0)
    eng.call("zn_kv_fp8_plan", 16, out)
    assert list(out) == [0, 0]
    eng.call("zn_set_kv_fp8", 1)
    # a generation in which the mode is in effect and no code caches are bound is an error, not a bf16 generation
    ip = A.setup_cache(batch_size=6, max_seqlen=32)
    delayed = torch.full((3, NQB, 20), -1, dtype=torch.int32, device=DEV)
    kv_ptrs = (C.c_void_p * 2)(*[ip.key_value_memory_dict[i][0].data_ptr() for i in range(2)])
    sp = _lib.zn_sampling()
    eng.call("zn_gen_begin", 3, kv_ptrs, 32, ip.lengths_per_sample.data_ptr(), delayed.data_ptr(), 20, 1, 8, 2.0, C.byref(sp), _lib.stream_ptr())
    hidden = torch.zeros(6, 4, synth.TINY_CFG["d_model"], dtype=bf, device=DEV)
    with torch.cuda.device(eng.device):
        rc = eng.lib.zn_prefill(eng.h, hidden.data_ptr(), 4, _lib.stream_ptr())
    assert rc == -3 and "zn_gen_bind_kv_fp8" in eng.lib.zn_last_error(eng.h).decode()
    eng.call("zn_gen_end")
    model, _ = build_model(synth.HYBRID_TINY_CFG, 23, DEV)
    heng = model.engine(4)
    with torch.cuda.device(heng.device):
        assert heng.lib.zn_set_kv_fp8(heng.h, 1) == -4 and "hybrid" in heng.lib.zn_last_error(heng.h).decode()


def test_with_the_fp8_mlp_stream():
    """Both FP8 modes on one model at full width: the same equality."""
    A, _ = build_model(dict(d_model=2048, n_layer=2, num_heads=16, num_heads_kv=4, d_ff=8192), 53, DEV)
    A.quantize_mlp_fp8()
    A.set_kv_cache("fp8")
    eng = A.engine(16)
    assert eng.mlp_fp8_plan(8) == [1, 1] and A.kv_fp8_plan(8)["attention_reads"] == "fp8"

    def run():
        cond = torch.cat([synth.conditioning(700 + i, "kv8.mlp", 2, 6, 2048) for i in range(4)], 0)
        cond = torch.cat([cond[0::2], cond[1::2]], 0).to(DEV)
        tr = {"logits": []}
        eng.call("zn_debug_eos_bias", float("-inf"))
        try:
            out = A.generate(cond, max_new_tokens=10, cfg_scale=2.0, batch_size=4, sampling_params=dict(temperature=0.0), _trace=tr)
        finally:
            eng.call("zn_debug_eos_bias", 0.0)
        torch.cuda.synchronize()
        return [out.cpu()], [l.cpu() for l in tr["logits"]]
    on = run()
    eng.call("zn_debug_tune", _lib.ZN_TUNE_KV_FP8, 2)
    try:
        off = run()
    finally:
        eng.call("zn_debug_tune", _lib.ZN_TUNE_KV_FP8, 1)
    _same_run(on, off, "quantize_mlp_fp8() + kv_cache='fp8'")
