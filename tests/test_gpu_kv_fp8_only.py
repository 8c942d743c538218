"""The codes-only FP8 KV cache (Zonos.set_kv_cache("fp8-only"), zn_set_kv_fp8_only) on the device, bit for bit against the
two-cache mode "fp8" (tests/test_gpu_kv_fp8.py):
  1. the prefill attention per op: zn_op_attn_prefill_rows_fp8 on the codes equals zn_op_attn_prefill_rows on the dequantised bf16 cache in every
     bit for every case of zonos_amd.testing.attention_cases_prefill() (both kernels, every head size and group, every dispatch edge), lies inside
     the float64 interval on the dequantised operands, does not depend on the code bytes at or past a row's context (0x00, random, 0x7F, 0xFF,
     0x7E), leaves its inputs and the canaries alone, and reads the codes (a negative control);
  2. the appends per op with no bf16 cache: the decode epilogues at 5, 16, 17 and 64 rows (groups and the wide plan), the prefill epilogue and
     rope_kv_rows_kernel write the codes of the two-cache append (kv_round_e4m3) and nothing else, q bit-equal, nothing at position max_len;
  3. the decode attention per op with kv_dev NULL at 5 and 64 rows, contexts 1 and 513;
  4. end to end on a tiny transformer: codes and per-step logits of an "fp8-only" model equal the same model in "fp8" through generate(),
     generate_batch(), serve() and serve_stream(), also with quantize_mlp_fp8(); no bf16 KV tensor is allocated, zn_gen_begin receives NULL, and
     bf16 buffers passed anyway stay untouched;
  5. the refusals."""
import ctypes as C

import pytest
import torch

from zonos_amd import _lib, synth
from zonos_amd import quant as Q
from zonos_amd import testing as T
from zonos_amd.autoencoder import DACAutoencoder
from zonos_amd.backbone import HipEngine
from zonos_amd.model import GenRequest, _sampling_struct
from zonos_amd.rows import code_rows
from zonos_amd.serving import serve_slack
from zonos_amd.testing import LF_PRO_LN, LF_PRO_NONE, LF_ROPE_KV, attention_compare, attention_reference, build_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
bf = torch.bfloat16
PAD = 4096                       # guard elements in front of and behind each buffer
KV_CANARY, CODE_CANARY = 768.0, 0xA5
CODE_TAILS = ("0x00", "random", "0x7F", "0xFF", "0x7E")      # what the code bytes at or past a row's context hold, in turn


def bits(t):
    return t.view(torch.int16)


class Guarded:
    """[PAD canary elements | the tensor | PAD canary elements] in one allocation."""

    def __init__(self, shape, dtype=bf):
        n = 1
        for s in shape:
            n *= int(s)
        self.canary = KV_CANARY if dtype == bf else CODE_CANARY
        self.buf = torch.full((n + 2 * PAD,), self.canary, dtype=dtype, device=DEV)
        self.view = self.buf[PAD:PAD + n].view(*shape)

    def ptr(self):
        return self.view.data_ptr()

    def check(self, label):
        assert bool((self.buf[:PAD] == self.canary).all()) and bool((self.buf[-PAD:] == self.canary).all()), f"{label}: a canary was overwritten"


# ---------------------------------------------------------------------------------------------- 1. the prefill attention on codes
TUNE_DEFAULT = {"ZN_TUNE_PREFILL_ATTN_VALU": 1}


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(hd, G):
        if (hd, G) not in cache:
            hq, hkv = T.AT_GEOM[(hd, G)]
            model, _ = build_model(dict(d_model=hq * hd, n_layer=1, num_heads=hq, num_heads_kv=hkv, d_ff=256), 31, DEV)
            cache[(hd, G)] = HipEngine(model.backbone, max_rows=16)
            cache[(hd, G)]._model = model
        return cache[(hd, G)]
    return get


def run_prefill_case(eng, c):
    st = _lib.stream_ptr()
    t = T.attention_case_tensors(c)
    (kq, kdq), (vq, vdq) = Q.kv_round_e4m3(t["k"]), Q.kv_round_e4m3(t["v"])
    assert float(torch.maximum(kdq.float().abs().max(), vdq.float().abs().max())) < 448.0
    ref = attention_reference(t["q"], kdq, vdq, t["scale"], t["visible"])
    q0, kv0 = (x.to(DEV) for x in T.attention_device_layout(c, dict(q=t["q"], k=kdq, v=vdq)))
    _, codes0 = T.attention_device_layout(c, dict(q=t["q"], k=kq, v=vq))
    codes0 = codes0.to(DEV)
    start = [int(s) for s in t["start"]]
    q, kv, codes, out = Guarded(q0.shape), Guarded(kv0.shape), Guarded(codes0.shape, torch.uint8), Guarded(q0.shape)
    row_len = torch.tensor(c.lens, dtype=torch.int32, device=DEV) if c.ragged else None
    rl = None if row_len is None else row_len.data_ptr()
    cmp = ref.valid[:, None, :, None].expand_as(ref.lo)

    def launch(fp8):
        out.view.fill_(KV_CANARY)
        if fp8:
            eng.call("zn_op_attn_prefill_rows_fp8", q.ptr(), codes.ptr(), c.cap, out.ptr(), c.S, c.R, c.base, rl, st)
        else:
            eng.call("zn_op_attn_prefill_rows", q.ptr(), kv.ptr(), c.cap, out.ptr(), c.S, c.R, c.base, rl, st)
        torch.cuda.synchronize()
        for g in (q, kv, codes, out):
            g.check(c.name)
        return T.attention_from_device_layout(c, out.view)
    headroom = 0.0
    try:
        for key, val in c.tune:
            eng.call("zn_debug_tune", getattr(_lib, key), val)
        q.view.copy_(q0)
        kv.view.copy_(kv0)
        want = launch(False)                               # the bf16 form on the dequantised cache
        for tail in CODE_TAILS:
            codes.view.copy_(codes0)
            for r in range(c.R):
                if tail == "random":
                    g = torch.Generator().manual_seed(4100 + r)
                    codes.view[r, start[r]:] = torch.randint(0, 256, tuple(codes.view[r, start[r]:].shape), generator=g, dtype=torch.uint8).to(DEV)
                else:
                    codes.view[r, start[r]:] = int(tail, 16)
            q_in, codes_in = q.view.clone(), codes.view.clone()
            label = f"{c.name} code tail {tail}"
            got = launch(True)
            assert torch.equal(bits(q.view), bits(q_in)) and torch.equal(codes.view, codes_in), f"{label}: an input was written"
            if not bool(cmp.all()):                        # positions at or past row_len[r] keep the canary
                assert bool((got.float()[~cmp] == KV_CANARY).all()), f"{label}: a position at or past row_len was written"
            assert torch.equal(bits(got)[cmp], bits(want)[cmp]), f"{label} ({c.kernel}): the FP8 form differs from the bf16 form on the dequantised cache"
            res = attention_compare(got, ref, label, quiet=True)
            assert res.ok and res.outside == 0 and res.nonfinite == 0, (label, c.kernel, res.line(label))
            headroom = max(headroom, res.headroom)
        # negative control: query 0 of row 0 sees key `base` with a weight that shows (its only key, or its spotlight); its V codes decide the output,
        # the codes of the first key past the row's context do not
        codes.view.copy_(codes0)
        codes.view[0, start[0]] ^= 0x55
        assert torch.equal(bits(launch(True))[cmp], bits(want)[cmp]), f"{c.name}: a code past the row's context changed the output"
        codes.view.copy_(codes0)
        codes.view[0, c.base, 1] ^= 0x80                   # the sign of every V element of the key
        assert not torch.equal(bits(launch(True))[0, :, 0], bits(want)[0, :, 0]), f"{c.name}: the output does not follow the codes of a visible key"
    finally:
        for key, _ in c.tune:
            eng.call("zn_debug_tune", getattr(_lib, key), TUNE_DEFAULT[key])
    print(f"[prefill attention on codes {c.name}] {c.kernel}: == the bf16 form on the dequantised cache over {len(CODE_TAILS)} code tails, inside the float64 interval "
          f"(worst |got - exact| / (Theta A) {headroom:.3f})")


@pytest.mark.parametrize("kern,hd,G", [("mfma", 128, 1), ("mfma", 128, 2), ("mfma", 128, 4), ("mfma", 128, 8), ("valu", 128, 1), ("valu", 128, 2), ("valu", 128, 4),
                                       ("valu", 128, 8), ("valu", 64, 4), ("valu", 64, 2), ("valu", 32, 4), ("valu", 32, 8)])
def test_prefill_attention_on_codes_every_kernel(engines, kern, hd, G):
    cases = [c for c in T.attention_cases_prefill() if (c.hd, c.G) == (hd, G) and f" {kern} " in c.name]
    assert len(cases) >= 5 and all((kern == "mfma") == ("mfma" in c.kernel) for c in cases)
    for c in cases:
        run_prefill_case(engines(hd, G), c)


def test_prefill_fp8_entry_validates_before_launching(engines):
    eng = engines(128, 4)
    hq, hkv = T.AT_GEOM[(128, 4)]
    S, cap = 8, 16
    q, out = Guarded((2, S, hq * 128)), Guarded((2, S, hq * 128))
    codes = torch.zeros(2, cap, 2, hkv, 128, dtype=torch.uint8, device=DEV)
    st = _lib.stream_ptr()

    def call(qp, cp, outp, S_, rows, base):
        with torch.cuda.device(eng.device):
            return eng.lib.zn_op_attn_prefill_rows_fp8(eng.h, qp, cp, cap, outp, S_, rows, base, None, st)
    assert call(q.ptr(), codes.data_ptr(), out.ptr(), S, 2, -1) == -1
    assert call(q.ptr(), codes.data_ptr(), out.ptr(), S, 2, cap - S + 1) == -1 and "positions" in eng.lib.zn_last_error(eng.h).decode()
    assert call(None, codes.data_ptr(), out.ptr(), S, 2, 0) == -1 and call(q.ptr(), None, out.ptr(), S, 2, 0) == -1 and call(q.ptr(), codes.data_ptr(), None, S, 2, 0) == -1
    assert call(q.ptr(), codes.data_ptr(), out.ptr(), S, 18, 0) == -1 and "max_rows" in eng.lib.zn_last_error(eng.h).decode()
    torch.cuda.synchronize()
    assert bool((out.buf == KV_CANARY).all()), "a refused call launched something"
    assert call(q.ptr(), codes.data_ptr(), out.ptr(), S, 2, cap - S) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 2. the appends with no bf16 cache
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


class Caches:
    """A bf16 cache [rows][max_len][2][NK] of seeded finite values and a code cache full of canary bytes, each between guards."""

    def __init__(self, rows, max_len, tag):
        self.shape = (rows, max_len, 2, NK)
        self.kv0 = torch.from_numpy(synth.normal(62, f"kv8only.cache.{tag}.{rows}.{max_len}", self.shape)).to(bf).to(DEV)
        self.kv, self.codes = Guarded(self.shape), Guarded(self.shape, torch.uint8)
        self.reset()

    def reset(self):
        self.kv.view.copy_(self.kv0)
        self.codes.view.fill_(CODE_CANARY)

    def check(self, label):
        self.kv.check(label)
        self.codes.check(label)


def run_linear(eng, w, cache, pro, rows, x, mode, lengths=None, prefill=0, pf_S=0, pf_base=0, out=None):
    """mode: "off" (no code cache bound), "both" (the two-cache append), "codes" (codes bound, the bf16 cache NULL)."""
    st = _lib.stream_ptr()
    q_out = torch.full((rows, NQ), float("nan"), dtype=bf, device=DEV)
    op = _lib.zn_linear_op(pro=pro, epi=LF_ROPE_KV, rows=rows, N=NQKV, K=KIN, prefill=prefill, target_blocks=4, max_len=cache.shape[1], pf_S=pf_S, pf_base=pf_base)
    op.x, op.W, op.q_out = x.data_ptr(), w["W"].data_ptr(), q_out.data_ptr()
    op.kv = None if mode == "codes" else cache.kv.ptr()
    if pro == LF_PRO_LN:
        op.ln_w, op.ln_b = w["ln_w"].data_ptr(), w["ln_b"].data_ptr()
    if lengths is not None:
        op.lengths = lengths.data_ptr()
    if out is not None:
        op.out = out.data_ptr()
    eng.call("zn_op_bind_kv_fp8", None if mode == "off" else cache.codes.ptr())
    try:
        eng.call("zn_op_linear_fused", C.byref(op), st)
        torch.cuda.synchronize()
    finally:
        eng.call("zn_op_bind_kv_fp8", None)
    assert op.plan_dict()["err"] == 0
    return q_out.cpu(), op.plan_dict()


def _x(rows, tag):
    scale = torch.linspace(0.5, 3.0, rows)[:, None]
    return (torch.from_numpy(synth.normal(63, f"kv8only.x.{tag}.{rows}", (rows, KIN))) * scale).to(bf).to(DEV)


def check_codes_only(cache, kv_off, codes_both, codes_only, cr, pos, label, meets_capacity=True):
    """kv_off: the bf16 cache after the op with no code cache (CPU); codes_both / codes_only: the code cache after the two-cache and the codes-only append."""
    fits = pos < cache.shape[1]
    assert bool(fits.any()) and (not meets_capacity or bool((~fits).any())), f"{label}: the case must append somewhere and meet the capacity somewhere"
    touched = torch.zeros(cache.shape[:2], dtype=torch.bool)
    touched[cr[fits], pos[fits]] = True
    app = kv_off[touched]
    assert bool(torch.isfinite(app.float()).all()) and float(app.float().abs().max()) > 448 and float(app.float().abs()[app != 0].min()) < 2.0 ** -9, label
    q, _ = Q.kv_round_e4m3(app)
    assert torch.equal(codes_both[touched], q), f"{label}: the two-cache append does not write kv_round_e4m3's codes"
    assert torch.equal(codes_only[touched], q), f"{label}: the codes-only append does not write the codes of the two-cache append"
    assert bool((codes_only[~touched] == CODE_CANARY).all()), f"{label}: codes were written at a position that was not appended (position max_len included)"
    assert torch.equal(bits(cache.kv.view), bits(cache.kv0)), f"{label}: the codes-only append wrote the bf16 cache it was not given"
    cache.check(label)


@pytest.mark.parametrize("rows,wide", [(5, 0), (16, 0), (17, 0), (17, 1), (64, 0), (64, 1)])
def test_decode_append_writes_the_codes_alone(lin_engines, lin_weights, rows, wide):
    """gemv_epilogue<EPI_ROPE_KV> with GemvArgs::kv == NULL as the 5..64-row projection kernels use it: groups of 16 rows (17 = 16 + a one-row GEMV
    launch), and up to 64 rows per weight pass (ZN_TUNE_WIDE_ROWS = 2), with and without the LayerNorm prologue, at both head sizes."""
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
                cache, x, ld = Caches(rows + 1, L, "d"), _x(rows, "d"), lens.to(torch.int32).to(DEV)
                q_off, plan = run_linear(eng, lin_weights, cache, pro, rows, x, "off", lengths=ld)
                kv_off = cache.kv.view.cpu()
                cache.reset()
                q_both, _ = run_linear(eng, lin_weights, cache, pro, rows, x, "both", lengths=ld)
                codes_both = cache.codes.view.cpu()
                cache.reset()
                q_only, plan_only = run_linear(eng, lin_weights, cache, pro, rows, x, "codes", lengths=ld)
                assert plan_only == plan and (rows <= 16 or plan["rows_per_launch"] == (64 if wide else 16)), (label, plan)
                assert bool(torch.isfinite(q_off.float()).all()) and torch.equal(bits(q_only), bits(q_off)) and torch.equal(bits(q_both), bits(q_off)), f"{label}: q must not change"
                check_codes_only(cache, kv_off, codes_both, cache.codes.view.cpu(), cr, lens, label)
        finally:
            if wide:
                eng.call("zn_debug_tune", _lib.ZN_TUNE_WIDE_ROWS, 1)


@pytest.mark.parametrize("rows,S,base", [(34, 17, 3), (64, 32, 0)])
def test_prefill_append_in_the_epilogue_and_in_rope_kv_rows_writes_the_codes_alone(lin_engines, lin_weights, rows, S, base):
    eng, st, R = lin_engines[128], _lib.stream_ptr(), rows // S
    x = _x(rows, "p")
    m = torch.arange(rows)
    cr, pos = m // S, base + m % S
    # 1. in the epilogue (the entry point wants base + S <= max_len: the capacity is met in form 2)
    cache = Caches(R + 1, base + S + 3, "p")
    out = torch.full((rows, NQKV), float("nan"), dtype=bf, device=DEV)
    q_off, plan = run_linear(eng, lin_weights, cache, LF_PRO_NONE, rows, x, "off", prefill=1, pf_S=S, pf_base=base, out=out)
    assert plan["rope_done"] == 1 and plan["kernel"] == "GEMM16K", plan
    kv_off = cache.kv.view.cpu()
    cache.reset()
    run_linear(eng, lin_weights, cache, LF_PRO_NONE, rows, x, "both", prefill=1, pf_S=S, pf_base=base, out=out)
    codes_both = cache.codes.view.cpu()
    cache.reset()
    q_only, _ = run_linear(eng, lin_weights, cache, LF_PRO_NONE, rows, x, "codes", prefill=1, pf_S=S, pf_base=base, out=out)
    assert torch.equal(bits(q_only), bits(q_off))
    check_codes_only(cache, kv_off, codes_both, cache.codes.view.cpu(), cr, pos, "prefill epilogue", meets_capacity=False)
    # 2. projection, then rope_kv_rows_kernel; max_len = base + S - 2: the last two positions of every row write nothing
    eng.call("zn_debug_tune", _lib.ZN_TUNE_NO_PREFILL_GEMM16K, 2)
    try:
        _, plan = run_linear(eng, lin_weights, Caches(R + 1, base + S + 3, "p2"), LF_PRO_NONE, rows, x, "both", prefill=1, pf_S=S, pf_base=base, out=out)
    finally:
        eng.call("zn_debug_tune", _lib.ZN_TUNE_NO_PREFILL_GEMM16K, 1)
    assert plan["rope_done"] == 0 and bool(torch.isfinite(out.float()).all()), plan
    max_len = base + S - 2
    cache = Caches(R + 1, max_len, "p3")
    qkv = {k: out.clone() for k in ("off", "both", "codes")}
    codes_seen = {}
    for mode in ("off", "both", "codes"):
        cache.reset()
        eng.call("zn_op_bind_kv_fp8", None if mode == "off" else cache.codes.ptr())
        try:
            eng.call("zn_op_rope_kv_rows", qkv[mode].data_ptr(), None if mode == "codes" else cache.kv.ptr(), max_len, S, base, R, st)
            torch.cuda.synchronize()
        finally:
            eng.call("zn_op_bind_kv_fp8", None)
        if mode == "off":
            kv_off = cache.kv.view.cpu()
        codes_seen[mode] = cache.codes.view.cpu()
    assert torch.equal(bits(qkv["codes"]), bits(qkv["off"])) and not torch.equal(bits(qkv["codes"][:, :NQ]), bits(out[:, :NQ])), "q is rotated in place, the same in every mode"
    check_codes_only(cache, kv_off, codes_seen["both"], codes_seen["codes"], cr, pos, "rope_kv_rows")
    # without a bound code cache a NULL cache stays the error it is
    with torch.cuda.device(eng.device):
        assert eng.lib.zn_op_rope_kv_rows(eng.h, qkv["off"].data_ptr(), None, max_len, S, base, R, st) == -1
    op = _lib.zn_linear_op(pro=LF_PRO_NONE, epi=LF_ROPE_KV, rows=5, N=NQKV, K=KIN, prefill=0, target_blocks=4, max_len=16)
    q_out, ld = torch.zeros(5, NQ, dtype=bf, device=DEV), torch.zeros(5, dtype=torch.int32, device=DEV)
    op.x, op.W, op.q_out, op.lengths, op.kv = x.data_ptr(), lin_weights["W"].data_ptr(), q_out.data_ptr(), ld.data_ptr(), None
    with torch.cuda.device(eng.device):
        assert eng.lib.zn_op_linear_fused(eng.h, C.byref(op), st) == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- 3. the decode attention with no bf16 cache
def test_decode_attention_with_a_null_bf16_cache():
    hq, hkv, hd, cap = 8, 2, 128, 520
    model, _ = build_model(dict(d_model=hq * hd, n_layer=1, num_heads=hq, num_heads_kv=hkv, d_ff=256), 31, DEV)
    eng = HipEngine(model.backbone, max_rows=64)
    st = _lib.stream_ptr()
    g = torch.Generator().manual_seed(77)
    pq, pdq = Q.kv_round_e4m3(torch.from_numpy(synth.normal(64, "kv8only.pool", (1 << 14,))).to(bf))
    idx = torch.randint(0, pq.numel(), (64, cap, 2, hkv, hd), generator=g)
    codes, kv = pq[idx].to(DEV).contiguous(), pdq[idx].to(DEV).contiguous()
    q = torch.randn(64, hq * hd, generator=g).to(bf).to(DEV)
    lens = torch.tensor([(1, 513)[r % 2] for r in range(64)])
    lengths = (lens - 1).to(torch.int32).to(DEV)

    def run(rows, kv_ptr, bound=True):
        out = Guarded((rows, hq * hd))
        eng.call("zn_op_bind_kv_fp8", codes.data_ptr() if bound else None)
        try:
            with torch.cuda.device(eng.device):
                rc = eng.lib.zn_op_attn_decode(eng.h, q.data_ptr(), kv_ptr, cap, lengths.data_ptr(), None, out.ptr(), rows, st)
            torch.cuda.synchronize()
        finally:
            eng.call("zn_op_bind_kv_fp8", None)
        out.check(f"decode attention rows {rows}")
        return rc, out.view.cpu()
    for rows in (5, 64):
        rc2, both = run(rows, kv.data_ptr())
        rc1, only = run(rows, None)
        assert rc1 == 0 and rc2 == 0 and bool(torch.isfinite(only.float()).all())
        assert torch.equal(bits(only), bits(both)), f"rows {rows}: the call without a bf16 cache differs from the call with both caches"
    # a NULL cache is legal only where a bound code cache is what the launch reads
    rc, out = run(5, None, bound=False)
    assert rc == -1 and bool((out == KV_CANARY).all())
    rc, out = run(4, None)
    assert rc == -1 and bool((out == KV_CANARY).all()), "at 4 rows the codes are not read"
    eng.call("zn_debug_tune", _lib.ZN_TUNE_KV_FP8, 2)
    try:
        rc, out = run(5, None)
    finally:
        eng.call("zn_debug_tune", _lib.ZN_TUNE_KV_FP8, 1)
    assert rc == -1 and bool((out == KV_CANARY).all()), "ZN_TUNE_KV_FP8 = 2 reads the bf16 cache: none given"


# ---------------------------------------------------------------------------------------------- 4. end to end
NQB = 9


class Spy:
    """Records what the one buffer helper (Zonos._kv_buffers) returned and what zn_gen_begin received as its KV pointers."""

    def __init__(self, model):
        self.model, self.eng = model, model.engine(16)
        self.bufs, self.begin = [], []

    def __enter__(self):
        helper, call = self.model._kv_buffers, self.eng.call

        def kv_buffers(*a, **k):
            self.bufs.append(helper(*a, **k))
            return self.bufs[-1]

        def spy_call(name, *args):
            if name == "zn_gen_begin":
                self.begin.append(args[1])
            return call(name, *args)
        self.model._kv_buffers, self.eng.call = kv_buffers, spy_call
        return self

    def __exit__(self, *a):
        del self.model._kv_buffers, self.eng.call

    def assert_codes_only(self, n, what):
        assert len(self.bufs) == n and len(self.begin) == n, (what, len(self.bufs), len(self.begin))
        for b in self.bufs:
            assert b.kv_ptrs is None and b.ip.key_value_memory_dict == {} and b.codes is not None and all(t.dtype == torch.uint8 for t in b.codes), f"{what}: a bf16 KV tensor was allocated"
        assert all(p is None for p in self.begin), f"{what}: zn_gen_begin did not receive NULL"


@pytest.fixture(scope="module")
def tiny():
    """A: "fp8-only".  F: the same weights in "fp8" (two caches).  B: the mode off."""
    dac = DACAutoencoder(synth.dac_state_dict(4321, encoder=False), device=DEV)
    A, F, B = (build_model(synth.TINY_CFG, 77, DEV, dac=dac, peaky=True)[0] for _ in range(3))
    assert A.set_kv_cache("fp8-only").kv_cache == "fp8-only" and F.set_kv_cache("fp8").kv_cache == "fp8" and B.kv_cache == "bf16"
    for m in (A, F, B):
        m.engine(16)
    return A, F, B


def _cond(i, L, halves=2):
    return synth.conditioning(500 + i, "kv8.e2e", halves, L, synth.TINY_CFG["d_model"]).to(DEV)


def _generate(model, batch, steps=12, d_model=None, eng_rows=16):
    cond = torch.cat([_cond(i, 6) if d_model is None else synth.conditioning(700 + i, "kv8.mlp", 2, 6, d_model).to(DEV) for i in range(batch)], 0)
    cond = torch.cat([cond[0::2], cond[1::2]], 0)
    tr = {"logits": []}
    eng = model.engine(eng_rows)
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


def test_generate_equals_the_two_cache_mode(tiny):
    A, F, B = tiny
    assert A.kv_cache_plan(6) == {"rounded": True, "attention_reads": "fp8", "bf16_cache": False}
    assert F.kv_cache_plan(6) == {"rounded": True, "attention_reads": "fp8", "bf16_cache": True}
    assert A.kv_fp8_plan(6) == F.kv_fp8_plan(6)
    with Spy(A) as spy:
        only = _generate(A, 3)
    spy.assert_codes_only(1, "generate(batch_size=3)")
    both = _generate(F, 3)
    _same_run(only, both, "generate(batch_size=3), 'fp8-only' against 'fp8'")
    _same_run(only, _generate(B, 3), "generate(batch_size=3) against the mode-off model: the rounding must show", differ=True)
    # ZN_TUNE_KV_FP8 = 2 has no bf16 cache to fall back to: ignored, and the plan says so
    eng = A.engine(16)
    eng.call("zn_debug_tune", _lib.ZN_TUNE_KV_FP8, 2)
    try:
        assert A.kv_cache_plan(6) == {"rounded": True, "attention_reads": "fp8", "bf16_cache": False}
        _same_run(_generate(A, 3), both, "generate(batch_size=3) under ZN_TUNE_KV_FP8 = 2")
    finally:
        eng.call("zn_debug_tune", _lib.ZN_TUNE_KV_FP8, 1)


@pytest.mark.parametrize("batch", [1, 2])
def test_the_mode_is_inert_below_five_rows(tiny, batch):
    A, _, B = tiny
    assert A.kv_cache_plan(2 * batch) == {"rounded": False, "attention_reads": "bf16", "bf16_cache": True}
    with Spy(A) as spy:
        got = _generate(A, batch)
    assert len(spy.bufs) == 1 and spy.bufs[0].kv_ptrs is not None and spy.bufs[0].codes is None and len(spy.bufs[0].ip.key_value_memory_dict) == 2
    _same_run(got, _generate(B, batch), f"generate(batch_size={batch})")


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
    A, F, _ = tiny
    with Spy(A) as spy:
        only = _batch(A, ragged, mixed)
    spy.assert_codes_only(1, "generate_batch")
    _same_run(only, _batch(F, ragged, mixed), f"generate_batch(ragged_prefix={ragged}, mixed_guidance={mixed}), 'fp8-only' against 'fp8'")


def _requests(n):
    return [GenRequest(_cond(40 + i, 4 + i % 3), sampling_params=dict(temperature=0.0), cfg_scale=(2.0, 1.5, 3.0)[i % 3], max_new_tokens=6 + i % 4) for i in range(n)]


def test_serve_session_in_which_requests_join_late(tiny):
    A, F, _ = tiny

    def session(model):
        src = _requests(5) + [None, None] + _requests(12)[5:]                  # 12 requests for 8 slots; some arrive while the session runs
        tr = {}
        out = {r.index: r for r in model.serve(iter(src), slots=8, max_prompt=8, max_new_tokens=10, guided=True, sched_every=4, _trace=tr)}
        assert sorted(out) == list(range(12)) and all(r.error is None for r in out.values())
        assert any(kind == "admit" and step > 0 for kind, step, _ in tr["slots"]), "no request joined the running session"
        held = [[b for b, who in enumerate(holders) if who is not None] for _, _, holders in tr["slots"]]
        return [out[i].codes.cpu() for i in range(12)], [l.cpu()[rows] for l, rows in zip(tr["logits"], held)], tr["slots"]
    with Spy(A) as spy:
        only = session(A)
    spy.assert_codes_only(1, "serve(slots=8)")
    both = session(F)
    assert only[2] == both[2], "the two sessions must schedule alike"
    _same_run(only, both, "serve(slots=8), 'fp8-only' against 'fp8'")


def test_serve_stream(tiny):
    A, F, _ = tiny

    def session(model):
        codes, wavs = {}, {}
        for ch in model.serve_stream(iter(_requests(10)), slots=8, max_prompt=8, max_new_tokens=10, guided=True, sched_every=4, chunk_frames=4):
            assert ch.error is None
            codes.setdefault(ch.index, []).append(ch.codes.cpu())
            wavs.setdefault(ch.index, []).append(ch.wav.cpu())
        return [torch.cat(codes[i], 2) for i in range(10)], [torch.cat(wavs[i], 2) for i in range(10)]
    with Spy(A) as spy:
        only = session(A)
    spy.assert_codes_only(1, "serve_stream(slots=8)")
    both = session(F)
    assert all(torch.equal(x, y) for x, y in zip(only[0], both[0])), "serve_stream: codes differ"
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(only[1], both[1])), "serve_stream: samples differ"


def test_with_the_fp8_mlp_stream():
    """Both FP8 modes on one model at full width: the same equality."""
    A, _ = build_model(dict(d_model=2048, n_layer=2, num_heads=16, num_heads_kv=4, d_ff=8192), 53, DEV)
    A.quantize_mlp_fp8()
    runs = {}
    for mode in ("fp8-only", "fp8"):
        A.set_kv_cache(mode)
        assert A.engine(16).mlp_fp8_plan(8) == [1, 1] and A.kv_cache_plan(8) == {"rounded": True, "attention_reads": "fp8", "bf16_cache": mode == "fp8"}
        runs[mode] = _generate(A, 4, steps=10, d_model=2048)
    _same_run(runs["fp8-only"], runs["fp8"], "quantize_mlp_fp8() + kv_cache='fp8-only' against 'fp8'")


def _canary_caches(n_layer, nbytes):
    return [torch.full((nbytes // 2,), KV_CANARY, dtype=bf, device=DEV) for _ in range(n_layer)]


def test_bf16_buffers_passed_anyway_are_never_touched(tiny):
    """The engine driven directly: a codes-only generation (prefill, eight steps) and a codes-only session (an admission, eight steps, an admission into
    a freed slot, eight steps) that are handed canary-filled bf16 caches find every element unchanged."""
    A, _, _ = tiny
    eng, st = A.engine(16), _lib.stream_ptr()
    n_layer, d = A.config.backbone.n_layer, synth.TINY_CFG["d_model"]
    sp = _sampling_struct({}, 0)
    g = torch.Generator().manual_seed(9)

    def buffers(rows, max_len):
        caches = _canary_caches(n_layer, int(eng.lib.zn_kv_bytes_per_layer(C.byref(eng.zc), rows, max_len)))
        codes = [torch.zeros(int(eng.lib.zn_kv_fp8_bytes_per_layer(C.byref(eng.zc), rows, max_len)), dtype=torch.uint8, device=DEV) for _ in range(n_layer)]
        return caches, codes, (C.c_void_p * n_layer)(*[c.data_ptr() for c in caches]), (C.c_void_p * n_layer)(*[c.data_ptr() for c in codes])

    def untouched(caches, what):
        torch.cuda.synchronize()
        assert all(bool((c == KV_CANARY).all()) for c in caches), f"{what}: a bf16 buffer of a codes-only generation was written"
    # a generation: 3 guided utterances = 6 rows
    caches, codes, kv_ptrs, code_ptrs = buffers(6, 32)
    lengths = torch.zeros(6, dtype=torch.int32, device=DEV)
    delayed = code_rows([None] * 3, [12] * 3, 12 + NQB, NQB, 1025, DEV)
    eng.call("zn_gen_begin", 3, kv_ptrs, 32, lengths.data_ptr(), delayed.data_ptr(), 12 + NQB, 1, 12, 2.0, C.byref(sp), st)
    try:
        eng.call("zn_gen_bind_kv_fp8", code_ptrs)
        hidden = torch.randn(6, 5, d, generator=g).to(bf).to(DEV)
        eng.call("zn_prefill", hidden.data_ptr(), 5, st)
        untouched(caches, "prefill")
        assert all(int(c.view(6, 32, -1)[:, :5].max()) > 0 for c in codes), "the prefill wrote no codes"
        eng.call("zn_decode_steps", 8, st)
        untouched(caches, "eight steps")
        assert lengths.tolist() == [13] * 6
    finally:
        torch.cuda.synchronize()
        eng.call("zn_gen_end")
    # a session: 4 guided slots = 8 rows
    slack = serve_slack(8)
    max_new, S = 6, 5
    width = max_new + NQB + slack
    max_len = (S - 1 + width + 7) // 8 * 8
    caches, codes, kv_ptrs, code_ptrs = buffers(8, max_len)
    lengths = torch.zeros(8, dtype=torch.int32, device=DEV)
    delayed = torch.full((4, NQB, width), 1025, dtype=torch.int32, device=DEV)

    def admit(slots):
        n = len(slots)
        adm = (_lib.zn_admit * n)()
        for j, slot in enumerate(slots):
            delayed[slot].copy_(code_rows([None], [max_new], width, NQB, 1025, DEV)[0])
            adm[j].slot, adm[j].row_len, adm[j].prefix_len = slot, S, 0
            adm[j].params.sp = _sampling_struct({}, 0)
            adm[j].params.cfg_scale, adm[j].params.max_new_tokens = 2.0, max_new
        hidden = torch.randn(2 * n, S, d, generator=g).to(bf).to(DEV)
        eng.call("zn_gen_admit", adm, n, hidden.data_ptr(), S, st)
        torch.cuda.synchronize()
    eng.call("zn_gen_begin", 4, kv_ptrs, max_len, lengths.data_ptr(), delayed.data_ptr(), width, 1, max_new, 2.0, C.byref(sp), st)
    try:
        eng.call("zn_gen_bind_kv_fp8", code_ptrs)
        eng.call("zn_gen_open_slots", slack)
        admit([0, 2])
        untouched(caches, "an admission")
        seen = codes[0].view(8, max_len, -1)
        assert int(seen[0, :S].max()) > 0 and int(seen[2, :S].max()) > 0 and int(seen[[1, 3, 5, 7]].max()) == 0, "rows that are not named stay untouched"
        eng.call("zn_decode_steps", 8, st)
        untouched(caches, "eight steps of the session")
        eng.call("zn_decode_steps", 8, st)
        eng.call("zn_gen_retire", 0)
        eng.call("zn_gen_retire", 2)
        admit([0, 1])
        eng.call("zn_decode_steps", 8, st)
        untouched(caches, "an admission into a freed slot and eight more steps")
    finally:
        torch.cuda.synchronize()
        eng.call("zn_gen_end")


# ---------------------------------------------------------------------------------------------- 5. the refusals
def test_refusals(tiny):
    A, _, _ = tiny
    eng, st = A.engine(16), _lib.stream_ptr()
    n_layer, d = A.config.backbone.n_layer, synth.TINY_CFG["d_model"]
    out = (C.c_int32 * 3)()
    eng.call("zn_kv_cache_plan", 16, out)
    assert list(out) == [1, 1, 0]
    eng.call("zn_kv_cache_plan", 4, out)
    assert list(out) == [0, 0, 1]

    def rc_of(name, *args):
        with torch.cuda.device(eng.device):
            rc = getattr(eng.lib, name)(eng.h, *args)
        return rc, eng.lib.zn_last_error(eng.h).decode()
    # the setter inside a generation
    gen = A.serve(iter(_requests(2)), slots=4, max_prompt=8, max_new_tokens=10, guided=True)
    next(gen)
    rc, msg = rc_of("zn_set_kv_fp8_only", 0)
    assert rc == -3 and "inside a generation" in msg
    gen.close()
    # a codes-only generation with no code caches bound: ZN_ERR_STATE from the prefill, an admission and the steps - never a bf16 generation
    sp = _sampling_struct({}, 0)
    lengths = torch.zeros(8, dtype=torch.int32, device=DEV)
    delayed = torch.full((4, NQB, 40), 1025, dtype=torch.int32, device=DEV)
    hidden = torch.zeros(8, 4, d, dtype=bf, device=DEV)
    eng.call("zn_gen_begin", 4, None, 48, lengths.data_ptr(), delayed.data_ptr(), 40, 1, 8, 2.0, C.byref(sp), st)
    try:
        rc, msg = rc_of("zn_prefill", hidden.data_ptr(), 4, st)
        assert rc == -3 and "zn_gen_bind_kv_fp8" in msg
        rc, msg = rc_of("zn_decode_steps", 1, st)
        assert rc == -3 and "zn_gen_bind_kv_fp8" in msg
        eng.call("zn_gen_open_slots", serve_slack(8))
        adm = (_lib.zn_admit * 1)()
        adm[0].slot, adm[0].row_len, adm[0].prefix_len = 0, 4, 0
        adm[0].params.sp, adm[0].params.cfg_scale, adm[0].params.max_new_tokens = sp, 2.0, 4
        rc, msg = rc_of("zn_gen_admit", adm, 1, hidden.data_ptr(), 4, st)
        assert rc == -3 and "zn_gen_bind_kv_fp8" in msg
        assert lengths.tolist() == [0] * 8
    finally:
        torch.cuda.synchronize()
        eng.call("zn_gen_end")
    # with the second flag off the NULL caches are the error they were
    eng.call("zn_set_kv_fp8_only", 0)
    try:
        eng.call("zn_kv_cache_plan", 16, out)
        assert list(out) == [1, 1, 1]
        rc, _ = rc_of("zn_gen_begin", 4, None, 48, lengths.data_ptr(), delayed.data_ptr(), 40, 1, 8, 2.0, C.byref(sp), st)
        assert rc == -1
    finally:
        eng.call("zn_set_kv_fp8_only", 1)
    # below 5 rows the mode is inert: NULL caches are refused there too
    rc, _ = rc_of("zn_gen_begin", 2, None, 48, lengths.data_ptr(), delayed.data_ptr(), 40, 1, 8, 2.0, C.byref(sp), st)
    assert rc == -1
    # a hybrid handle
    model, _ = build_model(synth.HYBRID_TINY_CFG, 23, DEV)
    heng = model.engine(4)
    with torch.cuda.device(heng.device):
        assert heng.lib.zn_set_kv_fp8_only(heng.h, 1) == -4 and "hybrid" in heng.lib.zn_last_error(heng.h).decode()
    with pytest.raises(ValueError, match="hybrid"):
        model.set_kv_cache("fp8-only")
