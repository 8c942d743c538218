"""Decode and prefill attention as single ops, per launch shape: every output element of zn_op_attn_decode and zn_op_attn_prefill_rows is held to
the float64 interval of zonos_amd.testing.attention_reference - no mean, no exempted element (tests/test_attention_compare_cpu.py shows on the
CPU that torch's SDPA and a plain fp32 restatement stay inside it on every case here, and that ten subtly wrong kernels do not).  Every case
runs once per tail pattern (AT_TAILS: the keys at or past a row's context hold zeros, finite data, and four NaN / Inf bit patterns - the cache
is torch.empty in production) and must give the SAME BITS each time; q, kv and out sit between canaries, out is filled with the canary before the
call, the inputs must come back unchanged, and the op runs twice per pattern so that the split pass's tickets are back at zero.

Case -> kernel (AttnCase.kernel, printed with every case):
  d128g4 r{1,2,4} cap512                      attn_block_kernel<128,4,fused,DS1>
  d128g4 r16 cap512, r4 split_cols=2          attn_block_kernel<128,4,fused,DS4> with the npairs % 8 == 0 workgroup remap (32 and 8 pairs)
  d128g4 r{5,6} cap512, r2 split_cols=2       attn_block_kernel<128,4,fused,DS4> without it (10, 12 and 4 pairs)
  d128g4 r16 cap512 split_cols=1              attn_block_kernel<128,4,fused,DS1> at 16 rows
  d128g4 r* cap520 / cap1032, fused_max=1     attn_scores_kernel<128,4> + attn_block_kernel<128,4,split,DS1> (rows <= 4) or DS2 (rows >= 5, split_cols=2)
  d128g{1,2,8}, d64g{4,2}, d32g{4,8}          the same two shapes at the other groups and head sizes (DS1 below head size 128)
  d128g4 rise / fall / tie, d64g4 rise        the block recurrence with f_j < 1e-20, f_j = 1 and a tie across keys 511 | 512
  d128g4 r2 cap{4096..16384} nb{8,9,16,17,32} the eight-at-a-time loops of the ticketed combine, up to the 32-block limit
  p128g{1,2,4,8} mfma *                       attn_prefill_mfma_kernel<G>
  p{128,64,32}g* valu *                       attn_prefill_kernel<hd,G>
  ... S{n}+{base}, ... ragged                 base > 0 (the seam) and row_len (the ragged prefill) of either kernel"""
import ctypes as C

import pytest
import torch

from zonos_amd import _lib
from zonos_amd import testing as T
from zonos_amd.backbone import HipEngine
from zonos_amd.testing import (AT_TAILS, attention_apply_tail, attention_case_tensors, attention_compare, attention_device_layout,
                               attention_from_device_layout, attention_reference, build_model)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PADN, CANARY = 4096, 768.0             # canary elements in front of and behind every buffer; their value (exact in bf16)
TUNE_DEFAULT = {"ZN_TUNE_ATTN_SPLIT_COLS": 3, "ZN_TUNE_ATTN_FUSED_MAX_KEYS": 512, "ZN_TUNE_PREFILL_ATTN_VALU": 1}
bf = torch.bfloat16


def _engine(hd, G, n_layer=1):
    hq, hkv = T.AT_GEOM[(hd, G)]
    model, _ = build_model(dict(d_model=hq * hd, n_layer=n_layer, num_heads=hq, num_heads_kv=hkv, d_ff=256), 31, DEV)
    eng = HipEngine(model.backbone, max_rows=16)
    eng._model = model
    return eng


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(hd, G):
        if (hd, G) not in cache:
            cache[(hd, G)] = _engine(hd, G)
        return cache[(hd, G)]
    return get


class Guarded:
    """[PADN canary elements | the tensor | PADN canary elements] in one allocation."""

    def __init__(self, shape, dtype=bf):
        n = 1
        for s in shape:
            n *= int(s)
        self.buf = torch.full((n + 2 * PADN,), CANARY, dtype=dtype, device=DEV)
        self.view = self.buf[PADN:PADN + n].view(*shape)

    def ptr(self):
        return self.view.data_ptr()

    def check(self, label):
        assert bool((self.buf[:PADN] == CANARY).all()) and bool((self.buf[-PADN:] == CANARY).all()), f"{label}: a canary was overwritten"


def _launch(eng, c, q, kv, out, lengths, ext, row_len, st, entry=None):
    if c.kind == "decode":
        eng.call("zn_op_attn_decode", q.ptr(), kv.ptr(), c.cap, lengths.data_ptr(), None if ext is None else ext.data_ptr(), out.ptr(), c.R, st)
    elif entry == "zn_op_attn_prefill":
        eng.call("zn_op_attn_prefill", q.ptr(), kv.ptr(), c.cap, out.ptr(), c.S, c.R, st)
    else:
        eng.call("zn_op_attn_prefill_rows", q.ptr(), kv.ptr(), c.cap, out.ptr(), c.S, c.R, c.base, None if row_len is None else row_len.data_ptr(), st)


_REFS: dict = {}


def case_ref(c):
    """Tensors and interval of a case; the ext variants of a shape share theirs (ext moves the fexp / libm split only)."""
    key = c._replace(name="", ext="null", tune=(), kernel="")
    if key not in _REFS:
        t = attention_case_tensors(c._replace(ext="null"))
        _REFS[key] = (t, attention_reference(t["q"], t["k"], t["v"], t["scale"], t["visible"]))
    return _REFS[key]


def run_case(eng, c, tails=AT_TAILS):
    """One case over every tail pattern; returns the output bits [R][Hq][Sq][hd] (the same for every pattern) and the interval."""
    st = _lib.stream_ptr()
    t0, ref = case_ref(c)
    t = attention_case_tensors(c) if c.ext != "null" else t0
    q0, kv0 = (x.to(DEV) for x in attention_device_layout(c, t))
    q, kv, out = Guarded(q0.shape), Guarded(kv0.shape), Guarded(q0.shape)
    lengths = ext = row_len = None
    if c.kind == "decode":
        lengths = (torch.tensor(c.lens, dtype=torch.int32) - 1).to(DEV)
        ext = None if t["ext"] is None else t["ext"].to(torch.int32).to(DEV)
    elif c.ragged:
        row_len = torch.tensor(c.lens, dtype=torch.int32, device=DEV)
    cmp = ref.valid[:, None, :, None].expand_as(ref.lo)
    first, outside, nonfinite, headroom = None, 0, 0, 0.0
    try:
        for key, val in c.tune:
            eng.call("zn_debug_tune", getattr(_lib, key), val)
        for tail in tails:
            q.view.copy_(q0)
            kv.view.copy_(kv0)
            attention_apply_tail(c, q.view, kv.view, t["start"], tail)
            q_in, kv_in = q.view.clone(), kv.view.clone()
            for _ in range(2):                           # twice: the arrival tickets must be back at zero after a launch
                out.view.fill_(CANARY)
                _launch(eng, c, q, kv, out, lengths, ext, row_len, st)
            torch.cuda.synchronize()
            label = f"{c.name} tail {tail}"
            for g in (q, kv, out):
                g.check(label)
            assert torch.equal(q.view.view(torch.int16), q_in.view(torch.int16)) and torch.equal(kv.view.view(torch.int16), kv_in.view(torch.int16)), \
                f"{label}: an input was written"
            got = attention_from_device_layout(c, out.view)
            if not bool(cmp.all()):                      # positions at or past row_len[r] keep the canary
                assert bool((got.float()[~cmp] == CANARY).all()), f"{label}: a position at or past row_len was written"
            res = attention_compare(got, ref, label, quiet=True)
            assert res.ok and res.outside == 0 and res.nonfinite == 0, (label, c.kernel, res.line(label))
            outside, nonfinite, headroom = outside + res.outside, nonfinite + res.nonfinite, max(headroom, res.headroom)
            if first is None:
                first = got
                if c.kind == "prefill" and c.base == 0 and not c.ragged:      # the production entry: the same launch, the same bits
                    out.view.fill_(CANARY)
                    _launch(eng, c, q, kv, out, lengths, ext, row_len, st, entry="zn_op_attn_prefill")
                    torch.cuda.synchronize()
                    assert torch.equal(attention_from_device_layout(c, out.view).view(torch.int16), got.view(torch.int16)), label
            else:
                assert torch.equal(got.view(torch.int16)[cmp], first.view(torch.int16)[cmp]), f"{label}: the output depends on what the tail holds"
    finally:
        for key, _ in c.tune:
            eng.call("zn_debug_tune", getattr(_lib, key), TUNE_DEFAULT[key])
    print(f"[attention {c.name}] {c.kernel}: outside [lo, hi] {outside}, non-finite {nonfinite} of {int(cmp.sum())} x {len(tails)} tails (identical bits); "
          f"worst |got - exact| / (Theta A) {headroom:.3f}; Theta max {float(ref.theta.max()):.3g}; eta_exp {T.AT_FEXP_MEASURED:.4g} -> 2^-13")
    return first, ref


def _decode(pred):
    return [c for c in T.attention_cases_decode() if pred(c)]


_plain = lambda c: c.ext == "null" and c.family in ("spot", "diffuse") and c.cap <= 1032


@pytest.mark.parametrize("cap", [512, 520, 1032])
def test_decode_head128_group4_rows_and_column_split(engines, cap):
    """Rows 1, 2, 4, 5, 6 and 16 at one capacity (fused at 512; scores + block pass at 520 and 1032), the value-column split by default and forced
    both ways, ragged contexts on every chunk, round and block edge."""
    cases = _decode(lambda c: _plain(c) and (c.hd, c.G) == (128, 4) and c.cap == cap)
    assert len(cases) >= 9
    for c in cases:
        run_case(engines(128, 4), c)


@pytest.mark.parametrize("hd,G", [(128, 1), (128, 2), (128, 8), (64, 4), (64, 2), (32, 4), (32, 8)])
def test_decode_other_groups_and_head_sizes(engines, hd, G):
    cases = _decode(lambda c: _plain(c) and (c.hd, c.G) == (hd, G))
    assert len(cases) == 4
    for c in cases:
        run_case(engines(hd, G), c)


def test_decode_score_range_and_block_recurrence(engines):
    cases = _decode(lambda c: c.family in ("rise", "fall", "tie"))
    assert len(cases) == 5
    for c in cases:
        run_case(engines(c.hd, c.G), c)


@pytest.mark.parametrize("cap", [4096, 4608, 8192, 8704, 16384])
def test_decode_combine_depth(engines, cap):
    (c,) = _decode(lambda c: c.cap == cap)
    run_case(engines(128, 4), c)


def test_decode_ext_moves_only_the_exponential_split(engines):
    """ext = NULL, L, and L rounded up to the reference's query split: every variant inside the interval; ext < L gives the bits of NULL."""
    eng = engines(128, 4)
    for cap in (512, 1032):
        cases = {c.ext: c for c in _decode(lambda c: c.ext != "null" and c.cap == cap)}
        assert set(cases) == {"L", "split", "short"}
        null, _ = run_case(eng, cases["L"]._replace(name=cases["L"].name.replace("ext=L", "ext=NULL"), ext="null"), tails=AT_TAILS[:3])
        bits = {e: run_case(eng, c, tails=AT_TAILS[:3])[0] for e, c in cases.items()}
        assert torch.equal(bits["short"].view(torch.int16), null.view(torch.int16)), "ext below L must not change a bit"
        assert torch.equal(bits["L"].view(torch.int16), null.view(torch.int16)), "ext = L is what NULL means"


def test_decode_refuses_more_than_32_blocks(engines):
    eng = engines(128, 4)
    hq, hkv = T.AT_GEOM[(128, 4)]
    cap = 16385
    q, out = Guarded((2, hq * 128)), Guarded((2, hq * 128))
    kv = torch.zeros(2, cap, 2, hkv, 128, dtype=bf, device=DEV)
    lengths = torch.tensor([cap - 1, 5], dtype=torch.int32, device=DEV)
    with torch.cuda.device(eng.device):
        rc = eng.lib.zn_op_attn_decode(eng.h, q.ptr(), kv.data_ptr(), cap, lengths.data_ptr(), None, out.ptr(), 2, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and "32 blocks" in eng.lib.zn_last_error(eng.h).decode(), (rc, eng.lib.zn_last_error(eng.h))
    assert bool((out.buf == CANARY).all()), "a refused call launched something"
    (c,) = _decode(lambda c: c.name == "d128g4 r2 cap512")              # and the handle still serves what fits
    run_case(eng, c, tails=AT_TAILS[:1])


def test_decode_short_context_after_long_one_matches_a_fresh_handle(engines):
    """h->scores, h->cmax, h->pv_part and the tickets outlive a launch: 1500 keys, then 3 keys at the same capacity, on one handle, against the
    same 3-key launch on a handle that has seen nothing."""
    used, fresh = engines(128, 4), _engine(128, 4)
    long = T.AttnCase("d128g4 history 1500", "decode", "spot", 128, 4, 1536, (1500, 1400), kernel="scores + split")
    short = T.AttnCase("d128g4 history 3", "decode", "spot", 128, 4, 1536, (3, 2), kernel="scores + split")
    run_case(used, long, tails=AT_TAILS[:1])
    a, _ = run_case(used, short, tails=AT_TAILS[:3])
    b, _ = run_case(fresh, short, tails=AT_TAILS[:3])
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "the result depends on what an earlier launch left in the workspace"


def _prefill(pred):
    return [c for c in T.attention_cases_prefill() if pred(c)]


@pytest.mark.parametrize("kern,hd,G", [("mfma", 128, 1), ("mfma", 128, 2), ("mfma", 128, 4), ("mfma", 128, 8), ("valu", 128, 1), ("valu", 128, 2), ("valu", 128, 4),
                                       ("valu", 128, 8), ("valu", 64, 4), ("valu", 64, 2), ("valu", 32, 4), ("valu", 32, 8)])
def test_prefill_every_kernel(engines, kern, hd, G):
    """S = 1, TQ - 1, TQ, TQ + 1 (TQ = 64 / G positions per workgroup), 513, ragged row_len; at G = 4: the query-split thresholds 191 / 192 / 767 /
    768, the block edge 512, base 5 / 500 / 511 with S = 20 (the seam), the range cases, and 1025 positions once."""
    cases = _prefill(lambda c: (c.hd, c.G) == (hd, G) and f" {kern} " in c.name)
    assert len(cases) >= 5 and all((kern == "mfma") == ("mfma" in c.kernel) for c in cases)
    for c in cases:
        run_case(engines(hd, G), c)


def test_prefill_rows_entry_validates_before_launching(engines):
    eng = engines(128, 4)
    hq, hkv = T.AT_GEOM[(128, 4)]
    S, cap = 8, 16
    q, out = Guarded((2, S, hq * 128)), Guarded((2, S, hq * 128))
    kv = torch.zeros(2, cap, 2, hkv, 128, dtype=bf, device=DEV)
    st = _lib.stream_ptr()

    def call(qp, kvp, outp, S_, rows, base):
        with torch.cuda.device(eng.device):
            return eng.lib.zn_op_attn_prefill_rows(eng.h, qp, kvp, cap, outp, S_, rows, base, None, st)
    assert call(q.ptr(), kv.data_ptr(), out.ptr(), S, 2, -1) == -1
    assert call(q.ptr(), kv.data_ptr(), out.ptr(), S, 2, cap - S + 1) == -1 and "positions" in eng.lib.zn_last_error(eng.h).decode()
    assert call(None, kv.data_ptr(), out.ptr(), S, 2, 0) == -1 and call(q.ptr(), None, out.ptr(), S, 2, 0) == -1 and call(q.ptr(), kv.data_ptr(), None, S, 2, 0) == -1
    assert call(q.ptr(), kv.data_ptr(), out.ptr(), S, 18, 0) == -1 and "max_rows" in eng.lib.zn_last_error(eng.h).decode()
    assert eng.lib.zn_op_attn_prefill_rows(None, q.ptr(), kv.data_ptr(), cap, out.ptr(), S, 2, 0, None, st) == -1
    torch.cuda.synchronize()
    assert bool((out.buf == CANARY).all()), "a refused call launched something"
    assert call(q.ptr(), kv.data_ptr(), out.ptr(), S, 2, cap - S) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("rows", [1, 2])
def test_layer_path_does_not_read_the_cache_tail(rows):
    """zn_op_backbone_forward on a two-layer model with caller-owned caches: one decode position at base 9, seven positions at base 0 and at base 9.
    The cache positions the call does not write - at or past base + S - hold zeros in one run and NaN / Inf patterns in the other (torch.empty in
    production): the outputs are the same bits, and those positions come back as they were."""
    eng = _engine(128, 4, n_layer=2)
    hq, hkv = T.AT_GEOM[(128, 4)]
    d, cap = hq * 128, 24
    for S, base in ((1, 9), (7, 0), (7, 9)):
        hidden = torch.from_numpy(T.synth.normal(T.AT_SEED, f"at.layer.h.{rows}.{S}", (rows, S, d))).to(bf).to(DEV)
        outs = []
        for tail in ("zeros", "0x7FC0", "0xFFFF", "0x7F80"):
            caches = []
            for li in range(2):
                kv = torch.from_numpy(T.synth.normal(T.AT_SEED, f"at.layer.kv.{li}.{rows}", (rows, cap, 2, hkv, 128))).to(bf).to(DEV)
                bits = 0 if tail == "zeros" else int(tail, 16)
                kv.view(torch.int16)[:, base:] = bits - 65536 if bits >= 32768 else bits
                caches.append(kv)
            before = [kv.clone() for kv in caches]
            ptrs = (C.c_void_p * 2)(*[kv.data_ptr() for kv in caches])
            out = Guarded((rows, S, d))
            eng.call("zn_op_backbone_forward", hidden.data_ptr(), out.ptr(), ptrs, cap, base, S, rows, _lib.stream_ptr())
            torch.cuda.synchronize()
            out.check(f"layer path S {S} base {base} tail {tail}")
            assert bool(torch.isfinite(out.view.float()).all()), (S, base, tail)
            for kv, b in zip(caches, before):
                assert torch.equal(kv.view(torch.int16)[:, :base], b.view(torch.int16)[:, :base]) and \
                    torch.equal(kv.view(torch.int16)[:, base + S:], b.view(torch.int16)[:, base + S:]), "a cache position the call does not own changed"
                assert bool(torch.isfinite(kv[:, base:base + S].float()).all())
            outs.append(out.view.clone())
        for o in outs[1:]:
            assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16)), f"S {S} base {base}: the output depends on what the cache tail holds"
        print(f"[attention layer path rows {rows} S {S} base {base}] bit-identical over 4 tail patterns; decode path of the handle "
              f"{eng.lib.zn_decode_path(eng.h)} (detail {eng.lib.zn_decode_path_detail(eng.h)})")
