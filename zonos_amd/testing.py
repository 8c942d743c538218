"""Helpers shared by tests, bench.py and smoke(): build a `Zonos` around synthetic weights (zonos_amd/synth.py)."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import synth
from .autoencoder import DACAutoencoder
from .config import BackboneConfig, PrefixConditionerConfig, ZonosConfig
from .model import Zonos


def _attn_cfg(cfg: dict) -> dict:
    """config.json's backbone.attn_cfg for a synthetic configuration.  Hybrid configurations without an "attn_cfg" entry keep
    the attention form of the first hybrid tests (interleaved rotary over the whole head, no biases), spelled out here
    because mamba_ssm's MHA defaults differ (zonos_amd/backbone/_hip.py attention_options)."""
    base = dict(num_heads=cfg["num_heads"], num_heads_kv=cfg["num_heads_kv"])
    if not cfg.get("ssm_cfg"):
        return base
    if "attn_cfg" in cfg:
        return {**base, **cfg["attn_cfg"]}
    return {**base, "causal": True, "rotary_emb_dim": cfg["d_model"] // cfg["num_heads"], "rotary_emb_interleaved": True,
            "qkv_proj_bias": False, "out_proj_bias": False}


def zonos_config(cfg: dict, conditioners: list | None = None, projection: str = "none") -> ZonosConfig:
    return ZonosConfig(BackboneConfig(d_model=cfg["d_model"], n_layer=cfg["n_layer"], attn_mlp_d_intermediate=cfg["d_ff"],
                                      attn_layer_idx=list(cfg.get("attn_layer_idx", range(cfg["n_layer"]))), ssm_cfg=dict(cfg.get("ssm_cfg") or {}),
                                      attn_cfg=_attn_cfg(cfg), rms_norm=bool(cfg.get("rms_norm", False)),
                                      residual_in_fp32=bool(cfg.get("residual_in_fp32", False))),
                       PrefixConditionerConfig(list(conditioners or []), projection))


def build_model(cfg: dict, seed: int, device="cuda", dac: DACAutoencoder | None = None, peaky: bool = False, conditioners: list | None = None,
                projection: str = "none"):
    """Returns (model on `device`, CPU state dict).  The state dict uses the reference's key contract."""
    sd = synth.zonos_state_dict(cfg, seed, peaky=peaky)
    sd.update({"prefix_conditioner." + k: v for k, v in synth.conditioner_state_dict(conditioners or [], cfg["d_model"], seed, projection).items()})
    with torch.device("meta"):
        model = Zonos(zonos_config(cfg, conditioners, projection), autoencoder=dac or DACAutoencoder())
    model.load_state_dict({k: v for k, v in sd.items()}, assign=True, strict=True)
    model = model.to(device)
    return model.eval(), sd


# ------------------------------------------------------------------ DAC decode: small configurations and the pointwise comparator

# Decoder configurations small enough for a float64 CPU oracle in a fraction of a second, chosen for what the 44.1 kHz one never reaches:
# output-channel counts below a tile (32, 48), every output-channel tiling of the fp32 family (64 | 96 | 128, and the pad-to-128 branch),
# strides 6 and 10, and rows per frame (6, 12 | 2, 12, 120 | 4, 24) that the 128-row tiles are no multiple of.
DAC_SMALL = {
    "S1": dict(hidden=64, dec_hidden=128, ratios=(6, 2)),
    "S2": dict(hidden=32, dec_hidden=256, ratios=(2, 6, 10)),
    "S3": dict(hidden=48, dec_hidden=192, ratios=(4, 6)),
}
DAC_SMALL_CODEBOOK = 64


def build_small_dac(name: str, seed: int = 4321, device="cuda:0"):
    """Returns (DACAutoencoder of DAC_SMALL[name] with decoder-only synthetic weights, CPU state dict, ratios)."""
    c = DAC_SMALL[name]
    dw = synth.dac_state_dict(seed, encoder=False, codebook_size=DAC_SMALL_CODEBOOK, **c)
    ae = DACAutoencoder(dw, config=dict(codebook_size=DAC_SMALL_CODEBOOK, hidden_size=c["hidden"], decoder_hidden_size=c["dec_hidden"],
                                        upsampling_ratios=tuple(c["ratios"])), device=device)
    return ae, dw, tuple(c["ratios"])


DAC_POINTWISE_FACTOR = 8.0     # bar: max|gpu - oracle64| <= 8 x max|oracle32 - oracle64| over the case


class DacPointwise(NamedTuple):
    e32: float                 # max|oracle32 - oracle64|: what fp32 arithmetic alone costs on this case
    err: float                 # max|gpu - oracle64|
    ratio: float               # err / e32
    index: tuple               # (batch row, sample) of the worst sample
    ok: bool                   # err <= factor * e32

    def line(self, label: str, hop: int) -> str:
        b, s = self.index
        return (f"[dac pointwise {label}] err/e32 {self.ratio:.3f} (err {self.err:.3g}, e32 {self.e32:.3g}) worst at row {b} sample {s}: "
                f"mod 128 = {s % 128}, mod hop {hop} = {s % hop}")


def dac_oracle_pair(dw: dict, codes: torch.Tensor, ratios) -> tuple[torch.Tensor, torch.Tensor]:
    """The CPU oracle's waveform as committed (fp32) and with every weight cast to float64 (the same code, float64 end to end)."""
    from oracle import zonos_oracle as zo
    codes = codes.cpu().long()
    ref32 = zo.dac_decode(dw, codes, ratios=tuple(ratios))
    ref64 = zo.dac_decode({k: v.double() for k, v in dw.items()}, codes, ratios=tuple(ratios))
    assert ref32.dtype == torch.float32 and ref64.dtype == torch.float64
    return ref32, ref64


def pointwise_compare(wav, ref32, ref64, hop: int, label: str = "", factor: float = DAC_POINTWISE_FACTOR) -> DacPointwise:
    """Worst single sample of `wav` [B, 1, N] against the float64 reference, in units of the fp32 reference's own worst sample.  Prints one
    line: the ratio and where the worst sample sits (modulo the 128-sample tile of the last layers and modulo the hop)."""
    w = torch.as_tensor(wav).detach().cpu().double()
    r32, r64 = torch.as_tensor(ref32).double(), torch.as_tensor(ref64).double()
    if not (w.shape == r32.shape == r64.shape):
        raise ValueError(f"shapes differ: {tuple(w.shape)} vs {tuple(r32.shape)} / {tuple(r64.shape)}")
    e32 = float((r32 - r64).abs().max())
    d = (w - r64).abs().reshape(w.shape[0], -1)
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
    flat = int(d.argmax())
    b, s = divmod(flat, d.shape[1])
    err = float(d[b, s])
    res = DacPointwise(e32, err, err / e32 if e32 > 0 else float("inf"), (b, s), err <= factor * e32)
    print("\n" + res.line(label, hop))
    return res


def dac_pointwise(wav, dw: dict, codes: torch.Tensor, ratios, label: str = "", refs=None) -> DacPointwise:
    """Pointwise comparison of a GPU waveform with zo.dac_decode in float64 (`refs`: a dac_oracle_pair() computed before, to share it)."""
    ref32, ref64 = refs if refs is not None else dac_oracle_pair(dw, codes, ratios)
    hop = 1
    for r in ratios:
        hop *= int(r)
    return pointwise_compare(wav, ref32, ref64, hop, label)


# ------------------------------------------------------------------ fused linears: float64 interval reference, comparator, case table
# One fused linear out = epi(pro(x) W^T) (zn_op_linear_fused) against float64 arithmetic on the bf16 operands.  The bar is an interval per
# output element, not a tolerance: a = sum_k x~[r,k] W[n,k] exactly (bf16 x bf16 products are exact in fp32, their float64 sum is exact to
# 2^-53), e = 1.01 K 2^-24 sum_k |x~ W| bounds the error of an fp32 sum of those products in ANY order (fma chains, matrix cores, split-K
# slices, ticketed combines), and every epilogue is a composition of monotone roundings, so the least and greatest value the kernel may store
# are the epilogue at the ends (or corners) of [a - e, a + e].  lo and hi are bf16 values themselves: lo <= got <= hi is an exact test.
LF_PRO_NONE, LF_PRO_LN, LF_PRO_GATED = 0, 1, 2
LF_STORE, LF_RESID, LF_SILU, LF_ROPE_KV, LF_F32 = 0, 1, 2, 3, 4
LF_SUM_BOUND = 1.01 * 2.0 ** -24          # per term of the contraction: the a-priori bound of an fp32 sum in any order
LF_AMBIGUOUS_CAP = 0.01                   # condition on the committed inputs: at most 1 % of a row's normalised elements sit at a bf16 rounding boundary
# silu in fp32, g / (1 + expf(-g)): expf within 1 ulp, the add and the correctly rounded divide within 0.5 ulp each, and the error of expf
# reaches the quotient scaled by E / (1 + E) <= 1: relative error <= 2 * 2^-24 (1 + o(1)) < 2^-22.  The reference evaluates silu in float64 and
# widens its ends by that before the bf16 rounding.
LF_SILU_FP32_REL = 2.0 ** -22
_SILU_ARGMIN, _SILU_MIN = -1.2784645427610738, -0.27846454276107374


def bf16_round64(v: torch.Tensor) -> torch.Tensor:
    """float64 -> the bf16 value the kernels' two roundings (fp32, then bf16, both to nearest even) give, as float64.  Monotone."""
    return v.to(torch.float32).to(torch.bfloat16).to(torch.float64)


class LinearFusedRef(NamedTuple):
    lo: torch.Tensor           # float64 tensors holding bf16 values (fp32-exact for LF_F32): [rows][N], LF_SILU [rows][N / 2], LF_ROPE_KV [rows][q | k | v]
    hi: torch.Tensor
    mid: torch.Tensor          # the epilogue of a itself
    ambiguous: float           # largest share of a row's normalised activations that may round to either bf16 neighbour
    xt: torch.Tensor           # the activation the contraction saw (float64 of bf16 values), centre choice


def fused_activation(pro: int, x, ln_w, ln_b, gv, eps: float):
    """(centre, low, high) of the activation the kernel's contract defines, as float64 of bf16 values: x itself, bf16(LayerNorm64(x)), or the
    gated RMS form bf16(v rstd w) of gemv_kernel's PRO_GATED.  A normalised element whose float64 value lies within delta of a bf16 rounding
    boundary may round either way; delta = DAC_POINTWISE_FACTOR x the row's max |torch fp32 CPU form - float64| (the reference's own arithmetic)."""
    if pro == LF_PRO_NONE:
        xc = x.double()
        return xc, xc, xc
    if pro == LF_PRO_LN:
        K = x.shape[-1]
        xd, w, b = x.double(), ln_w.double(), ln_b.double()
        mu = xd.mean(-1, keepdim=True)
        v64 = (xd - mu) / torch.sqrt(((xd - mu) ** 2).mean(-1, keepdim=True) + eps) * w + b
        v32 = torch.nn.functional.layer_norm(x.float(), (K,), ln_w.float(), ln_b.float(), eps).double()
    else:
        g, gf = gv.double(), gv.float()
        v64 = g / torch.sqrt((g * g).mean(-1, keepdim=True) + eps) * ln_w.double()
        v32 = ((gf * (1.0 / torch.sqrt((gf * gf).mean(-1, keepdim=True) + eps))) * ln_w.float()).double()
    delta = DAC_POINTWISE_FACTOR * (v32 - v64).abs().amax(-1, keepdim=True)
    return bf16_round64(v64), bf16_round64(v64 - delta), bf16_round64(v64 + delta)


def _silu64(g):
    return g / (1.0 + torch.exp(-g))


def _rope_corners(t0s, t1s, cs, sn):
    """bf16 results of the interleaved-pair rotation (four fp32 products and two fp32 sums, each rounded on its own: zn_rope_pair) at every
    combination of the given pair values; returns (re_min, re_max, im_min, im_max)."""
    res, ims = [], []
    for x0 in t0s:
        for x1 in t1s:
            x0f, x1f = x0.float(), x1.float()
            res.append((x0f * cs - x1f * sn).to(torch.bfloat16).double())
            ims.append((x1f * cs + x0f * sn).to(torch.bfloat16).double())
    res, ims = torch.stack(res), torch.stack(ims)
    return res.amin(0), res.amax(0), ims.amin(0), ims.amax(0)


def linear_fused_reference(pro: int, epi: int, W, x=None, ln_w=None, ln_b=None, gv=None, bias=None, resid=None, eps: float = 1e-5,
                           rope=None, positions=None, hd: int = 0, n_heads: int = 0, n_heads_kv: int = 0, chunk: int = 4096) -> LinearFusedRef:
    """CPU tensors in (bf16; gv fp32; rope fp32 [positions][hd / 2][2]; positions int [rows], already clamped to the table)."""
    xc, xl, xh = fused_activation(pro, x, ln_w, ln_b, gv, float(np.float32(eps)))
    rows, K = xc.shape
    N = W.shape[0]
    span, xa = xh - xl, torch.maximum(xl.abs(), xh.abs())
    ambiguous = float((span != 0).double().mean(-1).max())
    a, e = torch.empty(rows, N, dtype=torch.float64), torch.empty(rows, N, dtype=torch.float64)
    for n0 in range(0, N, chunk):
        w = W[n0:n0 + chunk].double()
        wa = w.abs()
        a[:, n0:n0 + chunk] = xc @ w.T
        e[:, n0:n0 + chunk] = LF_SUM_BOUND * K * (xa @ wa.T) + span @ wa.T          # (for the ambiguous k: |W[n,k]| ulp_bf16(x~_k))
    al, ah = a - e, a + e
    if epi == LF_STORE:
        b = bias.double() if bias is not None else 0.0
        f = lambda t: bf16_round64(t + b)
        lo, hi, mid = f(al), f(ah), f(a)
    elif epi == LF_F32:
        lo, hi, mid = bf16_round64(al), bf16_round64(ah), bf16_round64(a)
    elif epi == LF_RESID:
        f = lambda t: bf16_round64(resid.double() + bf16_round64(t))
        lo, hi, mid = f(al), f(ah), f(a)
    elif epi == LF_SILU:
        F = N // 2
        yl, yh, gl, gh = bf16_round64(al[:, :F]), bf16_round64(ah[:, :F]), bf16_round64(al[:, F:]), bf16_round64(ah[:, F:])
        s0, s1 = _silu64(gl), _silu64(gh)
        smin, smax = torch.minimum(s0, s1), torch.maximum(s0, s1)
        smin = torch.where((gl < _SILU_ARGMIN) & (gh > _SILU_ARGMIN), torch.full_like(smin, _SILU_MIN), smin)
        sl, sh = bf16_round64(smin - smin.abs() * LF_SILU_FP32_REL), bf16_round64(smax + smax.abs() * LF_SILU_FP32_REL)
        c = torch.stack([bf16_round64(y * s) for y in (yl, yh) for s in (sl, sh)])
        lo, hi = c.amin(0), c.amax(0)
        mid = bf16_round64(bf16_round64(a[:, :F]) * bf16_round64(_silu64(bf16_round64(a[:, F:]))))
    elif epi == LF_ROPE_KV:
        nr = (n_heads + n_heads_kv) * hd                                   # q | k rotate, v is stored as rounded
        assert N == nr + n_heads_kv * hd and rope is not None and positions is not None
        tl, th, tc = bf16_round64(al), bf16_round64(ah), bf16_round64(a)
        tab = rope[positions.long()]                                       # [rows][hd / 2][2]
        j = torch.arange(nr // 2) % (hd // 2)
        cs, sn = tab[:, j, 0].float(), tab[:, j, 1].float()
        lo, hi, mid = tl.clone(), th.clone(), tc.clone()
        rl, rh, il, ih = _rope_corners((tl[:, 0:nr:2], th[:, 0:nr:2]), (tl[:, 1:nr:2], th[:, 1:nr:2]), cs, sn)
        lo[:, 0:nr:2], hi[:, 0:nr:2], lo[:, 1:nr:2], hi[:, 1:nr:2] = rl, rh, il, ih
        rm, _, im, _ = _rope_corners((tc[:, 0:nr:2],), (tc[:, 1:nr:2],), cs, sn)
        mid[:, 0:nr:2], mid[:, 1:nr:2] = rm, im
    else:
        raise ValueError(f"epilogue {epi}")
    return LinearFusedRef(lo, hi, mid, ambiguous, xc)


class LinearFusedCheck(NamedTuple):
    violations: int            # elements outside [lo, hi] (a NaN is outside)
    total: int
    eq_mid: float              # share of outputs bit-equal to the epilogue of the exact sum
    worst: tuple               # (row, column) of the element farthest outside, or farthest from mid when none is outside
    ok: bool

    def line(self, label: str, period: int = 0) -> str:
        r, c = self.worst
        per = f", mod {period} = {c % period}" if period > 0 else ""
        return (f"[linear fused {label}] outside [lo, hi]: {self.violations} of {self.total}; bit-equal to mid {self.eq_mid:.5f}; worst at row {r} "
                f"column {c}: mod 16 = {c % 16}{per}")


def linear_fused_compare(got, ref: LinearFusedRef, label: str = "", period: int = 0, columns=None) -> LinearFusedCheck:
    """lo <= got <= hi on every element (`columns`: a slice of the reference's columns the output holds, e.g. q alone).  Prints one line."""
    g = torch.as_tensor(got).detach().cpu().double()
    lo, hi, mid = (t if columns is None else t[:, columns] for t in (ref.lo, ref.hi, ref.mid))
    if g.shape != lo.shape:
        raise ValueError(f"shapes differ: {tuple(g.shape)} vs {tuple(lo.shape)}")
    inside = (g >= lo) & (g <= hi)
    out = torch.where(torch.isfinite(g), torch.maximum(lo - g, g - hi).clamp(min=0.0), torch.full_like(g, float("inf")))
    score = out if not bool(inside.all()) else (g - mid).abs()
    r, c = divmod(int(score.argmax()), g.shape[1])
    res = LinearFusedCheck(int((~inside).sum()), g.numel(), float((g == mid).double().mean()), (r, c), bool(inside.all()))
    print("\n" + res.line(label, period))
    return res


class LinearCase(NamedTuple):
    """One call of zn_op_linear_fused and the plan it must report (`expect`: pairs of (field of zn_linear_op.plan_dict(), value))."""
    family: str
    pro: int
    epi: int
    rows: int
    N: int
    K: int
    expect: tuple = ()
    prefill: int = 0
    bias: bool = False
    tune: tuple = ()           # ((zn_debug_tune key name, value), ...) in force during the call, restored to (key, 1) after it
    lengths: tuple = ()        # LF_ROPE_KV decode: position of the new token per row
    pf_S: int = 0              # LF_ROPE_KV prefill: positions per cache row, first position
    pf_base: int = 0
    hd: int = 128              # LF_ROPE_KV: which handle (16 / 4 heads of 128 or 32 / 8 heads of 64)
    twice: bool = False        # split-K: run twice in a row, the arrival tickets must be back at zero

    @property
    def label(self) -> str:
        pro, epi = ("none", "ln", "gated")[self.pro], ("store", "resid", "silu", "rope_kv", "f32")[self.epi]
        extra = ("+bias" if self.bias else "") + (" prefill" if self.prefill else "") + (f" hd{self.hd}" if self.epi == LF_ROPE_KV else "") + \
                (f" S{self.pf_S}+{self.pf_base}" if self.pf_S else "") + "".join(f" {k}={v}" for k, v in self.tune)
        return f"{self.family} {pro}x{epi}{extra} rows {self.rows} N {self.N} K {self.K}"


LF_MAX_LEN = 16                # cache capacity of the RoPE + KV-append cases
LF_SEED = 20
_GEMV_KS_NCH = {8: (1, 1), 264: (1, 1), 512: (1, 1), 520: (1, 2), 1024: (1, 2), 2048: (1, 4), 3072: (1, 8), 4096: (4, 2), 8192: (4, 4), 16384: (4, 8)}
_GEMV_LN_NCH = {264: 1, 2048: 4, 4096: 8}        # LayerNorm prologue: whole rows per wave, ks 1


def _gemv_expect(N, K, ks, nch):
    # target_blocks 4: N = 72 (36 units), 64 and 96 (SiLU: 32 and 48) divide over the grid exactly; 73 is odd, 74 leaves a unit tail
    return (("kernel", "GEMV"), ("ks", ks), ("nch", nch), ("full", int(K == ks * nch * 512 and N in (64, 72, 96))))


def linear_cases_gemv(K: int) -> list:
    """rows 1..4 (groups of 2 and 4 rows, each mask-free only when full), grid of 4 workgroups."""
    ks, nch = _GEMV_KS_NCH[K]
    out = []
    for rows in (1, 2, 3, 4):
        for N in (72, 73, 74):
            ex = _gemv_expect(N, K, ks, nch)
            out += [LinearCase("gemv", LF_PRO_NONE, LF_STORE, rows, N, K, ex), LinearCase("gemv", LF_PRO_NONE, LF_STORE, rows, N, K, ex, bias=True),
                    LinearCase("gemv", LF_PRO_NONE, LF_RESID, rows, N, K, ex), LinearCase("gemv", LF_PRO_NONE, LF_F32, rows, N, K, ex)]
        for N in (64, 96):
            out.append(LinearCase("gemv", LF_PRO_NONE, LF_SILU, rows, N, K, _gemv_expect(N, K, ks, nch)))
        if K in _GEMV_LN_NCH:
            for epi, N in ((LF_STORE, 72), (LF_STORE, 73), (LF_RESID, 74), (LF_F32, 73), (LF_SILU, 96)):
                out.append(LinearCase("gemv", LF_PRO_LN, epi, rows, N, K, _gemv_expect(N, K, 1, _GEMV_LN_NCH[K])))
        if K in (2048, 4096):
            for N in (72, 73):
                out.append(LinearCase("gemv", LF_PRO_GATED, LF_STORE, rows, N, K, _gemv_expect(N, K, ks, nch)))
    return out


def linear_cases_rope(hd: int) -> list:
    """Split + RoPE + KV append, N = 3072, K = 2048: the GEMV (rows 1..4, one row each at position 0, 5, capacity - 1 and - nothing is appended -
    capacity), gemm16k_kernel in a decode step (LayerNorm as its prologue, and without) and over the rows of a short prefill."""
    L = LF_MAX_LEN
    gemv_lens = {1: (5,), 2: (L - 1, L), 3: (0, L - 1, L), 4: (0, 5, L - 1, L)}      # the row at capacity comes last: a broken guard would write into the canary row behind it
    out = []
    for pro in (LF_PRO_LN, LF_PRO_NONE):
        for rows in (1, 2, 3, 4):
            out.append(LinearCase("rope", pro, LF_ROPE_KV, rows, 3072, 2048, (("kernel", "GEMV"), ("ks", 1), ("nch", 4), ("full", 1)), lengths=gemv_lens[rows], hd=hd))
        for rows in (5, 16, 17):
            lens = tuple((0, 5, L - 1)[r % 3] if r < rows - 1 else L for r in range(rows))
            out.append(LinearCase("rope", pro, LF_ROPE_KV, rows, 3072, 2048, (("kernel", "GEMM16K"), ("nch", 2), ("ln_pro", int(pro == LF_PRO_LN)), ("ln_launch", 0)),
                                  lengths=lens, hd=hd))
    for rows, S, base in ((17, 17, 7), (34, 17, 0), (48, 24, 7), (64, 32, 0)):
        out.append(LinearCase("rope", LF_PRO_NONE, LF_ROPE_KV, rows, 3072, 2048, (("kernel", "GEMM16K"), ("nch", 2), ("rope_done", 1), ("epi", LF_ROPE_KV)),
                              prefill=1, pf_S=S, pf_base=base, hd=hd))
    return out


def linear_cases_gemm16k() -> list:
    out = []
    for rows in (5, 15, 16, 17):                   # 17: two launches, 16 + 1
        for N in (16, 72):                         # one tile; a clamped edge tile
            for K, nch in ((2048, 2), (4096, 4)):
                ex = (("kernel", "GEMM16K"), ("nch", nch), ("ln_pro", 0), ("ln_launch", 0), ("rows_per_launch", 16))
                for epi in (LF_STORE, LF_RESID, LF_F32):
                    out.append(LinearCase("gemm16k", LF_PRO_NONE, epi, rows, N, K, ex))
                out.append(LinearCase("gemm16k", LF_PRO_LN, LF_STORE, rows, N, K,
                                      (("kernel", "GEMM16K"), ("nch", nch), ("ln_pro", int(K == 2048)), ("ln_launch", int(K == 4096)))))
    return out


def linear_cases_gemm16s() -> list:
    out = []
    shapes = ((96, 256, 2, 3, 1), (7168, 1024, 2, 224, 2), (2048, 8192, 2, 64, 8), (96, 8192, 2, 3, 16), (32736, 256, 4, 512, 1), (16400, 2048, 2, 513, 1))
    for rows in (5, 16):
        for N, K, nwv, groups, ksplit in shapes:
            ex = (("kernel", "GEMM16S"), ("nwv", nwv), ("groups", groups), ("ksplit", ksplit), ("lnp", 0))
            for epi in (LF_STORE, LF_RESID, LF_F32):
                out.append(LinearCase("gemm16s", LF_PRO_NONE, epi, rows, N, K, ex + (("ln_launch", 0),), twice=ksplit > 1))
            Ns = 16416 if N == 16400 else N          # the gate needs N / 2 to be a multiple of 16: 513 groups of 16 value rows
            out.append(LinearCase("gemm16s", LF_PRO_NONE, LF_SILU, rows, Ns, K, ex + (("ln_launch", 0),), twice=ksplit > 1))
            if K <= 4096:                            # LayerNorm as a launch in front
                out.append(LinearCase("gemm16s", LF_PRO_LN, LF_STORE, rows, N, K, ex + (("ln_launch", 1),), twice=ksplit > 1))
    return out


def linear_cases_gemm16() -> list:
    out = []
    for rows in (5, 16):
        for N, K, nw, tile8, blocks, Ns, nws, bs in ((96, 128, 4, 1, 12, 96, 4, 3), (100, 384, 4, 0, 7, 96, 4, 3), (1000, 512, 8, 1, 125, 992, 8, 31),
                                                     (7168, 512, 4, 0, 448, 7168, 8, 224)):
            ex = (("kernel", "GEMM16"), ("nw", nw), ("tile8", tile8), ("blocks", blocks))
            for epi in (LF_STORE, LF_RESID, LF_F32):
                out.append(LinearCase("gemm16", LF_PRO_NONE, epi, rows, N, K, ex))
            out.append(LinearCase("gemm16", LF_PRO_NONE, LF_SILU, rows, Ns, K, (("kernel", "GEMM16"), ("nw", nws), ("tile8", 0), ("blocks", bs))))
        t = (("ZN_TUNE_SMALL_M_LDS", 1),)            # the LDS-staged kernels off: shapes they would take
        for N, K, nw, tile8, blocks, Ns, bs in ((96, 8192, 16, 1, 12, 96, 3), (4104, 256, 4, 0, 257, 8224, 257)):
            ex = (("kernel", "GEMM16"), ("nw", nw), ("tile8", tile8), ("blocks", blocks))
            for epi in (LF_STORE, LF_RESID, LF_F32):
                out.append(LinearCase("gemm16", LF_PRO_NONE, epi, rows, N, K, ex, tune=t))
            out.append(LinearCase("gemm16", LF_PRO_NONE, LF_SILU, rows, Ns, K, (("kernel", "GEMM16"), ("nw", nw), ("tile8", 0), ("blocks", bs)), tune=t))
    return out


def linear_cases_prefill() -> list:
    out = []
    for rows in (17, 33, 64):                      # gemm64s_kernel; what it does not serve (a gate of 48 or 80 or 100 rows, K = 160) goes to the tiled GEMM
        for N, K, ksplit in ((96, 256, 1), (96, 8192, 16), (128, 256, 1), (128, 8192, 16)):
            ex = (("kernel", "GEMM64S"), ("groups", 2), ("ksplit", ksplit))
            for epi in (LF_STORE, LF_RESID) + ((LF_SILU,) if N == 128 else ()):
                out.append(LinearCase("prefill", LF_PRO_NONE, epi, rows, N, K, ex, prefill=1, twice=ksplit > 1))
        for N, K in ((160, 256), (200, 160)):
            out.append(LinearCase("prefill", LF_PRO_NONE, LF_SILU, rows, N, K, (("kernel", "GEMM_TILED"),), prefill=1))
    for rows in (65, 129, 257):                    # the tiled GEMM: direct fragments, and (from 256 rows, K a multiple of 64) LDS-staged panels
        for N, K in ((96, 256), (160, 256), (200, 160)):
            for epi in (LF_STORE, LF_RESID, LF_SILU):
                out.append(LinearCase("prefill", LF_PRO_NONE, epi, rows, N, K, (("kernel", "GEMM_TILED"),), prefill=1))
        out.append(LinearCase("prefill", LF_PRO_NONE, LF_RESID, rows, 96, 8192, (("kernel", "GEMM_TILED"),), prefill=1))
    return out


LF_PAIR_ROWS = (5, 10, 16, 24)
# fc1 behind the projection that leaves LayerNorm statistics: (N, nwv, groups, ksplit) at K = 2048
LF_PAIR_FC1 = ((2560, 2, 80, 4), (2592, 2, 81, 4), (10240, 2, 320, 2), (16384, 2, 512, 1), (32736, 4, 512, 1))


def linear_cases_pair(rows: int, N: int, k_out: int = 2048, launch: bool = False) -> tuple:
    """(out, fc1): out_proj + residual at N = 2048 leaving statistics, then LayerNorm x SiLU gate normalising from them - or, `launch`
    (ZN_TUNE_FC1_LN_LAUNCH = 2), nothing handed over and layernorm_kernel in front of fc1."""
    nwv, groups, ksplit = next(t[1:] for t in LF_PAIR_FC1 if t[0] == N)
    t = (("ZN_TUNE_FC1_LN_LAUNCH", 2),) if launch else ()
    out = LinearCase("pair.out", LF_PRO_NONE, LF_RESID, rows, 2048, k_out,
                     (("kernel", "GEMM16K"), ("nch", k_out // 1024), ("writes_ln_stats", int(not launch))), tune=t)
    fc1 = LinearCase("pair.fc1", LF_PRO_LN, LF_SILU, rows, N, 2048,
                     (("kernel", "GEMM16S"), ("nwv", nwv), ("groups", groups), ("ksplit", ksplit), ("lnp", int(not launch)), ("reads_ln_stats", int(not launch)),
                      ("ln_launch", int(launch))), tune=t, twice=ksplit > 1)
    return out, fc1


_LF_W_CACHE: dict = {}
# Seeds of the activation tensors whose default-seed draw left more than LF_AMBIGUOUS_CAP of some row at a bf16 rounding boundary of its LayerNorm
# (found on the CPU by tests/test_linear_compare_cpu.py's condition; the cap itself never moves)
LF_SEEDS: dict = {"x.3.264": 22, "x.3.4096": 21, "gv.4.4096": 21, "x.5.2048": 21, "x.16.2048": 23, "x.17.2048": 23, "x.15.2048": 22, "x.17.4096": 21,
                  "x.5.256": 21, "x.16.256": 28, "x.16.1024": 26,
                  # the residual rows of the statistics pair (fc1 normalises out_proj's output)
                  "res.pair.out.5.4096": 21, "res.pair.out.10.2048": 23, "res.pair.out.10.4096": 21, "res.pair.out.16.2048": 21, "res.pair.out.16.4096": 25,
                  "res.pair.out.24.2048": 25, "res.pair.out.24.4096": 57}


def lf_seed(tag: str) -> int:
    return LF_SEEDS.get(tag, LF_SEED)


def linear_case_tensors(c: LinearCase, x=None) -> dict:
    """The CPU operands of a case, from synth with fixed tags: weights U(-1/sqrt(K), 1/sqrt(K)), activation rows of different mean and scale
    (as in test_fc1_layernorm_from_handed_over_statistics).  `x`: the activations to use instead (fc1 behind a real out_proj)."""
    key = (c.N, c.K)
    if key not in _LF_W_CACHE:
        _LF_W_CACHE[key] = torch.from_numpy(synth.uniform(LF_SEED, f"lf.w.{c.N}.{c.K}", (c.N, c.K), 1.0 / float(np.sqrt(c.K)))).to(torch.bfloat16)
    t = {"W": _LF_W_CACHE[key]}
    # rows of different scale (0.5 .. 3) and mean (-1 .. 1 of the row's scale: more would only grow the fp32 LayerNorm's own cancellation error, and
    # with it the share of activations that may round either way)
    scale = torch.linspace(0.5, 3.0, c.rows)[:, None]
    shift = scale * torch.linspace(-1.0, 1.0, c.rows)[:, None]
    if c.pro == LF_PRO_GATED:
        t["gv"] = (torch.from_numpy(synth.normal(lf_seed(f"gv.{c.rows}.{c.K}"), f"lf.gv.{c.rows}.{c.K}", (c.rows, c.K))) * scale).contiguous()
    elif x is not None:
        t["x"] = x
    else:
        t["x"] = (torch.from_numpy(synth.normal(lf_seed(f"x.{c.rows}.{c.K}"), f"lf.x.{c.rows}.{c.K}", (c.rows, c.K))) * scale + shift).to(torch.bfloat16)
    if c.pro != LF_PRO_NONE:
        t["ln_w"] = (1.0 + torch.from_numpy(synth.uniform(LF_SEED, f"lf.lnw.{c.K}", (c.K,), 0.3))).to(torch.bfloat16)
    if c.pro == LF_PRO_LN:
        t["ln_b"] = torch.from_numpy(synth.uniform(LF_SEED, f"lf.lnb.{c.K}", (c.K,), 0.2)).to(torch.bfloat16)
    if c.bias:
        t["bias"] = torch.from_numpy(synth.uniform(LF_SEED, f"lf.bias.{c.N}", (c.N,), 0.5)).to(torch.bfloat16)
    if c.epi == LF_RESID:
        res = torch.from_numpy(synth.normal(lf_seed(f"res.{c.family}.{c.rows}.{c.K}"), f"lf.res.{c.rows}.{c.N}", (c.rows, c.N)))
        if c.family == "pair.out":                   # the residual stream fc1 then normalises: rows of different mean and scale here too
            res = res * scale + shift
        t["resid"] = res.to(torch.bfloat16)
    return t


def linear_case_positions(c: LinearCase):
    """LF_ROPE_KV: (cache row, position) of every activation row."""
    if c.prefill:
        m = torch.arange(c.rows)
        return m // c.pf_S, c.pf_base + m % c.pf_S
    return torch.arange(c.rows), torch.tensor(c.lengths, dtype=torch.long)


def linear_case_reference(c: LinearCase, t: dict, eps: float, rope=None, rope_positions: int = 0) -> LinearFusedRef:
    kw = {}
    if c.epi == LF_ROPE_KV:
        _, pos = linear_case_positions(c)
        kw = dict(rope=rope, positions=pos.clamp(max=rope_positions - 1), hd=c.hd, n_heads=2048 // c.hd, n_heads_kv=512 // c.hd)
    return linear_fused_reference(c.pro, c.epi, t["W"], x=t.get("x"), ln_w=t.get("ln_w"), ln_b=t.get("ln_b"), gv=t.get("gv"), bias=t.get("bias"),
                                  resid=t.get("resid"), eps=eps, **kw)
