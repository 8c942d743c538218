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


# ------------------------------------------------------------------ attention: float64 interval reference, comparator, fp32 restatement, case tables
# Decode and prefill attention against float64 arithmetic on the bf16 operands.  As for the fused linears the bar is an interval per output
# element with bf16 ends (bf16_round64 is monotone: lo <= got <= hi is an exact test and no element is exempt).  With the true weights
# w_t = softmax_t((q.k_t) scale) over the visible keys, exact_d = sum_t w_t v_td and A_d = sum_t w_t |v_td|, every kernel here computes
#   out_d = fl(N_d * fl(1 / l)),   N_d = sum_t c_t P_t v_td (fp32, some order),   l = sum_t c_t e_t (fp32, some order),
# where e_t = exp~(fl(s~_t - m)) with m the running maximum through the key's 512-key block, P_t = bf16(e_t) and c_t the product of the later
# blocks' rescales f_j = exp(m_{j-1} - m_j).  c_t multiplies numerator and denominator alike and exp(-m) is common to all keys, so neither the
# error of f_j nor the choice of m reaches the quotient: out_d = sum_t w_t rho_t v_td with every rho_t inside [1 / (1 + Theta), 1 + Theta], hence
# |out_d - exact_d| <= Theta A_d.  Theta is assembled from these terms and nothing else (u = 2^-24, the unit roundoff of fp32):
#   eps       score error, absolute: bf16 x bf16 products are exact in fp32; their fp32 sum in any order (fma chain, matrix cores) costs LF_SUM_BOUND
#             per term over hd terms of sum_i |q_i k_ti|, the scale multiply and fl32(1 / sqrt(hd)) one rounding each (2 u |s_t|).  It enters a
#             weight as e^{+-2 eps}: once through the numerator, once through the denominator.
#   AT_SUB    rounding of s - m: u |s - m| with |s - m| <= -ln(FLT_MIN) + 1 on the keys that count (below), again twice.
#   eta       AT_FEXP_ETA, the relative error of the exponential: the one term IEEE does not give.  zn_fexp_u20 is restated in numpy below
#             (fexp_u20_np) and measured against float64 exp on a dense grid (fexp_u20_max_rel_error); libm's expf (<= 1 ulp) is far inside it.
#   AT_BF16   P = bf16(e): 2^-8, half an ulp of an 8-bit significand (at most; 2^-9 is the error at the top of a binade).  The dominant term.
#             The row sum takes the unrounded e, so it appears once.
#   gamma     fp32 sums of L terms (row sum: positive terms; P.V: against sum |P v|) at LF_SUM_BOUND per term, plus one multiply and one add per
#             512-key block for the recurrence acc = acc f_j + pv_j (2 u per block), for numerator and denominator each.
#   2 u + u   the reciprocal (<= 1 ulp) and the final multiply; the final bf16 rounding is applied to the interval's ends.
#   Theta = e^{2 (eps + AT_SUB)} (1 + eta) (1 + AT_BF16) (1 + gamma) (1 + 2 u) (1 + u) / ((1 - eta) (1 - gamma)) - 1.
# Absolute term: a key with s_t - max_t s_t < ln(FLT_MIN) + AT_DEAD_MARGIN may be flushed to zero (fexp_u20 returns 0 below ln(FLT_MIN); a product
# with an underflowing f_j loses its precision), or be kept: its whole weight, (1 + Theta) sum_dead w_t |v_td|, is added, and FLT_MIN L max|v| for
# arithmetic in the subnormal range.  The margin of 1 covers eps (the reference refuses eps >= 0.5).
AT_U = 2.0 ** -24
AT_BF16 = 2.0 ** -8
AT_LN_FLT_MIN = float(np.log(np.float64(np.finfo(np.float32).tiny)))       # -87.3365...
AT_DEAD_MARGIN = 1.0
AT_SUB = AT_U * (AT_DEAD_MARGIN - AT_LN_FLT_MIN)
# max |fexp_u20_np(x) / exp(x) - 1| over fexp_u20_grid() measures AT_FEXP_MEASURED (tests/test_attention_compare_cpu.py measures it again and prints it);
# the constant is the next power of two above it.
AT_FEXP_MEASURED = 1.1243e-4                                               # at x = -36.0435, over 4 207 519 fp32 arguments
AT_FEXP_ETA = 2.0 ** -13                                                   # 1.2207e-4
_FEXP_LOW = np.uint32(0xc2aeac50).view(np.float32)                         # ln(FLT_MIN) as zn_fexp_u20 spells it


def fexp_u20_np(x) -> np.ndarray:
    """zn_fexp_u20 (zonos_amd/csrc/zn_common.h) in numpy: float32 operations, a truncating cast.  An fma is the float64 product (exact: 24 x 24
    bits) plus the addend, rounded to float64 and then to float32 - a double rounding that can differ from the fused one by an ulp of float32
    on rare inputs, five orders below the error measured here."""
    x = np.asarray(x, dtype=np.float32)
    fma = lambda a, b, c: (a.astype(np.float64) * np.float64(b) + np.float64(c)).astype(np.float32)
    log2e = np.uint32(0x3fb8aa3b).view(np.float32)
    c0, c1 = np.float32(0.00010703434948458272), np.float32(0.30354260500649682)
    c2, c3 = np.float32(-0.22433836478672356), np.float32(-0.079204240219773236)
    ok = x >= _FEXP_LOW                                                     # false for NaN too
    src = np.where(ok, x, np.float32(0.0)) * log2e
    frac = src - np.floor(src)
    r = fma(frac, c3, c2)
    r = fma(frac, r.astype(np.float64), c1)
    r = fma(frac, r.astype(np.float64), c0)
    src = src - r
    tmp = (np.float64(8388608.0) * src.astype(np.float64) + np.float64(1065353216.0)).astype(np.float32)
    i = np.clip(np.trunc(tmp), -2147483648.0, 2147483520.0).astype(np.int32)   # (the conversion saturates; arguments in [ln(FLT_MIN), 0] never get there)
    return np.where(ok, i, np.int32(0)).astype(np.int32).view(np.float32)


def fexp_u20_grid() -> np.ndarray:
    """Every fp32 value of a dense grid on [ln(FLT_MIN), 0]: 2^22 equally spaced points, and 64 consecutive fp32 values on either side of every
    multiple of ln 2 (where the polynomial's argument wraps)."""
    g = np.linspace(float(_FEXP_LOW), 0.0, 1 << 22).astype(np.float32)
    k = (np.arange(0, 127, dtype=np.float64) * -np.log(2.0)).astype(np.float32)
    k = k[k >= _FEXP_LOW]
    near = (k.view(np.int32)[:, None] + np.arange(-64, 65, dtype=np.int32)[None, :]).reshape(-1).view(np.float32)
    near = near[(near >= _FEXP_LOW) & (near <= 0)]
    return np.unique(np.concatenate([g, near, np.array([_FEXP_LOW, 0.0], dtype=np.float32)]))


def fexp_u20_max_rel_error() -> tuple:
    """(max relative deviation of fexp_u20_np from float64 exp over fexp_u20_grid(), the argument where it occurs, grid size)."""
    x = fexp_u20_grid()
    d = np.abs(fexp_u20_np(x).astype(np.float64) / np.exp(x.astype(np.float64)) - 1.0)
    i = int(d.argmax())
    return float(d[i]), float(x[i]), int(x.size)


class AttentionRef(NamedTuple):
    lo: torch.Tensor           # float64 tensors [R][Hq][Sq][hd]; lo and hi hold bf16 values
    hi: torch.Tensor
    exact: torch.Tensor
    weight_abs: torch.Tensor   # A_d = sum_t w_t |v_td|
    theta: torch.Tensor        # [R][Hq][Sq]
    valid: torch.Tensor        # bool [R][Sq]: the query sees at least one key (others are not compared)
    wmax: torch.Tensor         # [R][Hq][Sq] largest weight and its key: what the spotlight cases assert
    tmax: torch.Tensor


def attention_reference(q, k, v, scale: float, visible) -> AttentionRef:
    """q bf16 [R][Hq][Sq][hd], k and v bf16 [R][Hkv][T][hd], visible bool [R][Sq][T] (the same for every head).  Keys no query of the row sees
    may hold anything (NaN patterns): they are never touched."""
    R, Hq, Sq, hd = q.shape
    Hkv, T = k.shape[1], k.shape[2]
    G = Hq // Hkv
    lo, hi, exact, wabs = (torch.zeros(R, Hq, Sq, hd, dtype=torch.float64) for _ in range(4))
    theta, wmax = torch.zeros(R, Hq, Sq, dtype=torch.float64), torch.zeros(R, Hq, Sq, dtype=torch.float64)
    tmax = torch.zeros(R, Hq, Sq, dtype=torch.long)
    valid = visible.any(-1)
    for r in range(R):
        vis = visible[r]                                                    # [Sq][T]
        seen = vis.any(0)
        n = int(seen.nonzero().max()) + 1 if bool(seen.any()) else 1        # keys past the last visible one are left out altogether
        vis, seen = vis[:, :n], seen[:n]
        kk = torch.where(seen[None, :, None], k[r, :, :n].double(), torch.zeros((), dtype=torch.float64)).repeat_interleave(G, 0)
        vv = torch.where(seen[None, :, None], v[r, :, :n].double(), torch.zeros((), dtype=torch.float64)).repeat_interleave(G, 0)
        qq = q[r].double()
        s = torch.einsum("hsd,htd->hst", qq, kk) * scale
        sabs = torch.einsum("hsd,htd->hst", qq.abs(), kk.abs()) * scale
        eps = torch.where(vis[None], hd * LF_SUM_BOUND * sabs + 2 * AT_U * s.abs(), torch.zeros((), dtype=torch.float64)).amax(-1)
        if float(eps.max()) >= 0.5:
            raise ValueError(f"score error bound {float(eps.max()):.3g} >= 0.5: the dead-key margin does not cover it")
        sm = torch.where(vis[None], s, torch.full((), float("-inf"), dtype=torch.float64))
        M = sm.amax(-1, keepdim=True)
        M = torch.where(torch.isfinite(M), M, torch.zeros_like(M))          # a query without keys: weights 0, not compared
        e = torch.exp(sm - M)
        w = e / e.sum(-1, keepdim=True).clamp(min=1e-300)
        dead = vis[None] & (sm - M < AT_LN_FLT_MIN + AT_DEAD_MARGIN)
        ex = torch.einsum("hst,htd->hsd", w, vv)
        A = torch.einsum("hst,htd->hsd", w, vv.abs())
        Ad = torch.einsum("hst,htd->hsd", w * dead, vv.abs())
        L = vis.sum(-1).double()[None]                                      # [1][Sq]
        gamma = LF_SUM_BOUND * L + 2 * AT_U * ((n + 511) // 512)
        th = torch.exp(2 * (eps + AT_SUB)) * (1 + AT_FEXP_ETA) * (1 + AT_BF16) * (1 + gamma) * (1 + 2 * AT_U) * (1 + AT_U) / ((1 - AT_FEXP_ETA) * (1 - gamma)) - 1
        tol = th[..., None] * A + (1 + th[..., None]) * Ad + float(np.finfo(np.float32).tiny) * L[..., None] * vv.abs().amax(1)[:, None, :]
        if not bool(torch.isfinite(ex).all() and torch.isfinite(tol).all()):
            raise ValueError("the float64 reference is not finite")
        lo[r], hi[r], exact[r], wabs[r], theta[r] = bf16_round64(ex - tol), bf16_round64(ex + tol), ex, A, th
        wmax[r], tmax[r] = w.max(-1)
    return AttentionRef(lo, hi, exact, wabs, theta, valid, wmax, tmax)


class AttentionCheck(NamedTuple):
    outside: int               # compared elements outside [lo, hi] (a NaN is outside)
    nonfinite: int             # compared elements that are NaN or Inf
    total: int
    headroom: float            # worst |got - exact| / (Theta A_d): reported, not asserted (the bf16 rounding of the output alone can exceed 1)
    worst: tuple               # (row, head, position, dim) of the element farthest outside, or of the worst headroom
    ok: bool

    def line(self, label: str) -> str:
        r, h, s, d = self.worst
        return (f"[attention {label}] outside [lo, hi]: {self.outside} of {self.total}; non-finite {self.nonfinite}; worst |got - exact| / (Theta A) "
                f"{self.headroom:.3f} at row {r} head {h} position {s} dim {d}")


def attention_compare(got, ref: AttentionRef, label: str = "", quiet: bool = False) -> AttentionCheck:
    """lo <= got <= hi on every element of every query that sees a key; got [R][Hq][Sq][hd].  Prints one line."""
    g = torch.as_tensor(got).detach().cpu().double()
    if g.shape != ref.lo.shape:
        raise ValueError(f"shapes differ: {tuple(g.shape)} vs {tuple(ref.lo.shape)}")
    cmp = ref.valid[:, None, :, None].expand_as(g)
    fin = torch.isfinite(g)
    inside = (g >= ref.lo) & (g <= ref.hi)
    bad = cmp & ~inside
    over = torch.where(fin, torch.maximum(ref.lo - g, g - ref.hi).clamp(min=0.0), torch.full_like(g, float("inf")))
    ratio = (g - ref.exact).abs() / (ref.theta[..., None] * ref.weight_abs).clamp(min=1e-300)
    ratio = torch.where(cmp & fin & (ref.weight_abs > 0), ratio, torch.zeros_like(ratio))
    score = torch.where(cmp, over, torch.zeros_like(over)) if bool(bad.any()) else ratio
    idx = int(score.argmax())
    worst = tuple(int(i) for i in np.unravel_index(idx, tuple(g.shape)))
    res = AttentionCheck(int(bad.sum()), int((cmp & ~fin).sum()), int(cmp.sum()), float(ratio.max()), worst, not bool(bad.any()) and bool((fin | ~cmp).all()))
    if not quiet:
        print("\n" + res.line(label))
    return res


def attention_restatement(q, k, v, scale: float, visible, span=None, mut: str = "") -> torch.Tensor:
    """The kernels' arithmetic in plain fp32 (torch CPU matmuls for the two contractions, in whatever order they sum): 512-key blocks, the running
    maximum, e = fexp_u20 on the first 16 floor(n / 16) keys of the block's span and libm exp on the rest, the row sum of the unrounded e,
    P = bf16(e), the recurrence acc = acc f_j + pv_j, out = bf16(acc (1 / l)).  Keys no query of the row sees are zeroed first, as the kernels do.
    span int [R][Sq]: keys the reference's query block spans (default: the query's own keys).  Shapes as attention_reference; returns bf16.
    mut: "no_rescale" (f_j = 1), "no_max" (nothing subtracted), "tail_unmasked" (every key of the buffer counts) - tests/test_attention_compare_cpu.py."""
    R, Hq, Sq, hd = q.shape
    Hkv, T = k.shape[1], k.shape[2]
    G = Hq // Hkv
    out = torch.full((R, Hq, Sq, hd), float("nan"), dtype=torch.bfloat16)
    sc32 = torch.tensor(np.float32(scale))
    ninf = torch.full((), float("-inf"))
    for r in range(R):
        vis = visible[r] if mut != "tail_unmasked" else torch.ones_like(visible[r])
        seen = vis.any(0)
        n = int(seen.nonzero().max()) + 1 if bool(seen.any()) else 1
        vis, seen = vis[:, :n], seen[:n]
        kk = torch.where(seen[None, :, None], k[r, :, :n].float(), torch.zeros(())).repeat_interleave(G, 0)
        vv = torch.where(seen[None, :, None], v[r, :, :n].float(), torch.zeros(())).repeat_interleave(G, 0)
        s = torch.matmul(q[r].float(), kk.transpose(1, 2)) * sc32           # [Hq][Sq][n]
        Lq = vis.sum(-1)
        E = torch.maximum(span[r], Lq) if span is not None else Lq
        m = torch.full((Hq, Sq), float("-inf"))
        acc, l = torch.zeros(Hq, Sq, hd), torch.zeros(Hq, Sq)
        for t0 in range(0, n, 512):
            t1 = min(n, t0 + 512)
            vb, sb = vis[None, :, t0:t1], s[:, :, t0:t1]
            mj = torch.maximum(m, torch.where(vb, sb, ninf).amax(-1))
            if mut == "no_max":
                mj = torch.zeros_like(mj)
            f = torch.exp(m - mj) if t0 > 0 else torch.zeros_like(mj)
            f = torch.where(torch.isfinite(mj) & torch.isfinite(m), f, torch.zeros_like(f)) if t0 > 0 else f
            if mut == "no_rescale" and t0 > 0:
                f = torch.ones_like(f)
            x = torch.where(vb, sb - torch.where(torch.isfinite(mj), mj, torch.zeros_like(mj))[..., None], torch.zeros(()))
            nvec = (E - t0).clamp(min=0, max=512) & ~15                     # [Sq]
            fast = torch.arange(t1 - t0)[None, :] < nvec[:, None]
            e = torch.where(fast[None], torch.from_numpy(fexp_u20_np(x.numpy())), torch.exp(x))
            e = torch.where(vb, e, torch.zeros(()))
            acc = acc * f[..., None] + torch.matmul(e.to(torch.bfloat16).float(), vv[:, t0:t1])
            l = l * f + e.sum(-1)
            m = mj
        out[r] = (acc * (1.0 / l)[..., None]).to(torch.bfloat16)
    return out


# ---- inputs.  Three families: "diffuse" (N(0, 1) q, K, V: every weight about 1 / L), "spot" (one key per (row, head) - per (row, position) in
# prefill - is c q / |q| with its scaled score at AT_SPOT_SCORE, so it holds more than half of the weight; its V row is a positive ramp, distinct
# by position, against V rows of the other sign; the first key PAST the context is a stronger spotlight still, had it been visible), and the
# range cases "rise" / "fall" / "tie" (q and K along one direction per kv head: scaled scores run from -100 to 100 over the cache, so that every
# block rescale f_j is below 1e-20 and the earlier blocks vanish, or from 100 to -100, f_j = 1 and the later blocks flush to zero, or hold their
# maximum of 60 twice, on keys 511 and 512 with the same K row).
AT_TAILS = ("zeros", "random", "0x7FC0", "0xFFFF", "0x7F80", "0xFF80")      # what the keys at or past a row's context hold, in turn
AT_SEED = 40
AT_SEEDS: dict = {}            # tag -> seed, for an operand whose default draw left a spotlight below half of the weight (none needed so far)
AT_SPOT_SCORE, AT_NEXT_SCORE = 20.0, 30.0
AT_EDGES = (0, 15, 16, 63, 64, 127, 128, 511, 512, 513, 1023, 1024)
# (head size, group) -> (query heads, kv heads) of the single-layer model that serves it (d_model = query heads x head size)
AT_GEOM = {(128, 1): (2, 2), (128, 2): (4, 2), (128, 4): (8, 2), (128, 8): (8, 1), (64, 4): (8, 2), (64, 2): (4, 2), (32, 4): (8, 2), (32, 8): (8, 1)}
AT_LENS_512 = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 511, 512, 300, 2, 449, 512)
AT_LENS_1032 = (1, 16, 17, 64, 65, 128, 129, 511, 512, 513, 1023, 1024, 1025, 1032, 700, 3)      # 1032: a multiple of 8, not of 64


class AttnCase(NamedTuple):
    name: str
    kind: str                  # "decode" (zn_op_attn_decode) | "prefill" (zn_op_attn_prefill_rows)
    family: str                # diffuse | spot | spot_next | rise | fall | tie
    hd: int
    G: int
    cap: int                   # cache capacity (max_len)
    lens: tuple = ()           # decode: keys per row; prefill with `ragged`: row_len per row
    rows: int = 0              # prefill
    S: int = 0
    base: int = 0
    ragged: bool = False
    tune: tuple = ()           # ((zn_debug_tune key name, value), ...) in force during the call
    ext: str = "null"          # decode: ext = NULL | "L" | "split" (L rounded up to the query split) | "short" (below L: the bits of NULL)
    kernel: str = ""           # the kernel template (and branch) the case is there for

    @property
    def R(self) -> int:
        return len(self.lens) if self.kind == "decode" else self.rows

    @property
    def heads(self) -> tuple:
        return AT_GEOM[(self.hd, self.G)]


def at_qsplit(S: int) -> int:
    """Query split of the reference's CPU flash kernel for a sequence of S positions."""
    return 256 if S >= 768 else 64 if S >= 192 else 32


def _at_pick(lens: tuple, rows: int) -> tuple:
    """`rows` of the 16 contexts; between them the row counts of a capacity walk all 16."""
    return {16: lens, 6: lens[10:16], 5: lens[5:10], 4: lens[0:4], 2: (lens[11], lens[4]), 1: (lens[12],)}[rows]


def attention_cases_decode() -> list:
    out = []
    fam = {16: "spot", 6: "diffuse", 5: "spot", 4: "diffuse", 2: "spot", 1: "diffuse"}

    def shape(hd, G, rows, cap, tune=()):
        t = dict(tune)
        fused = cap <= min(512, t.get("ZN_TUNE_ATTN_FUSED_MAX_KEYS", 512))
        sc = hd == 128 and (t.get("ZN_TUNE_ATTN_SPLIT_COLS") == 2 or (t.get("ZN_TUNE_ATTN_SPLIT_COLS") != 1 and rows > 4))
        ds = (4 if fused else 2) if sc else 1
        k = f"attn_block_kernel<{hd},{G},{'fused' if fused else 'split'},DS{ds}>" + ("" if fused else f" + attn_scores_kernel<{hd},{G}>")
        if fused and ds > 1:
            k += " remap" if rows * AT_GEOM[(hd, G)][1] % 8 == 0 else " no-remap"
        return k
    for cap, lens in ((512, AT_LENS_512), (520, AT_LENS_512), (1032, AT_LENS_1032)):
        for rows in (1, 2, 4, 5, 6, 16):
            out.append(AttnCase(f"d128g4 r{rows} cap{cap}", "decode", fam[rows], 128, 4, cap, _at_pick(lens, rows), kernel=shape(128, 4, rows, cap)))
        for rows, mode in ((4, 2), (2, 2), (16, 1)):
            tune = (("ZN_TUNE_ATTN_SPLIT_COLS", mode),)
            out.append(AttnCase(f"d128g4 r{rows} cap{cap} split_cols={mode}", "decode", "spot", 128, 4, cap, _at_pick(lens, rows), tune=tune,
                                kernel=shape(128, 4, rows, cap, tune)))
    for rows in (2, 5):
        tune = (("ZN_TUNE_ATTN_FUSED_MAX_KEYS", 1),)
        out.append(AttnCase(f"d128g4 r{rows} cap512 fused_max=1", "decode", "spot", 128, 4, 512, _at_pick(AT_LENS_512, rows), tune=tune,
                            kernel=shape(128, 4, rows, 512, tune)))
    for hd, G in ((128, 1), (128, 2), (128, 8), (64, 4), (64, 2), (32, 4), (32, 8)):
        for rows in (2, 5):
            for cap, lens in ((512, AT_LENS_512), (1032, AT_LENS_1032)):
                out.append(AttnCase(f"d{hd}g{G} r{rows} cap{cap}", "decode", "spot" if rows == 2 else "diffuse", hd, G, cap, _at_pick(lens, rows),
                                    kernel=shape(hd, G, rows, cap)))
    for family in ("rise", "fall", "tie"):
        out.append(AttnCase(f"d128g4 {family} cap1536", "decode", family, 128, 4, 1536, (1536, 1300), kernel=shape(128, 4, 2, 1536)))
    out.append(AttnCase("d128g4 fall cap512", "decode", "fall", 128, 4, 512, (512, 400), kernel=shape(128, 4, 2, 512)))
    out.append(AttnCase("d64g4 rise cap1536", "decode", "rise", 64, 4, 1536, (1536, 1300), kernel=shape(64, 4, 2, 1536)))
    for cap in (4096, 4608, 8192, 8704, 16384):          # the ticketed combine at nb = 8, 9, 16, 17, 32
        out.append(AttnCase(f"d128g4 r2 cap{cap} nb{(cap + 511) // 512}", "decode", "spot", 128, 4, cap, (cap, cap - 700), kernel=shape(128, 4, 2, cap)))
    for cap, lens in ((512, (300, 77)), (1032, (1000, 700))):
        for ext in ("L", "split", "short"):
            out.append(AttnCase(f"d128g4 r2 cap{cap} ext={ext}", "decode", "spot", 128, 4, cap, lens, ext=ext, kernel=shape(128, 4, 2, cap)))
    return out


def attention_cases_prefill() -> list:
    out = []
    configs = [("mfma", 128, G) for G in (1, 2, 4, 8)] + [("valu", 128, G) for G in (1, 2, 4, 8)] + [("valu", 64, 4), ("valu", 64, 2), ("valu", 32, 4), ("valu", 32, 8)]
    for kern, hd, G in configs:
        tune = (("ZN_TUNE_PREFILL_ATTN_VALU", 2 if kern == "valu" else 1),)
        kname = f"attn_prefill_mfma_kernel<{G}>" if kern == "mfma" else f"attn_prefill_kernel<{hd},{G}>"
        mk = lambda family, S, rows=2, base=0, lens=(), ragged=False: AttnCase(
            f"p{hd}g{G} {kern} {family} S{S}" + (f"+{base}" if base else "") + (" ragged" if ragged else ""), "prefill", family, hd, G, base + S + 3, lens, rows, S, base,
            ragged, tune, kernel=kname)
        TQ = 64 // G
        for i, S in enumerate(sorted({1, TQ - 1, TQ, TQ + 1} - {0})):
            out.append(mk(("spot", "diffuse", "spot_next", "spot")[i % 4], S))
        out.append(mk("spot", TQ + 5, rows=4, lens=(1, TQ, TQ + 1, TQ + 5), ragged=True))
        out.append(mk("spot_next", 513, rows=1))
        if (hd, G) in ((128, 4), (64, 4)):
            for S, family in ((191, "spot"), (192, "diffuse"), (512, "spot"), (767, "spot_next"), (768, "spot")):
                out.append(mk(family, S, rows=1))
            for base in (5, 500, 511):
                out.append(mk("spot", 20, base=base))
            for family in ("rise", "fall", "tie"):
                out.append(mk(family, 600, rows=1))
    mf = (("ZN_TUNE_PREFILL_ATTN_VALU", 1),)
    out.append(AttnCase("p128g4 mfma spot S1025", "prefill", "spot", 128, 4, 1028, (), 1, 1025, 0, False, mf, kernel="attn_prefill_mfma_kernel<4>"))
    return out


def at_seed(tag: str) -> int:
    return AT_SEEDS.get(tag, AT_SEED)


def _at_normal(tag: str, shape) -> torch.Tensor:
    return torch.from_numpy(synth.normal(at_seed(tag), "at." + tag, shape))


def attention_case_tensors(c: AttnCase) -> dict:
    """CPU operands of a case.  q bf16 [R][Hq][Sq][hd]; k, v bf16 [R][Hkv][cap][hd] with finite data everywhere (the "random" tail); visible bool
    [R][Sq][cap]; span int [R][Sq]: keys the reference's query block spans; ext (decode): int [R] or None; start int [R]: first cache position of
    the tail; spots: (row, head, position, key) of every query whose largest weight must be >= 0.5 and sit on that key."""
    hq, hkv = c.heads
    G, hd, R, cap = c.G, c.hd, c.R, c.cap
    Sq = 1 if c.kind == "decode" else c.S
    scale = 1.0 / float(np.sqrt(hd))
    tag = f"{c.kind}.{c.family}.{hd}.{hq}.{hkv}.{R}.{Sq}.{cap}"
    q, k, v = _at_normal("q." + tag, (R, hq, Sq, hd)), _at_normal("k." + tag, (R, hkv, cap, hd)), _at_normal("v." + tag, (R, hkv, cap, hd))
    tt = torch.arange(cap)
    if c.kind == "decode":
        L = torch.tensor(c.lens)
        visible = (tt[None, None, :] < L[:, None, None])
        start, pos0 = L.clone(), L - 1                                     # pos0: cache position of query 0
    else:
        Sv = torch.tensor(c.lens) if c.ragged else torch.full((R,), c.S)
        ss = torch.arange(Sq)
        visible = (tt[None, None, :] <= c.base + ss[None, :, None]) & (ss[None, :, None] < Sv[:, None, None])
        start, pos0 = c.base + Sv, torch.full((R,), c.base)
    spots = []
    ramp = lambda t: (1.0 + torch.arange(hd) / hd) * (1.0 + (t % 7) / 8.0)
    if c.family in ("rise", "fall", "tie"):
        d = _at_normal("dir." + tag, (R, hkv, 1, hd))
        d = d / d.norm(dim=-1, keepdim=True)
        if c.family == "tie":
            a = 2.0 * _at_normal("a." + tag, (R, hkv, cap, 1))
            a[:, :, 511:513] = 60.0
        else:
            a = (-100.0 + 200.0 * tt / max(cap - 1, 1)).view(1, 1, cap, 1).expand(R, hkv, cap, 1)
            a = -a if c.family == "fall" else a
        k = d * a + 0.05 * k
        if c.family == "tie":
            k[:, :, 512] = k[:, :, 511]
        gain = (1.0 + 0.1 * (torch.arange(hq) % G)).view(1, hq, 1, 1)
        q = d.repeat_interleave(G, 1) * float(np.sqrt(hd)) * gain + 0.0 * q     # |q| scale = 1: the scaled score of key t is (1 + 0.1 g) a_t
    elif c.family != "diffuse":
        q = q.to(torch.bfloat16).float()
        qn = q / q.norm(dim=-1, keepdim=True)
        cq = lambda r, h, s, score: qn[r, h, s] * (score / (scale * float(q[r, h, s].norm())))
        if c.kind == "decode":
            v = -v.abs()
            for r in range(R):
                Lr = int(c.lens[r])
                edges = sorted({e for e in AT_EDGES if e < Lr} | {Lr - 1})
                for kvh in range(hkv):
                    for g in range(min(G, len(edges))):
                        h = kvh * G + g
                        t = edges[(r * hq + h) % len(edges)] if len(edges) >= G else edges[g]
                        k[r, kvh, t], v[r, kvh, t] = cq(r, h, 0, AT_SPOT_SCORE), ramp(t)
                        spots.append((r, h, 0, t))
                    if Lr < cap:                                           # had it been visible
                        k[r, kvh, Lr], v[r, kvh, Lr] = cq(r, kvh * G, 0, AT_NEXT_SCORE), 4.0 * ramp(Lr)
        else:
            sign = torch.where(tt % 2 == 0, 1.0, -1.0)
            v = torch.stack([ramp(t) for t in range(7)])[tt % 7][None, None] * sign.view(1, 1, cap, 1) + 0.0 * v
            shift = 1 if c.family == "spot_next" else 0                    # spot_next: the key one past a query's own is its spotlight
            for r in range(R):
                for s in range(Sq):
                    t = c.base + s + shift
                    if t >= cap:
                        continue
                    for kvh in range(hkv):
                        h = kvh * G + s % G
                        k[r, kvh, t] = cq(r, h, s, AT_NEXT_SCORE if shift else AT_SPOT_SCORE)
                        if not shift and bool(visible[r, s, t]):
                            spots.append((r, h, s, t))
    q, k, v = q.to(torch.bfloat16), k.to(torch.bfloat16), v.to(torch.bfloat16)
    ext = None
    if c.kind == "decode":
        L = torch.tensor(c.lens)
        qs = torch.tensor([at_qsplit(int(l)) for l in c.lens])
        ext = {"null": None, "L": L, "split": (L + qs - 1) // qs * qs, "short": (L - 5).clamp(min=1)}[c.ext]
        span = (torch.maximum(ext, L) if ext is not None else L)[:, None]
    else:
        qs = torch.tensor([at_qsplit(int(s)) for s in Sv])[:, None]
        ss = torch.arange(Sq)[None, :]
        span = c.base + torch.minimum((ss // qs) * qs + qs, Sv[:, None])
    return dict(q=q, k=k, v=v, visible=visible, span=span, ext=ext, start=start, scale=scale, spots=spots)


def attention_device_layout(c: AttnCase, t: dict) -> tuple:
    """(q, kv) as the ops take them: q [R][Hq hd] (decode) or [R][S][Hq hd], kv [R][cap][2][Hkv][hd]."""
    hq, hkv = c.heads
    q = t["q"][:, :, 0].reshape(c.R, hq * c.hd) if c.kind == "decode" else t["q"].transpose(1, 2).reshape(c.R, c.S, hq * c.hd)
    kv = torch.stack([t["k"], t["v"]], 1).permute(0, 3, 1, 2, 4)
    return q.contiguous(), kv.contiguous()


def attention_apply_tail(c: AttnCase, q, kv, start, tail: str):
    """Fills, in place (on whatever device the tensors live), the cache positions at or past start[r] - and for a ragged prefill the q rows at or
    past row_len[r] - with one of AT_TAILS ("random": what is there)."""
    if tail == "random":
        return
    bits = 0 if tail == "zeros" else int(tail, 16)
    bits = bits - 65536 if bits >= 32768 else bits
    kvi, qi = kv.view(torch.int16), q.view(torch.int16)
    for r in range(c.R):
        kvi[r, int(start[r]):] = bits
        if c.kind == "prefill" and c.ragged:
            qi[r, int(c.lens[r]):] = bits


def attention_from_device_layout(c: AttnCase, out) -> torch.Tensor:
    """out [R][Hq hd] or [R][S][Hq hd] -> [R][Hq][Sq][hd] on the CPU."""
    hq, _ = c.heads
    o = out.detach().cpu()
    return o.view(c.R, hq, 1, c.hd) if c.kind == "decode" else o.view(c.R, c.S, hq, c.hd).transpose(1, 2).contiguous()


# ------------------------------------------------------------------ weight-only FP8 (zonos_amd/quant.py): the inputs the CPU specification and the device kernels are both tested on

FP8_SEED = 41
FP8_MATRIX_SHAPES = ((96, 256), (64, 8192))


def fp8_seeded_matrix(N: int, K: int) -> torch.Tensor:
    """bf16 [N, K]: normal values with a row scale that spans 2^-12 .. 2^12, so that the rows' scale exponents differ and small values of a row
    fall into the codes' subnormal range."""
    w = torch.from_numpy(synth.normal(FP8_SEED, f"fp8.w.{N}.{K}", (N, K)))
    return (w * torch.exp2(torch.linspace(-12.0, 12.0, N))[:, None]).to(torch.bfloat16)


def fp8_adversarial_rows(K: int = 256) -> tuple:
    """(bf16 [rows, K], names): all zero; one non-zero element; amax exactly 448 * 2^j and one bf16 ulp either side of it; values on the
    midpoints of the code grid (ties to even both ways); values in the codes' subnormal range; amax beyond the clamp on both sides."""
    rows, names = [], []

    def add(name, vals):
        r = torch.zeros(K, dtype=torch.float64)
        v = torch.as_tensor(vals, dtype=torch.float64)
        r[: v.numel()] = v
        b = r.to(torch.float32).to(torch.bfloat16)
        assert torch.equal(b.double(), r), f"{name}: a value of the row is not a bf16"
        rows.append(b)
        names.append(name)
    add("zero", [])
    add("one element", [0.0, 0.0, -0.3984375])
    add("negative zero", [-0.0, 0.0, 1.0])
    for j in (-20, 0, 9):
        s = 2.0 ** j
        # 448 = 1.75 * 2^8: the bf16 neighbours are 446 and 450
        add(f"amax 448*2^{j}", [448.0 * s, -224.0 * s, 17.0 * s])
        add(f"amax 446*2^{j}", [-446.0 * s, 224.0 * s, 17.0 * s])
        add(f"amax 450*2^{j}", [450.0 * s, -225.0 * s, 17.0 * s])
    # midpoints of the grid at scale 2^0 (amax 448): in [16, 32) the step is 2 - 17 lies between 16 (even mantissa) and 18 (odd), 19 between
    # 18 and 20, ...; in [1, 2) the step is 1/8; 2^-6 .. : the lowest normal binade; below: subnormal steps of 2^-9, midpoints at odd
    # multiples of 2^-10 (2^-10 itself ties to zero, 3 * 2^-10 up to 2 * 2^-9)
    add("midpoints", [448.0, 17.0, -19.0, 21.0, 23.0, 1.0625, -1.1875, 1.9375, 240.0 + 8.0, -(224.0 + 8.0), 2.0 ** -6 + 2.0 ** -10, 2.0 ** -6 + 3 * 2.0 ** -10,
                      31.0, -31.5, 255.0])
    add("subnormal codes", [448.0, 2.0 ** -10, -(2.0 ** -10), 3 * 2.0 ** -10, 5 * 2.0 ** -10, -7 * 2.0 ** -10, 2.0 ** -9, 2.0 ** -11, 15 * 2.0 ** -10, 2.0 ** -6 - 2.0 ** -10,
                            2.0 ** -7, 1.5 * 2.0 ** -10, 0.75 * 2.0 ** -9, 2.0 ** -30])
    big, tiny = 2.0 ** 120, 2.0 ** -120
    add("beyond the clamp, large", [big, -big * 1.5, 448.0 * 2.0 ** 100, 450.0 * 2.0 ** 100, 2.0 ** 90, 2.0 ** -9 * 2.0 ** 100, 1.0, 1.9921875 * 2.0 ** 127])
    add("beyond the clamp, small", [tiny, -tiny, 2.0 ** -110, 3 * 2.0 ** -110, 2.0 ** -109, -(2.0 ** -108), 2.0 ** -126, 2.0 ** -133])
    return torch.stack(rows), names


def fp8_row_shifts(N: int) -> torch.Tensor:
    """int32 [N] in -3 .. 3: powers of two to scale the rows of a weight matrix by, so that the rows' FP8 scale exponents differ from row to row
    inside a 32-row workgroup, between value row u and gate row N / 2 + u (at the N of linear_cases_gemm16s / LF_PAIR_FC1 / d_ff = 8192), and
    between the last two rows - a kernel that looked a scale up under the wrong row index could not reproduce the bf16 launch."""
    r = torch.arange(N)
    return ((r * 5 + (r >> 4) + (r >> 10)) % 7 - 3).to(torch.int32)
