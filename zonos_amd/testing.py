"""Helpers shared by tests, bench.py and smoke(): build a `Zonos` around synthetic weights (zonos_amd/synth.py)."""
from __future__ import annotations

from typing import NamedTuple

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
