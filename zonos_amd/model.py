"""`Zonos` — the reference's model surface (zonos/model.py:43-548) over the MI355X HIP path.

Kept API: `Zonos.from_pretrained / from_local / setup_cache / embed_codes / apply_heads / generate`, attributes
`config, backbone, embeddings, fused_heads, autoencoder, device`.  The hot loop (model.py:467-502) runs as one
hipGraph replay per step inside libzonos_hip.so; the host only mirrors the reference's stop-check cadence
(tensor_ops.py:90-103) and the post-processing (model.py:511-539).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import sys
import threading
import json
from typing import Callable, Iterator, NamedTuple, Sequence

import torch
import torch.nn as nn

from . import _lib
from .autoencoder import DACAutoencoder
from .backbone import BACKBONES, HipEngine
from .backbone._hip import attention_options
from .codebook_pattern import revert_delay_pattern
from .conditioning import ConditioningCache, PrefixConditioner, prepare_conditioning_with_cache
from .config import InferenceParams, ZonosConfig
from .quant import KV_CACHE_MODES, KV_FP8_MIN_ROWS
from .rows import (GenCall, GenRequest, Hooks, check_request_shapes, code_rows, draw_seed, finalise_codes, finalise_row, map_codes, row_end_offset,  # noqa: F401
                   sampling_struct as _sampling_struct, stop_check_at)
from .serving import ServeChunk, ServeResult, SlotScheduler, StreamLedger, check_serve_request, release_limit  # noqa: F401
# (finalise_codes, row_end_offset, SlotScheduler, StreamLedger, check_serve_request: not used here, re-exported for tools and tests)
from .session import ServeSession, ServeShape
from .utils import DEFAULT_DEVICE, find_multiple

DEFAULT_BACKBONE_CLS = next(iter(BACKBONES.values()))


class StreamChunk(NamedTuple):
    """One step of `Zonos.stream`: the frames that became final (int64 [1, 9, k], as `generate()` returns them) and the samples they
    completed (float32 [1, 1, m] on the model's device).  k or m may be 0, never both."""
    codes: torch.Tensor
    wav: torch.Tensor


class KvBuffers(NamedTuple):
    """The KV buffers of one generation or session (`Zonos._kv_buffers`): `ip` (its key_value_memory_dict holds the bf16 caches, or nothing where the
    generation keeps codes only), `kv_ptrs` (the pointer array for zn_gen_begin; None: no bf16 cache, NULL there) and `codes` (one uint8 tensor per
    layer for zn_gen_bind_kv_fp8, or None where nothing is rounded)."""
    ip: InferenceParams
    kv_ptrs: object
    codes: list | None


MAX_BATCH_REQUESTS = 64       # utterances of one generate_batch() call: the batch the sampler tail's tables are sized for (ZN_TAIL_MAXB)


def check_requests(requests: Sequence[GenRequest], nq: int, d_model: int, ragged_prefix: bool = False,
                   mixed_guidance: bool = False) -> tuple[bool | None, int | list[int]]:
    """What `generate_batch` refuses before any launch (ValueError); returns (guided, audio prefix length) of the call.  With `ragged_prefix`
    the requests may bring audio prefixes of different lengths, and the second value is the list of their lengths (0 for None).  With
    `mixed_guidance` guided and cfg_scale == 1 requests may share the call: `guided` is then None when both kinds are present, every
    request's conditioning is checked against its own cfg_scale, and the call's rows (one per unguided request, two per guided one) must
    not exceed MAX_BATCH_REQUESTS."""
    n = len(requests)
    if n == 0:
        raise ValueError("generate_batch: no requests")
    if n > MAX_BATCH_REQUESTS:
        raise ValueError(f"generate_batch: {n} requests, one call holds at most {MAX_BATCH_REQUESTS}")
    guided = {float(r.cfg_scale) != 1.0 for r in requests}
    mixed = len(guided) > 1
    if mixed and mixed_guidance:
        rows = sum(2 if float(r.cfg_scale) != 1.0 else 1 for r in requests)
        if rows > MAX_BATCH_REQUESTS:
            raise ValueError(f"generate_batch: {rows} rows (one per cfg_scale == 1 request, two per guided one), a mixed call holds at most {MAX_BATCH_REQUESTS}")
    elif mixed:
        raise ValueError("generate_batch: requests with cfg_scale == 1 and with guidance cannot share a call (the batch's row layout "
                         f"differs): cfg_scale = {[float(r.cfg_scale) for r in requests]}")
    prefix_lens = [0 if r.audio_prefix_codes is None else int(r.audio_prefix_codes.shape[-1]) for r in requests]
    prefixes = set(prefix_lens)
    if len(prefixes) > 1 and not ragged_prefix:
        raise ValueError(f"generate_batch: audio prefixes of different lengths {sorted(prefixes)} in one call are not supported "
                         "(the audio prefix length is shared by the batch)")
    call_halves = None if mixed else (2 if guided.pop() else 1)
    for i, r in enumerate(requests):
        halves = call_halves if call_halves is not None else (2 if float(r.cfg_scale) != 1.0 else 1)
        a = r.audio_prefix_codes
        check_request_shapes(f"generate_batch: request {i}: ", r.conditioning.shape, halves, d_model, r.cfg_scale, r.max_new_tokens,
                             None if a is None else a.shape, nq)
        _sampling_struct(r.sampling_params, 0)             # unknown sampling keys: TypeError, as in generate()
    return (None if mixed else call_halves == 2), (prefix_lens if ragged_prefix else prefixes.pop())


def _drain(gen):
    """Run a generation generator to its end and return its value."""
    try:
        while True:
            next(gen)
    except StopIteration as e:
        return e.value


class Zonos(nn.Module):
    def __init__(self, config: ZonosConfig, backbone_cls=DEFAULT_BACKBONE_CLS, autoencoder: DACAutoencoder | None = None):
        super().__init__()
        self.config = config
        dim = config.backbone.d_model
        self.eos_token_id = config.eos_token_id
        self.masked_token_id = config.masked_token_id
        self.autoencoder = autoencoder if autoencoder is not None else DACAutoencoder()
        self.backbone = backbone_cls(config.backbone)
        self.prefix_conditioner = PrefixConditioner(config.prefix_conditioner, dim)
        self.prefix_conditioner.attach(lambda: self.engine(1))
        self._conditioning_cache = ConditioningCache(max_size=32)
        vocab_size = find_multiple(1026, 8)  # 1024 codes + EOS + MASK, padded to 1032 (model.py:79-80)
        self.embeddings = nn.ModuleList([nn.Embedding(vocab_size, dim) for _ in range(self.autoencoder.num_codebooks)])
        self.fused_heads = nn.Linear(dim, self.autoencoder.num_codebooks * 1025, bias=False)
        self._engine: HipEngine | None = None
        self._spare: HipEngine | None = None          # second handle over the same weights (a concurrent generate() call)
        self._spare_guard = threading.RLock()
        self._repeats = 0                             # generations repeated on the launches path after a reported hand-off timeout
        self.mlp_weights = "bf16"                     # "fp8" after quantize_mlp_fp8()
        self.mamba_weights = "bf16"                   # "fp8" after quantize_mamba_fp8()
        self.fp8_small_rows = False                   # decode steps of 1..4 rows on the launches path read an attached FP8 stream too (set_fp8_small_rows)
        self.kv_cache = "bf16"                        # "fp8" after set_kv_cache("fp8"): generations of 5 rows and more keep an E4M3 copy of K/V for the decode attention;
                                                      # "fp8-only": they keep the E4M3 codes alone (no bf16 KV cache)

    # ------------------------------------------------------------------ loading
    @property
    def device(self) -> torch.device:
        return next(self.parameters()).device

    @classmethod
    def from_pretrained(cls, repo_id: str, revision: str | None = None, device: str = DEFAULT_DEVICE, **kwargs) -> "Zonos":
        """model.py:103-126.  Resolves config.json / model.safetensors through huggingface_hub's local cache only
        semantics are the caller's (no network on the GPU box: pass a local snapshot via from_local)."""
        from huggingface_hub import hf_hub_download
        config_path = hf_hub_download(repo_id=repo_id, filename="config.json", revision=revision)
        model_path = hf_hub_download(repo_id=repo_id, filename="model.safetensors", revision=revision)
        return cls.from_local(config_path, model_path, device, **kwargs)

    @classmethod
    def from_local(cls, config_path: str, model_path: str, device: str = DEFAULT_DEVICE, backbone: str | None = None,
                   mlp_weights: str = "bf16", mamba_weights: str = "bf16", fp8_small_rows: bool = False, kv_cache: str = "bf16") -> "Zonos":
        """model.py:128-176: bf16 model, embeddings zero-padded to the 1032-row tables, heads.{i} fused.  mlp_weights="fp8":
        quantize_mlp_fp8() after loading (lossy with respect to the checkpoint; see there); mamba_weights="fp8": quantize_mamba_fp8() (the
        hybrid checkpoint; likewise); fp8_small_rows: set_fp8_small_rows() (decode steps of 1..4 rows read the stream too); kv_cache="fp8"
        or "fp8-only": set_kv_cache() with that mode (lossy with respect to the bf16 model; see there); the defaults change nothing."""
        import safetensors
        if mlp_weights not in ("bf16", "fp8"):
            raise _lib.ZonosHipError(f"mlp_weights must be 'bf16' or 'fp8', not {mlp_weights!r}")
        if mamba_weights not in ("bf16", "fp8"):
            raise _lib.ZonosHipError(f"mamba_weights must be 'bf16' or 'fp8', not {mamba_weights!r}")
        if kv_cache not in KV_CACHE_MODES:
            raise ValueError(f"kv_cache must be 'bf16', 'fp8' or 'fp8-only', not {kv_cache!r}")
        config = ZonosConfig.from_dict(json.load(open(config_path)))
        backbone_cls = BACKBONES[backbone] if backbone else DEFAULT_BACKBONE_CLS
        model = cls(config, backbone_cls).to(device, torch.bfloat16)
        sd = model.state_dict()
        expected, seen = set(sd), set()
        with safetensors.safe_open(model_path, framework="pt") as f:
            for k in f.keys():
                t = f.get_tensor(k)
                if k.startswith("embeddings.") and k.endswith(".weight") and k in sd and sd[k].shape[0] != t.shape[0] and sd[k].shape[1] == t.shape[1]:
                    padded = torch.zeros(sd[k].shape, dtype=t.dtype)
                    padded[: t.shape[0]] = t
                    t = padded
                sd[k] = t
                seen.add("fused_heads.weight" if k.startswith("heads.") and k.endswith(".weight") else k)
        # The reference loads strictly (model.py:174: a tensor the model does not know is an error).  A tensor the file lacks
        # would stay at its random initialisation there; here it is an error as well: either way a checkpoint that does not
        # match the configuration (e.g. bias tensors of an attn_cfg this backbone does not implement) never runs silently.
        unexpected, missing = sorted(seen - expected), sorted(expected - seen)
        if unexpected or missing:
            raise _lib.ZonosHipError(f"checkpoint {model_path} does not match the model built from {config_path}: "
                                     f"unexpected tensors {unexpected[:8]}{'...' if len(unexpected) > 8 else ''}, "
                                     f"missing tensors {missing[:8]}{'...' if len(missing) > 8 else ''}")
        model.load_state_dict(sd, strict=True)
        if mlp_weights == "fp8":
            model.quantize_mlp_fp8()
        if mamba_weights == "fp8":
            model.quantize_mamba_fp8()
        if fp8_small_rows:
            model.set_fp8_small_rows(True)
        if kv_cache != "bf16":
            model.set_kv_cache(kv_cache)
        return model

    @torch.inference_mode()
    def quantize_mlp_fp8(self, small_rows: bool = False) -> "Zonos":
        """Weight-only FP8 for fc1 / fc2 of every transformer block (zonos_amd/quant.py: E4M3 codes, one power-of-two scale per weight
        row).  Quantises on the device, OVERWRITES the bf16 parameters in place with the dequantised values and keeps the codes and
        exponents as buffers of the block's mlp (fc1_q, fc1_exp, fc2_q, fc2_exp; not part of the state dict).  Decode steps of 5 or
        more rows then stream the codes - half the bytes - and compute exactly what the bf16 kernels compute on the dequantised
        weights, which every other path keeps reading: steps of up to 4 rows keep reading the bf16 copy unless `small_rows`
        (set_fp8_small_rows: then the GEMV launches of 1..4 rows stream the codes too; the persistent kernels never do).  Lossy with respect to the checkpoint (|Wdq - w| <= 2^-4 |w|), exact with
        respect to the model's own weights afterwards; the effect on audio quality is unmeasured.  Cached engines are dropped."""
        if self.config.backbone.ssm_cfg:
            raise _lib.ZonosHipError("quantize_mlp_fp8: the hybrid stack has no FP8 path")
        if self.device.type != "cuda":
            raise _lib.ZonosHipError("quantize_mlp_fp8 runs on the device: move the model to a cuda device first")
        eng = self.engine(1)
        for blk in self.backbone.layers:
            for name in ("fc1", "fc2"):
                W = getattr(blk.mlp, name).weight.data
                N, K = W.shape
                q = torch.empty((N, K), dtype=torch.uint8, device=W.device)
                e = torch.empty((N,), dtype=torch.int8, device=W.device)
                eng.call("zn_op_fp8_quantize_rows", W.data_ptr(), N, K, q.data_ptr(), e.data_ptr(), eng.stream())
                eng.call("zn_op_fp8_dequant_rows", q.data_ptr(), e.data_ptr(), N, K, W.data_ptr(), eng.stream())
                blk.mlp.register_buffer(name + "_q", q, persistent=False)
                blk.mlp.register_buffer(name + "_exp", e, persistent=False)
        torch.cuda.synchronize(self.device)
        self._engine = self._spare = None
        self.backbone._engine = None
        self.mlp_weights = "fp8"
        if small_rows:
            self.set_fp8_small_rows(True)
        return self

    @torch.inference_mode()
    def quantize_mamba_fp8(self, small_rows: bool = False) -> "Zonos":
        """Weight-only FP8 for in_proj / out_proj of every Mamba2 layer of a hybrid model (zonos_amd/quant.py: E4M3 codes, one power-of-two
        scale per weight row) - about four fifths of the weight bytes a hybrid decode step reads.  Like quantize_mlp_fp8: quantises on the
        device, OVERWRITES the bf16 parameters in place with the dequantised values and keeps the codes and exponents as buffers of the
        mixer (in_proj_q, in_proj_exp, out_proj_q, out_proj_exp; not part of the state dict).  Decode steps of 5 or more rows then stream
        the codes - half the bytes - and compute exactly what the bf16 kernels compute on the dequantised weights; the prefill keeps
        reading the bf16 copy, and steps of up to 4 rows keep reading the bf16 copy unless `small_rows` (set_fp8_small_rows: then in_proj and
        out_proj of a step of 1..4 rows stream the codes too - batch 1 and 2, stream(), one-slot sessions).  Lossy with respect to the checkpoint (|Wdq - w| <= 2^-4 |w|), exact with respect to
        the model's own weights afterwards; the effect on audio quality is unmeasured.  Cached engines are dropped.
        Raises ZonosHipError - and changes nothing - on a transformer model, and on a hybrid model of other widths than the FP8 kernels
        serve (d_model 2048, d_inner 4096: Zonos-v0.1-hybrid): a stream that no decode step would read is refused, not carried along."""
        bb = self.config.backbone
        if not bb.ssm_cfg:
            raise _lib.ZonosHipError("quantize_mamba_fp8: a transformer model has no Mamba2 layers (quantize_mlp_fp8 serves its fc1 / fc2)")
        if self.device.type != "cuda":
            raise _lib.ZonosHipError("quantize_mamba_fp8 runs on the device: move the model to a cuda device first")
        mixers = [blk.mixer for blk in self.backbone.layers if blk.is_mamba]
        for mx in mixers:
            d_in, d_model = mx.out_proj.weight.shape[1], mx.in_proj.weight.shape[1]
            if d_model != 2048 or d_in != 4096:
                raise _lib.ZonosHipError(f"quantize_mamba_fp8: the FP8 kernels serve d_model 2048 and d_inner 4096 (got d_model {d_model}, d_inner {d_in})")
        eng = self.engine(1)
        for mx in mixers:
            for name in ("in_proj", "out_proj"):
                W = getattr(mx, name).weight.data
                N, K = W.shape
                q = torch.empty((N, K), dtype=torch.uint8, device=W.device)
                e = torch.empty((N,), dtype=torch.int8, device=W.device)
                eng.call("zn_op_fp8_quantize_rows", W.data_ptr(), N, K, q.data_ptr(), e.data_ptr(), eng.stream())
                eng.call("zn_op_fp8_dequant_rows", q.data_ptr(), e.data_ptr(), N, K, W.data_ptr(), eng.stream())
                mx.register_buffer(name + "_q", q, persistent=False)
                mx.register_buffer(name + "_exp", e, persistent=False)
        torch.cuda.synchronize(self.device)
        self._engine = self._spare = None
        self.backbone._engine = None
        self.mamba_weights = "fp8"
        if small_rows:
            self.set_fp8_small_rows(True)
        return self

    def set_fp8_small_rows(self, on: bool) -> "Zonos":
        """Whether decode steps of 1..4 rows on the launches path read the FP8 streams of a quantised model (quantize_mlp_fp8 / quantize_mamba_fp8)
        instead of the dequantised bf16 copy: the same bits from half the weight bytes (zn_debug_tune(ZN_TUNE_FP8_SMALL_ROWS, 2) on every engine
        of the model).  Off by default; without a stream it changes nothing.  Which path a generation takes does not change, and the persistent
        kernels (the transformer at batch 1) keep reading the bf16 copy.  Cached engines are dropped."""
        self.fp8_small_rows = bool(on)
        self._engine = self._spare = None
        self.backbone._engine = None
        return self

    def set_kv_cache(self, mode: str) -> "Zonos":
        """"fp8": generations and serving sessions whose decode step has 5 rows or more (three guided utterances, five unguided ones) round K (after RoPE)
        and V to the E4M3 grid at every KV append (zonos_amd/quant.py kv_round_e4m3: no scale, saturation at +-448), keep the rounded values in the
        bf16 cache - the prefill attention and every other reader see them - and the one-byte codes in a second cache, which the decode attention reads:
        half the K/V bytes per step.  Lossy with respect to the bf16 model (relative error up to 2^-4 per K/V element, absolute floor 2^-10), exact with
        respect to its own rounded cache; its effect on audio quality is unmeasured.  It costs memory: 1.5 x the KV bytes (the bf16 copy stays) - "fp8-only"
        drops that copy.
        "fp8-only": the same rounding, the same codes and the same results bit for bit, with the codes as the only KV storage of such a generation or
        session: no bf16 KV tensor is allocated, the appends write the codes alone, and the prefill attention and an admission's scratch cache read and
        hold codes too.  Half the KV bytes of the bf16 model, a third of "fp8" (kv_cache_bytes).
        With fewer rows either mode is inert (generate(batch_size <= 2), stream()).  "bf16" (the default) switches it off.  A hybrid model raises
        ValueError.  Cached engines are dropped."""
        if mode not in KV_CACHE_MODES:
            raise ValueError(f"kv_cache must be 'bf16', 'fp8' or 'fp8-only', not {mode!r}")
        if mode != "bf16" and self.config.backbone.ssm_cfg:
            raise ValueError(f"kv_cache={mode!r}: the hybrid stack's attention layers keep a bf16 KV cache")
        self.kv_cache = mode
        self._engine = self._spare = None
        self.backbone._engine = None
        return self

    def kv_fp8_plan(self, rows: int) -> dict:
        """What a generation whose decode step has `rows` rows (two per guided utterance) does with its K/V as this model is set now: {"rounded": whether
        the appends round to the E4M3 grid and keep the code cache, "attention_reads": "fp8" where the decode attention reads the codes, else "bf16"}."""
        rows = int(rows)
        if rows < 1:
            raise ValueError("kv_fp8_plan: rows must be >= 1")
        rounded = self.kv_cache != "bf16" and not self.config.backbone.ssm_cfg and rows >= KV_FP8_MIN_ROWS
        reads = rounded
        if rounded and self._engine is not None:      # (an engine's tune keys - ZN_TUNE_KV_FP8 = 2 - and the library's own plan decide where one exists)
            out = (C.c_int32 * 2)()
            self._engine.call("zn_kv_fp8_plan", rows, out)
            rounded, reads = bool(out[0]), bool(out[1])
        return {"rounded": rounded, "attention_reads": "fp8" if reads else "bf16"}

    def kv_cache_plan(self, rows: int) -> dict:
        """kv_fp8_plan's two keys with the same meaning, and "bf16_cache": whether a generation whose decode step has `rows` rows allocates the bf16 KV
        cache at all (False: codes only, set_kv_cache("fp8-only") in effect)."""
        plan = self.kv_fp8_plan(rows)
        codes_only = plan["rounded"] and self.kv_cache == "fp8-only"
        if codes_only and self._engine is not None:
            out = (C.c_int32 * 3)()
            self._engine.call("zn_kv_cache_plan", int(rows), out)
            codes_only = not out[2]
        return {**plan, "bf16_cache": not codes_only}

    def kv_cache_bytes(self, rows: int, max_len: int) -> dict:
        """The KV bytes a generation of `rows` rows and `max_len` positions (rounded up to a multiple of 8, as setup_cache does) allocates over all layers as
        this model is set now: {"bf16": n, "codes": n}, from the library's zn_kv_bytes_per_layer / zn_kv_fp8_bytes_per_layer."""
        rows, max_len = int(rows), find_multiple(int(max_len), 8)
        if rows < 1 or max_len < 1:
            raise ValueError("kv_cache_bytes: rows and max_len must be >= 1")
        plan = self.kv_cache_plan(rows)
        ao = attention_options(self.config.backbone)      # (the byte functions read the head geometry alone)
        zc = _lib.zn_config(d_model=self.config.backbone.d_model, n_heads=ao["num_heads"], n_heads_kv=ao["num_heads_kv"])
        lib, n_layer = _lib.load(), self.config.backbone.n_layer
        return {"bf16": n_layer * int(lib.zn_kv_bytes_per_layer(C.byref(zc), rows, max_len)) if plan["bf16_cache"] else 0,
                "codes": n_layer * int(lib.zn_kv_fp8_bytes_per_layer(C.byref(zc), rows, max_len)) if plan["rounded"] else 0}

    def _kv_buffers(self, eng: HipEngine, rows: int, max_seqlen: int) -> "KvBuffers":
        """The KV buffers of one generation or session of `rows` rows on `eng`, decided in one place from the library's plan (zn_kv_cache_plan): the
        InferenceParams (its key_value_memory_dict stays empty where no bf16 cache is needed: no bf16 KV tensor is allocated), the pointer array for
        zn_gen_begin (None -> NULL there) and the code caches (None where nothing is rounded), which `_bind_kv_buffers` hands to the library after
        zn_gen_begin.  The caller keeps the result alive to the generation's end."""
        out = (C.c_int32 * 3)()
        eng.call("zn_kv_cache_plan", rows, out)
        n_layer = self.config.backbone.n_layer
        if out[2]:
            ip = self.setup_cache(batch_size=rows, max_seqlen=max_seqlen)
            kv_ptrs = (C.c_void_p * n_layer)(*[ip.key_value_memory_dict[i][0].data_ptr() for i in range(n_layer)])
        else:
            ip = InferenceParams(find_multiple(max_seqlen, 8), rows, 0, 0, {}, torch.zeros(rows, dtype=torch.int32, device=self.device))
            kv_ptrs = None
        codes = None
        if out[0]:
            per = int(eng.lib.zn_kv_fp8_bytes_per_layer(C.byref(eng.zc), rows, ip.max_seqlen))
            codes = [torch.empty(per, dtype=torch.uint8, device=self.device) for _ in range(n_layer)]
        return KvBuffers(ip, kv_ptrs, codes)

    def _bind_kv_buffers(self, eng: HipEngine, bufs: "KvBuffers") -> None:
        """After zn_gen_begin: the code caches of `_kv_buffers`, where there are any (zn_gen_bind_kv_fp8)."""
        if bufs.codes is not None:
            eng.call("zn_gen_bind_kv_fp8", (C.c_void_p * len(bufs.codes))(*[t.data_ptr() for t in bufs.codes]))

    def _bind_kv_codes(self, eng: HipEngine, rows: int, max_len: int):
        """The code caches of the generation just begun on `eng` (zn_gen_bind_kv_fp8) where the FP8 KV cache is in effect for `rows` rows: one uint8
        tensor [rows, max_len, 2, Hkv, hd] per layer, which the caller keeps alive to the generation's end; else None."""
        if self.kv_cache == "bf16":
            return None
        out = (C.c_int32 * 2)()
        eng.call("zn_kv_fp8_plan", rows, out)
        if not out[0]:
            return None
        n_layer = self.config.backbone.n_layer
        per = int(eng.lib.zn_kv_fp8_bytes_per_layer(C.byref(eng.zc), rows, max_len))
        codes = [torch.empty(per, dtype=torch.uint8, device=self.device) for _ in range(n_layer)]
        eng.call("zn_gen_bind_kv_fp8", (C.c_void_p * n_layer)(*[t.data_ptr() for t in codes]))
        return codes

    def mamba_fp8_plan(self, rows: int) -> dict:
        """Whether in_proj and out_proj of the Mamba2 layers would read the FP8 stream in a decode step of `rows` rows (two per guided
        utterance) as this model's engine runs it now: {"in_proj": bool, "out_proj": bool}; both False before quantize_mamba_fp8(), up to
        4 rows unless fp8_small_rows, and under zn_debug_tune(ZN_TUNE_MAMBA_FP8, 2) on the engine."""
        a, b = self.engine((int(rows) + 1) // 2).mamba_fp8_plan(int(rows))
        return {"in_proj": bool(a), "out_proj": bool(b)}

    def _load_from_state_dict(self, state_dict, prefix, *args):
        """model.py:208-223: per-codebook heads.{i}.weight [1025,d] -> fused_heads.weight [9*1025,d]."""
        if f"{prefix}heads.0.weight" in state_dict:
            ws, i = [], 0
            while f"{prefix}heads.{i}.weight" in state_dict:
                ws.append(state_dict.pop(f"{prefix}heads.{i}.weight"))
                i += 1
            state_dict[f"{prefix}fused_heads.weight"] = torch.cat(ws, dim=0)
        super()._load_from_state_dict(state_dict, prefix, *args)

    def _apply(self, fn, *a, **k):
        self._engine = None       # device/dtype moves invalidate bound pointers
        self._spare = None
        if getattr(self.backbone, "_engine", None) is not None:
            self.backbone._engine = None
        return super()._apply(fn, *a, **k)

    def _new_engine(self, batch_size: int) -> HipEngine:
        eng = HipEngine(self.backbone, [m.weight for m in self.embeddings], self.fused_heads.weight,
                        max_rows=2 * batch_size, double_out_proj=getattr(self.backbone, "ref_double_out_proj", True),
                        n_codebooks=self.autoencoder.num_codebooks, vocab_head=1025, vocab_embed=self.embeddings[0].weight.shape[0],
                        eos_id=self.eos_token_id, mask_id=self.masked_token_id)
        if self.fp8_small_rows:      # (every engine of the model: the cached one and the spare)
            eng.call("zn_debug_tune", _lib.ZN_TUNE_FP8_SMALL_ROWS, 2)
        if self.kv_cache != "bf16":
            eng.call("zn_set_kv_fp8", 1)
            if self.kv_cache == "fp8-only":
                eng.call("zn_set_kv_fp8_only", 1)
        return eng

    def engine(self, batch_size: int = 1) -> HipEngine:
        # (both handles are created and replaced under one lock: two threads arriving together must not each build an engine,
        # nor drop the spare another thread is about to take)
        with self._spare_guard:
            e = self._engine
            if e is None or e.max_rows < 2 * batch_size or e.device != self.device:
                self._engine = e = self._new_engine(batch_size)
                self._spare = None
            return e

    def decode_rows_plan(self, rows: int) -> dict:
        """Activation rows per weight pass of in_proj, out_proj, fc1, fc2 and the heads in a decode step of `rows` rows (two per guided
        utterance) as this model's engine runs it now: 4 up to 4 rows, 16 up to 16 rows, 64 from 17 rows on - a step of 32 rows then reads
        every weight once, not once per 16 rows (`zn_debug_tune(ZN_TUNE_WIDE_ROWS, 1)` on the engine restores the groups of 16)."""
        return self.engine((int(rows) + 1) // 2).decode_rows_plan(int(rows))

    def hybrid_rows_plan(self, rows: int) -> dict:
        """The same report for a hybrid checkpoint: activation rows per weight pass of the Mamba2 in_proj and out_proj, the attention layers' in_proj,
        out_proj, fc1 and fc2, and the heads (`zn_debug_tune(ZN_TUNE_WIDE_HYBRID, 1)` on the engine puts the Mamba2 in_proj back to groups of 16).  Raises
        on a transformer checkpoint."""
        return self.engine((int(rows) + 1) // 2).hybrid_rows_plan(int(rows))

    def handoff_counters(self) -> dict:
        """Hand-off timeouts are never silent: per engine, what the library counted (include/zonos_hip.h zn_get_counters) plus the
        generations this model repeated after a reported timeout."""
        out = dict(repeated_generations=self._repeats)
        for name, e in (("engine", self._engine), ("spare", self._spare)):
            if e is not None:
                out[name] = e.counters()
        return out

    def _acquire_engine(self, batch_size: int) -> HipEngine:
        """The engine a generate() call runs on, with its lock held.  The reference serves two requests per model at a time
        (utilities/app_constants.py:18); one library handle carries one generation, so a second handle over the SAME weight tensors
        (a few MB of workspace) takes the second request instead of making it wait for the first.  The device's persistent-kernel
        tenancy (include/zonos_hip.h) stays with whichever generation began first; the other runs the launches path."""
        def take(e, blocking):
            # (the engine lock is re-entrant for the calls a generation makes on its own thread; `generating` keeps a generate()
            # nested in a callback from re-entering the handle that is mid-generation)
            if not e.lock.acquire(blocking=blocking):
                return False
            if getattr(e, "generating", False):
                e.lock.release()
                return False
            e.generating = True
            return True
        eng = self.engine(batch_size)
        if take(eng, False):
            return eng
        with self._spare_guard:
            sp = self._spare
            if sp is None or sp.max_rows < 2 * batch_size or sp.device != self.device:
                self._spare = sp = self._new_engine(batch_size)
        if take(sp, False):
            return sp
        if not take(eng, True):                             # both busy: queue on the first
            raise _lib.ZonosHipError("generate() re-entered from a callback while both of the model's engines are generating")
        return eng

    @contextlib.contextmanager
    def _engine_held(self, batch_size: int):
        """`_acquire_engine` for the length of a `with` block: the one place an engine is released."""
        eng = self._acquire_engine(batch_size)
        try:
            yield eng
        finally:
            eng.generating = False
            eng.lock.release()

    # ------------------------------------------------------------------ embed / heads
    @torch.inference_mode()
    def embed_codes(self, codes: torch.Tensor, _eng: HipEngine | None = None) -> torch.Tensor:
        """codec_utils.py:15-37: codes [B, n_q, T] -> bf16 [B, T, d]."""
        B, nq, T = codes.shape
        eng = _eng if _eng is not None else self.engine(1)
        flat = codes.permute(0, 2, 1).reshape(B * T, nq).to(device=self.device, dtype=torch.int32).contiguous()
        out = torch.empty(B * T, self.config.backbone.d_model, dtype=torch.bfloat16, device=self.device)
        eng.call("zn_op_embed", flat.data_ptr(), out.data_ptr(), B * T, eng.stream())
        return out.view(B, T, -1)

    @torch.inference_mode()
    def apply_heads(self, hidden_states: torch.Tensor) -> torch.Tensor:
        """codec_utils.py:40-79: [B, S, d] -> [B, n_q, S, 1025] (bf16)."""
        B, S, d = hidden_states.shape
        nq = self.autoencoder.num_codebooks
        eng = self.engine(1)
        x = hidden_states.reshape(B * S, d).contiguous()
        out = torch.empty(B * S, nq * 1025, dtype=torch.bfloat16, device=x.device)
        eng.call("zn_op_linear", x.data_ptr(), None, None, self.fused_heads.weight.data_ptr(), out.data_ptr(), B * S, nq * 1025, d, eng.stream())
        return out.view(B, S, nq, 1025).transpose(1, 2)

    @torch.inference_mode()
    def prepare_conditioning(self, cond_dict: dict, uncond_dict: dict | None = None, use_cache: bool = False, cfg_scale: float = 1.0) -> torch.Tensor:
        """model.py:237-265 -> conditioning_cache.py:139-193: [2B or B, L_c, d] bf16 ([cond ‖ uncond] when cfg_scale != 1; the B
        conditional rows at the default cfg_scale=1.0, which generate(cfg_scale=1.0) takes)."""
        return prepare_conditioning_with_cache(self.prefix_conditioner, cond_dict=cond_dict, uncond_dict=uncond_dict, use_cache=use_cache,
                                               cfg_scale=cfg_scale, cache=self._conditioning_cache if use_cache else None)

    def setup_cache(self, batch_size: int, max_seqlen: int, dtype: torch.dtype = torch.bfloat16) -> InferenceParams:
        """model.py:305-338: length rounded to x8, bf16 KV per layer, lengths_per_sample int32 zeros."""
        max_seqlen = find_multiple(max_seqlen, 8)
        kv = self.backbone.allocate_inference_cache(batch_size, max_seqlen, dtype=dtype)
        lengths = torch.zeros(batch_size, dtype=torch.int32, device=self.device)
        return InferenceParams(max_seqlen, batch_size, 0, 0, kv, lengths)

    def can_use_cudagraphs(self) -> bool:
        return self.device.type == "cuda"   # the step is always replayed as a hipGraph

    # ------------------------------------------------------------------ generate
    @torch.inference_mode()
    def generate(self, prefix_conditioning: torch.Tensor, audio_prefix_codes: torch.Tensor = None, max_new_tokens: int = 86 * 30,
                 cfg_scale: float = 2.0, batch_size: int = 1, sampling_params: dict = dict(min_p=0.1),
                 disable_torch_compile: bool = False, callback: Callable[[torch.Tensor, int, int], bool] | None = None,
                 seed: int | None = None, _trace: dict | None = None, conditioning_lengths: Sequence[int] | None = None):
        """zonos/model.py:354-548.  prefix_conditioning bf16 [2B, L_c, d] = [cond ‖ uncond] with guidance, or the B conditional
        rows [B, L_c, d] when cfg_scale == 1 (what `prepare_conditioning` returns at its default cfg_scale=1.0: no unconditional
        half, no CFG mix, half the rows per utterance); returns int64 [B, 9, T_out] with values in [0, 1023].  Batch semantics
        for B > 1 (the reference crashes there): B independent utterances, rows [cond_0..cond_{B-1},
        uncond_0..uncond_{B-1}] (or [cond_0..cond_{B-1}] without guidance).  `seed` seeds the device Gumbel-max stream (default:
        drawn from torch's generator).

        `conditioning_lengths` batches utterances of different prompt lengths: B valid lengths L_b in 1..L_c of a RIGHT-padded
        `prefix_conditioning` (`conditioning.pad_conditionings` builds both).  Utterance b's audio prefix follows its L_b valid positions
        directly and the padding is never read: every utterance gets the codes it would get in a batch of utterances of its own length
        (DESIGN.md 4.1b).  The audio prefix length and max_new_tokens stay shared by the batch.  None: every row holds L_c positions."""
        self._check_rows(prefix_conditioning, cfg_scale, batch_size, conditioning_lengths)
        call = GenCall.plain(prefix_conditioning, audio_prefix_codes, max_new_tokens, cfg_scale, batch_size, sampling_params, seed, conditioning_lengths)
        return self._run(call, Hooks(callback, _trace)).to(self.device)

    def _run(self, call: GenCall, hooks: Hooks):
        """One generation to its end, on an engine of its own.  An engine's handle holds the generation's state: a third concurrent call on
        one model queues here.  Engines are sized by rows (engine(b) holds 2 b): one unguided utterance runs on engine(1), like a guided one."""
        with self._engine_held((call.engine_rows + 1) // 2) as eng, torch.cuda.device(self.device):
            run = lambda: _drain(self._generation(eng, call, torch.cuda.current_stream(self.device), hooks))
            return self._with_timeout_policy(run, caller_saw_frames=hooks.callback is not None or hooks.trace is not None)

    def _check_rows(self, prefix_conditioning, cfg_scale, B, conditioning_lengths=None) -> int:
        n = prefix_conditioning.shape[0]
        if cfg_scale == 1:
            # [cond ‖ uncond] rows without guidance: the reference's prepare_conditioning would have returned B rows (conditioning_cache.py:172)
            assert n != 2 * B, f"cfg_scale=1 takes the batch_size={B} conditional rows only, got {n} rows ([cond ‖ uncond] is for cfg_scale != 1)"
            if n != B:
                raise ValueError(f"prefix_conditioning must have batch_size={B} rows when cfg_scale == 1, got {n}")
        elif n != 2 * B:
            raise ValueError(f"prefix_conditioning must have 2*batch_size={2 * B} rows, got {n}")
        if conditioning_lengths is not None:
            lens, L_c = list(conditioning_lengths), prefix_conditioning.shape[1]
            if len(lens) != B:
                raise ValueError(f"conditioning_lengths must hold batch_size={B} lengths, got {len(lens)}")
            bad = [v for v in lens if int(v) != v or not 1 <= int(v) <= L_c]
            if bad:
                raise ValueError(f"conditioning_lengths must lie in 1..{L_c} (the padded prefix_conditioning's length), got {bad}")
        self._check_device()
        return n

    def _check_device(self) -> None:
        if self.device.type != "cuda":
            raise _lib.ZonosHipError("zonos_amd runs on MI355X only: move the model to a cuda device (no CPU fallback)")

    @torch.inference_mode()
    def generate_batch(self, requests: Sequence[GenRequest], ragged_prefix: bool = False, _trace: dict | None = None,
                       mixed_guidance: bool = False) -> list[torch.Tensor]:
        """One generation for several requests, each with its own sampling parameters, seed, cfg_scale and max_new_tokens (and its own
        prompt length); returns, per request, int64 [1, 9, T_b] as `generate()` returns it, cut and finalised for that request alone.

        The conditionings are right-padded (`pad_conditionings`) and prefilled as `conditioning_lengths` does; the call runs max_b
        max_new_tokens frames at most and ends at the first stop check after every request has stopped or spent its budget.  Request b is
        sampled with the random stream of a one-utterance `generate(seed=seed_b)`, whatever slot it takes; its codes are
        its row's first prefix + max_new_tokens_b + 9 delayed columns, finalised at `row_end_offset`.  ValueError, before any launch: an
        empty list, more than MAX_BATCH_REQUESTS requests, guided and cfg_scale == 1 requests together, audio prefixes of different
        lengths.  A single request is `generate()` with its arguments.

        `ragged_prefix=True` lifts the last refusal: request b continues its own `audio_prefix_codes` of P_b frames (None: 0) and gets the
        codes it would get in a call whose requests all bring P_b frames.  Row b of the code buffer is left-aligned: its
        prefix, its max_new_tokens_b unknown cells, then the mask token; the device shifts the row's column by P_b - max_b P_b
        (zn_gen_set_prefix_rows), and the right-padded prefill rows are assembled by one kernel (zn_op_assemble_prefill).

        `mixed_guidance=True` lifts the refusal of guided and cfg_scale == 1 requests together: the call runs in the
        unguided layout with one row per cfg_scale == 1 request and two adjacent rows per guided one, in request order, at most
        MAX_BATCH_REQUESTS rows; the sampler of a guided request's rows mixes the two rows' logits (zn_row_params' row pair).  A guided
        request's result is read from its first row, and every request is finalised with the cadence of a call of len(requests)
        utterances.  `_trace` logits are then [rows, 9, 1025].  It composes with `ragged_prefix`; a call of one kind only is the call
        without the keyword."""
        reqs, dev = list(requests), self.device
        guided, _ = check_requests(reqs, self.config.codebook_dimension, self.config.backbone.d_model, ragged_prefix, mixed_guidance)
        if guided is not None and len(reqs) == 1:
            r = reqs[0]
            return [self.generate(r.conditioning, r.audio_prefix_codes, int(r.max_new_tokens), r.cfg_scale, 1, r.sampling_params, seed=r.seed,
                                  _trace=_trace)]
        self._check_device()
        # guided None: both kinds of request are present, the call runs R rows in the unguided layout
        call = GenCall.mixed(reqs, ragged_prefix, dev) if guided is None else GenCall.batch(reqs, guided, ragged_prefix, dev)
        return [o.to(dev) for o in self._run(call, Hooks(trace=_trace))]

    def serve(self, requests, slots: int = 8, max_prompt: int = 64, max_new_tokens: int = 86 * 30, guided: bool | None = True, sched_every: int = 8,
              _trace: dict | None = None, _stats: dict | None = None) -> Iterator[ServeResult]:
        """Requests join a running batch as slots free up: a generator of `ServeResult(index, codes, error)` in order of completion.

        `requests` is any iterable of `GenRequest`, pulled lazily: an item is taken only when a slot is free at a scheduling point (every
        `sched_every` decode steps, enqueued in one call), and an item that is None means that nothing is waiting right now.  `index`
        counts the requests pulled (None items do not count).  A request is prefilled into its slot while the other rows keep their state
        (zn_gen_admit), decodes there with its own parameters, seed, guidance strength, budget and audio prefix, and is retired at the
        first scheduling point at which a `generate_batch()` call of `slots` requests would have stopped watching it: its codes are the
        codes of its row in such a call.  `max_prompt` (conditioning positions + audio prefix frames of the longest
        request) and `max_new_tokens` size the KV cache and the code buffer once; a request that does not fit them, whose guidance differs
        from the session's (`guided`: cfg_scale != 1) or that is malformed yields ServeResult(index, None, ValueError) and takes no slot.

        `guided=None` opens a MIXED session: `slots` then counts rows, a cfg_scale == 1 request takes one and a guided
        request the two lowest idle ones (its conditional and its unconditional row; its codes are read from the lower).  Admission stays
        FIFO: a guided request at the head of the queue waits until two rows are idle and nothing overtakes it.  Every request's codes
        are those of its row in a `generate_batch()` call of `slots` ROWS of its own kind.  "retired" of `_trace` receives
        (index, its slots, their rows of the code buffer) per retirement of such a session.

        The engine and the stream current at the call are held while the generator is alive; `close()`, leaving the loop early or garbage
        collection releases them.  A session runs no persistent kernel, so no hand-off timeout can occur; any library error raises.
        `_trace`: one step per enqueue; "logits" receives [slots, 9, 1025] per admission and per step, "slots" a (kind, session step,
        request index per slot) record for each of them (an admission's record names the admitted slots only).  `_stats` (tools/servebench.py)
        receives the session's decode steps and admissions, per request index the time.perf_counter() at which its admission was enqueued
        (_stats["admitted_at"]), and with _stats["time_admissions"] set the seconds spent in admissions, each bracketed by a
        synchronisation."""
        dev, shape = self.device, self._serve_shape("serve", slots, max_prompt, max_new_tokens, guided, sched_every)
        return self._serve_gen(torch.cuda.current_stream(dev), iter(requests), shape, _trace, _stats)

    def serve_stream(self, requests, slots: int = 8, max_prompt: int = 64, max_new_tokens: int = 86 * 30, guided: bool | None = True,
                     sched_every: int = 8, chunk_frames: int = 16, _stats: dict | None = None, sample_rate: int | None = None,
                     pcm16: bool = False) -> Iterator[ServeChunk]:
        """`serve()` with audio as it happens: a generator of `ServeChunk(index, codes, wav, done, error)`.  The session is `serve()`'s -
        the same admissions, steps and retirements.  At a scheduling point every busy slot whose final frames (`release_limit` of its
        own column) have grown by at least `chunk_frames` since its last chunk yields them with the samples the DAC can decode from
        them, and every request retired there yields its last chunk (done=True): what `rows.finalise_row` keeps beyond the frames released.
        The windows of all slots are decoded in one ragged pass (`DACAutoencoder.stream_set`, zn_dac_decode_spans) on the session's
        stream.  For every request the concatenated codes equal the `ServeResult.codes` of `serve()` for the same source and settings,
        and the concatenated wav `autoencoder.decode()` of them, bit for bit.  A refused request yields
        ServeChunk(index, None, None, True, ValueError).  The engine is held as by `serve()`; `_stats` as there.  `sample_rate` / `pcm16`:
        every request's wav is `autoencoder.decode(codes, sample_rate, pcm16)` instead, resampled on the session's stream in one launch
        per scheduling point."""
        if int(chunk_frames) < 1:
            raise ValueError(f"serve_stream: chunk_frames must be >= 1, got {chunk_frames}")
        self.autoencoder._resampler(sample_rate, pcm16)           # (a bad rate is refused here, not at the first next())
        dev, shape = self.device, self._serve_shape("serve_stream", slots, max_prompt, max_new_tokens, guided, sched_every)
        return self._serve_gen(torch.cuda.current_stream(dev), iter(requests), shape, None, _stats, int(chunk_frames), (sample_rate, pcm16))

    def _serve_shape(self, who: str, slots, max_prompt, max_new_tokens, guided, sched_every) -> ServeShape:
        """The arguments serve() and serve_stream() share, checked; `who` names the caller in the messages."""
        slots, sched_every, max_prompt, max_new_tokens = int(slots), int(sched_every), int(max_prompt), int(max_new_tokens)
        if not 1 <= slots <= MAX_BATCH_REQUESTS:
            raise ValueError(f"{who}: slots must lie in 1..{MAX_BATCH_REQUESTS}, got {slots}")
        if sched_every < 1 or max_prompt < 1 or max_new_tokens < 1:
            raise ValueError(f"{who}: sched_every={sched_every}, max_prompt={max_prompt}, max_new_tokens={max_new_tokens} must all be >= 1")
        self._check_device()
        return ServeShape(slots, max_prompt, max_new_tokens, None if guided is None else bool(guided), sched_every)

    def _serve_gen(self, ts, source, shape: ServeShape, _trace, _stats=None, chunk_frames=None, audio=(None, False)):
        """The session of serve() (chunk_frames None: yields ServeResult) and of serve_stream() (yields ServeChunk): the engine is held
        while the generator is alive, and every scheduling point's results go out with the caller's device and stream current."""
        session = ServeSession(self, ts, source, shape, _trace, _stats, chunk_frames, audio)
        with self._engine_held((session.R + 1) // 2) as eng:
            try:
                session.open(eng)
                stop = False
                while not stop:
                    out, stop = session.point()
                    yield from out
            finally:
                session.close()

    def stream(self, prefix_conditioning: torch.Tensor, audio_prefix_codes: torch.Tensor = None, max_new_tokens: int = 86 * 30,
               cfg_scale: float = 2.0, sampling_params: dict = dict(min_p=0.1), seed: int | None = None, chunk_frames: int = 16,
               batch_size: int = 1, sample_rate: int | None = None, pcm16: bool = False) -> Iterator[StreamChunk]:
        """`generate()` + `autoencoder.decode()` as they happen: a generator of `StreamChunk(codes, wav)`.  Every `chunk_frames` decode steps
        it yields the frames that have become final (`release_limit`) and the samples the DAC can decode from them (`DACAutoencoder.stream`);
        the rest comes when the generation ends.  With the same arguments and seed, the concatenated codes equal `generate(...)` and the
        concatenated wav `autoencoder.decode(generate(...))`, bit for bit.  Batch size 1 (guided, or cfg_scale=1).

        The generation's engine and the device's persistent-kernel tenancy are held while the generator is alive; `close()`, leaving a for
        loop early or garbage collection releases them.  Every launch (decode steps and DAC) goes to the stream current when stream() is
        called.  A hand-off timeout raises: it is not repeated on the launches path, as the caller may already hold audio.
        `sample_rate` / `pcm16`: the concatenated wav is `autoencoder.decode(generate(...), sample_rate, pcm16)` instead, resampled on the
        generation's stream chunk by chunk."""
        if batch_size != 1:
            raise ValueError(f"stream() generates one utterance at a time, got batch_size={batch_size}")
        if int(chunk_frames) < 1:
            raise ValueError(f"chunk_frames must be >= 1, got {chunk_frames}")
        n = self._check_rows(prefix_conditioning, cfg_scale, 1)
        self.autoencoder._resampler(sample_rate, pcm16)           # (a bad rate is refused here, not at the first next())
        seed, dev = draw_seed(seed), self.device
        # (the record is built at the first next(), where the errors of its arguments have always been raised)
        build = lambda: GenCall.plain(prefix_conditioning, audio_prefix_codes, max_new_tokens, cfg_scale, 1, sampling_params, seed)
        return self._stream_gen(dev, torch.cuda.current_stream(dev), (n + 1) // 2, build, int(chunk_frames), (sample_rate, pcm16))

    def _stream_gen(self, dev, ts, rows, build, chunk, audio=(None, False)):
        nq, eos = self.config.codebook_dimension, self.eos_token_id
        with contextlib.ExitStack() as held:               # closed by hand below; also by close(), an error or garbage collection
            eng = held.enter_context(self._engine_held(rows))
            # (each stretch between two yields runs with the generation's device and stream current, and leaves the caller's as it found them)
            with torch.inference_mode(), torch.cuda.device(dev), torch.cuda.stream(ts):
                dac = self.autoencoder.stream(ts, *audio)
                gen = self._generation(eng, build(), ts, Hooks(chunk=chunk))

            @held.callback
            def end_generation():                          # before the engine goes back.  A stream left early: its steps drain, zn_gen_end
                with torch.cuda.device(dev), torch.cuda.stream(ts):
                    gen.close()
            released, scanned, eos_frame = 0, 0, None      # frames handed out; delayed columns of codebook 0 read; first EOS frame
            while True:
                with torch.inference_mode(), torch.cuda.device(dev), torch.cuda.stream(ts):
                    try:
                        delayed, offset = next(gen)
                    except StopIteration as e:
                        final = e.value                    # finalise_codes of the whole generation
                        if final.shape[2] < released:
                            raise _lib.ZonosHipError(f"stream(): {released} frames released, the generation kept {final.shape[2]}")
                        codes = final[..., released:].to(dev)
                        wav = torch.cat([dac.push(codes), dac.flush()], dim=2)
                        chunk_out = StreamChunk(codes, wav) if codes.shape[2] or wav.shape[2] else None
                        break
                    if eos_frame is None and offset > scanned:
                        col = delayed[0, 0, scanned + 1:offset + 1].cpu()       # codebook 0 of frames scanned .. offset - 1
                        hit = (col == eos).nonzero()
                        if len(hit):
                            eos_frame = scanned + int(hit[0, 0])
                        scanned = offset
                    limit = release_limit(offset, nq, eos_frame)
                    chunk_out = None
                    if limit > released:
                        codes = map_codes(revert_delay_pattern(delayed[..., released:limit + nq].cpu().to(torch.int64))).to(dev)
                        released = limit
                        chunk_out = StreamChunk(codes, dac.push(codes))
                if chunk_out is not None:
                    yield chunk_out
            held.close()                                   # the generation has ended: the engine is free before the last chunk goes out
            if chunk_out is not None:
                yield chunk_out

    def _with_timeout_policy(self, run, caller_saw_frames: bool):
        """A bounded in-kernel hand-off wait gave up (include/zonos_hip.h, INTEGRATION.md "Single tenant per device"): the results are void
        and the library has demoted this handle to the launches path, which has no in-launch hand-offs.  Nothing has been returned yet, so
        the generation is run once more there - unless the caller has already seen frames of it, or ZONOS_HIP_NO_TIMEOUT_RETRY=1 asks for
        the error itself (tests/conftest.py sets it for every test, so that no timeout can hide behind a repeated generation; bench.py
        counts repeats and fails on one).  Every repeat is counted (`handoff_counters`) and announced on stderr."""
        try:
            return run()
        except _lib.ZonosHipError as e:
            if "hand-off wait" not in str(e) or caller_saw_frames or os.environ.get("ZONOS_HIP_NO_TIMEOUT_RETRY") == "1":
                raise
            self._repeats += 1
            print(f"[zonos_amd] {e}\n[zonos_amd] repeating the generation on the launches path", file=sys.stderr, flush=True)
            return run()

    def _generation(self, eng, call: GenCall, ts, hooks: Hooks):
        """One generation on `eng` (held by the caller), with every launch on torch stream `ts`.  A generator: with `hooks.chunk` it yields
        (delayed codes, last column written) every `chunk` decode steps (Zonos.stream), and it returns what `call.finalise` makes of the
        codes, on the host: one tensor, or one per utterance or request of a batched call."""
        B, P, nq = call.B, call.P, self.config.codebook_dimension
        if call.ragged:
            # every row runs every step of the call: the KV capacity follows the longest prefilled row plus the call's steps
            L_c = max(L + p for L, p in zip(call.cond_lengths, call.prefix_lens)) - P
        else:
            L_c = call.cond.shape[1] if call.cond_lengths is None else max(call.cond_lengths)      # the KV capacity follows the longest VALID row
        t_total = P + call.max_new_tokens + nq
        bufs = self._kv_buffers(eng, call.engine_rows, L_c + t_total)      # (alive until zn_gen_end)
        ip = bufs.ip
        delayed = code_rows(call.prefixes, call.budgets, t_total, nq, self.masked_token_id, self.device)       # [B, nq, t_total]
        st = ts.cuda_stream
        eng.call("zn_gen_begin", B, bufs.kv_ptrs, ip.max_seqlen, ip.lengths_per_sample.data_ptr(), delayed.data_ptr(), t_total, P + 1,
                 call.max_new_tokens, float(call.cfg_scale), C.byref(call.sp), st)
        try:
            self._bind_kv_buffers(eng, bufs)
            if call.table is not None:
                eng.call("zn_gen_set_rows", call.table, B)
            if call.ragged:
                eng.call("zn_gen_set_prefix_rows", (C.c_int32 * B)(*call.prefix_lens), B)
            offset = yield from self._decode_loop(eng, ip, delayed, call, st, hooks)
        finally:
            # the device's persistent-kernel tenancy goes back once this generation's kernels have drained (include/zonos_hip.h)
            ts.synchronize()
            eng.call("zn_gen_end")
        return call.finalise(delayed, offset, nq, self.eos_token_id)

    def _finalise_row(self, delayed_row: torch.Tensor, P_b: int, max_new_tokens: int, B: int, nq: int):
        """`rows.finalise_row` with the model's EOS token: the name the tests of the serve sessions reach it by."""
        return finalise_row(delayed_row, P_b, max_new_tokens, B, nq, self.eos_token_id)

    def _decode_loop(self, eng, ip, delayed, call: GenCall, st, hooks: Hooks):
        """Prefill, first frame and the hot loop (model.py:421-509); a generator that returns the final column offset."""
        if call.ragged:
            S = self._prefill_ragged(eng, delayed, call, st)
        else:
            S = self._prefill_shared(eng, delayed, call, st)
        return (yield from self._loop_after_prefill(eng, ip, delayed, S, call, st, hooks))

    def _prefill_ragged(self, eng, delayed, call: GenCall, st) -> int:
        """generate_batch(ragged_prefix=True): row r = [cond_r[:L_b] ‖ embed(delayed_b[:, :P_b + 1]) ‖ zeros], b = r mod B, built for all rows
        by one kernel (zn_op_assemble_prefill); returns S, the longest row."""
        dev, B, cond_lengths, prefix_lens = self.device, call.B, call.cond_lengths, call.prefix_lens
        cond = call.cond.to(device=dev, dtype=torch.bfloat16).contiguous()
        R, L_c, d = cond.shape
        row_lens = [cond_lengths[r % B] + prefix_lens[r % B] + 1 for r in range(R)]
        S = max(row_lens)
        meta = torch.tensor([list(cond_lengths), list(prefix_lens)], dtype=torch.int32).to(dev)      # one host->device copy for both arrays
        hidden = torch.empty(R, S, d, dtype=torch.bfloat16, device=dev)
        row_len_dev = torch.empty(R, dtype=torch.int32, device=dev)
        eng.call("zn_op_assemble_prefill", cond.data_ptr(), L_c, meta[0].data_ptr(), delayed.data_ptr(), delayed.shape[2], meta[1].data_ptr(), B, R,
                 hidden.data_ptr(), S, row_len_dev.data_ptr(), st)
        eng.call("zn_prefill_rows", hidden.data_ptr(), S, (C.c_int32 * R)(*row_lens), st)
        return S

    def _prefill_shared(self, eng, delayed, call: GenCall, st) -> int:
        """The prefill of a call whose utterances share one audio prefix length; returns S, the longest row."""
        dev, B, prefix_conditioning, cond_lengths = self.device, call.B, call.cond, call.cond_lengths
        # prefill (generation_utils.py:236-244): [cond ‖ uncond] conditioning + embed(delayed[..., :P+1]) for both halves; without
        # guidance the B conditional rows and the embedding once (generation_utils.py:237)
        emb = self.embed_codes(delayed[..., :call.P + 1], _eng=eng)
        reps = prefix_conditioning.shape[0] // B
        hidden = torch.cat([prefix_conditioning.to(device=dev, dtype=torch.bfloat16), emb.repeat(reps, 1, 1)], dim=1).contiguous()
        S = hidden.shape[1]
        if cond_lengths is None:
            eng.call("zn_prefill", hidden.data_ptr(), S, st)
        else:
            # right-padded rows: row r = [cond_r[:L_r] ‖ emb_r ‖ padding] (the padding keeps whatever the caller's tensor holds there: it is never read)
            L_c, E, L_max = prefix_conditioning.shape[1], emb.shape[1], max(cond_lengths)
            embr = emb.repeat(reps, 1, 1)
            for r in range(hidden.shape[0]):
                L = cond_lengths[r % B]
                if L < L_c:
                    tail = hidden[r, L:L_c].clone()
                    hidden[r, L:L + E] = embr[r]
                    hidden[r, L + E:] = tail
            S = L_max + E
            hidden = hidden[:, :S].contiguous()
            row_len = (C.c_int32 * hidden.shape[0])(*[cond_lengths[r % B] + E for r in range(hidden.shape[0])])
            eng.call("zn_prefill_rows", hidden.data_ptr(), S, row_len, st)
        return S

    def _loop_after_prefill(self, eng, ip, delayed, S, call: GenCall, st, hooks: Hooks):
        """First frame and the hot loop (model.py:423-509), the prefill of S positions done; a generator that returns the final column
        offset.  With `hooks.chunk`, the steps are enqueued at least every `chunk` steps and it yields (delayed, column offset written
        last) there.  The stop flag is checked with the cadence of `call.cadence` utterances."""
        B, cadence, nq, offset, t_total = call.B, call.cadence, delayed.shape[1], call.P + 1, delayed.shape[2]
        callback, _trace, chunk = hooks.callback, hooks.trace, hooks.chunk
        eng.call("zn_sample_first", st)
        ip.seqlen_offset += S
        if _trace is not None:
            _trace.setdefault("logits", []).append(self._step_logits(eng, B, nq))
            if _trace.get("after_step") is not None:
                _trace["after_step"](-1, delayed, offset)
        # hot loop with the reference's stop-check cadence (tensor_ops.py:84-105)
        max_steps = t_total - offset
        frame = delayed[..., offset:offset + 1]
        pending, done = 0, C.c_int32(0)
        # Without a callback the stop flag of check k is read after the steps up to check k + 1 have been enqueued (the device ->
        # host round trip leaves the critical path); a stop seen late rolls `offset` back to the check that saw it, and the
        # over-run steps have only written columns beyond that cut.
        deferred = callback is None and _trace is None
        begun_at = None                                            # offset at the check whose read-back is in flight
        for step_idx in range(max_steps):
            offset += 1
            if offset >= t_total:
                break
            pending += 1
            ip.seqlen_offset += 1
            check = stop_check_at(step_idx, cadence)
            hook = chunk is not None and step_idx % chunk == chunk - 1
            if check or hook or callback is not None or _trace is not None:
                eng.call("zn_decode_steps", pending, st)
                pending = 0
                if _trace is not None:
                    _trace["logits"].append(self._step_logits(eng, B, nq))
                    hook = _trace.get("after_step")
                    if hook is not None:
                        hook(step_idx, delayed, offset)
                        eng.call("zn_codes_changed")        # the hook may rewrite the column the next step embeds
            if check and deferred:
                if begun_at is not None:
                    eng.call("zn_all_stopped_end", C.byref(done))
                    if done.value:
                        offset, begun_at = begun_at, None
                        break
                eng.call("zn_all_stopped_begin", st)
                begun_at = offset
            elif check:
                eng.call("zn_all_stopped", C.byref(done), st)
                if done.value:
                    break
            if callback is not None and not callback(frame, step_idx + 1, max_steps):
                break
            if hook:
                yield delayed, offset
        if pending:
            eng.call("zn_decode_steps", pending, st)
        if begun_at is not None:
            eng.call("zn_all_stopped_end", C.byref(done))
            if done.value:
                offset = begun_at
        eng.call("zn_all_stopped", C.byref(done), st)      # also surfaces a timed-out in-kernel hand-off of the last steps
        return offset

    def _step_logits(self, eng: HipEngine, B: int, nq: int) -> torch.Tensor:
        buf = torch.empty(B, nq, 1025, dtype=torch.float32, device=self.device)
        eng.call("zn_get_step_outputs", buf.data_ptr(), None, eng.stream())
        return buf

