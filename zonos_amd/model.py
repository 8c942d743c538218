"""`Zonos` — the reference's model surface (zonos/model.py:43-548) over the MI355X HIP path.

Kept API: `Zonos.from_pretrained / from_local / setup_cache / embed_codes / apply_heads / generate`, attributes
`config, backbone, embeddings, fused_heads, autoencoder, device`.  The hot loop (model.py:467-502) runs as one
hipGraph replay per step inside libzonos_hip.so; the host only mirrors the reference's stop-check cadence
(tensor_ops.py:90-103) and the post-processing (model.py:511-539).
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import threading
import time
import json
from dataclasses import dataclass, field
from typing import Callable, Iterator, NamedTuple, Sequence

import torch
import torch.nn as nn

from . import _lib
from .autoencoder import DACAutoencoder
from .backbone import BACKBONES, HipEngine
from .codebook_pattern import apply_delay_pattern, revert_delay_pattern
from .conditioning import ConditioningCache, PrefixConditioner, pad_conditioning_rows, pad_conditionings, prepare_conditioning_with_cache
from .config import InferenceParams, ZonosConfig
from .serving import (ServeChunk, ServeResult, SlotScheduler, StreamLedger, check_serve_request, release_limit, row_end_offset,  # noqa: F401
                      serve_slack, stop_check_at)     # (release_limit, row_end_offset, stop_check_at: defined there, used and re-exported here)
from .utils import DEFAULT_DEVICE, find_multiple

DEFAULT_BACKBONE_CLS = next(iter(BACKBONES.values()))

_SAMPLING_DEFAULTS = dict(temperature=1.0, top_p=0.0, top_k=0, min_p=0.0, linear=0.0, conf=0.0, quad=0.0,
                          repetition_penalty=3.0, repetition_penalty_window=2)   # zonos/sampling.py:166-178


def _sampling_struct(params: dict, seed: int) -> _lib.zn_sampling:
    unknown = set(params) - set(_SAMPLING_DEFAULTS)
    if unknown:
        raise TypeError(f"sample_from_logits() got unexpected keyword arguments {sorted(unknown)}")
    p = {**_SAMPLING_DEFAULTS, **params}
    return _lib.zn_sampling(temperature=p["temperature"], top_p=p["top_p"], top_k=int(p["top_k"]), min_p=p["min_p"],
                            linear=p["linear"], conf=p["conf"], quad=p["quad"], repetition_penalty=p["repetition_penalty"],
                            repetition_penalty_window=int(p["repetition_penalty_window"]), seed=seed & (2 ** 64 - 1))


class StreamChunk(NamedTuple):
    """One step of `Zonos.stream`: the frames that became final (int64 [1, 9, k], as `generate()` returns them) and the samples they
    completed (float32 [1, 1, m] on the model's device).  k or m may be 0, never both."""
    codes: torch.Tensor
    wav: torch.Tensor


def map_codes(out: torch.Tensor) -> torch.Tensor:
    """model.py:530-539: EOS / mask tokens to codes, clamped to the codebook."""
    out = torch.where(out > 1024, 512, out)
    out = torch.where(out == 1024, 0, out)
    return torch.clamp(out, 0, 1023)


def finalise_codes(out: torch.Tensor, offset: int, nq: int, eos_id: int) -> torch.Tensor:
    """model.py:511-539 on the reverted codes [B, nq, audio_len] of a generation whose loop ended at column `offset`: the EOS boundary
    search over the last min(50, valid_length // 4) frames, then the code mapping.  `generate()` and `stream()` both end here."""
    valid_length = offset - nq
    window = min(50, valid_length // 4)
    for pos in range(max(0, valid_length - window), valid_length):   # model.py:516-528
        if int((out[:, :, pos] == eos_id).sum()) >= nq // 2:
            valid_length = pos
            break
    return map_codes(out[..., :valid_length])


@dataclass
class GenRequest:
    """One utterance of `Zonos.generate_batch`: `generate()`'s per-call arguments, per request.  `conditioning` is what
    `prepare_conditioning` returns for the utterance: [2, L, d] = [cond ‖ uncond], or [1, L, d] when cfg_scale == 1."""
    conditioning: torch.Tensor
    sampling_params: dict = field(default_factory=lambda: dict(min_p=0.1))
    seed: int | None = None
    cfg_scale: float = 2.0
    max_new_tokens: int = 86 * 30
    audio_prefix_codes: torch.Tensor | None = None


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
        c = r.conditioning
        halves = call_halves if call_halves is not None else (2 if float(r.cfg_scale) != 1.0 else 1)
        if c.dim() != 3 or c.shape[0] != halves or c.shape[1] < 1 or c.shape[2] != d_model:
            raise ValueError(f"generate_batch: request {i}: conditioning of shape {tuple(c.shape)}, expected [{halves}, L >= 1, {d_model}] at "
                             f"cfg_scale={r.cfg_scale}")
        if int(r.max_new_tokens) != r.max_new_tokens or int(r.max_new_tokens) < 1:
            raise ValueError(f"generate_batch: request {i}: max_new_tokens must be a positive integer, got {r.max_new_tokens}")
        a = r.audio_prefix_codes
        if a is not None and (a.dim() != 3 or a.shape[0] != 1 or a.shape[1] != nq):
            raise ValueError(f"generate_batch: request {i}: audio_prefix_codes of shape {tuple(a.shape)}, expected [1, {nq}, P]")
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
                   mlp_weights: str = "bf16") -> "Zonos":
        """model.py:128-176: bf16 model, embeddings zero-padded to the 1032-row tables, heads.{i} fused.  mlp_weights="fp8":
        quantize_mlp_fp8() after loading (lossy with respect to the checkpoint; see there); the default changes nothing."""
        import safetensors
        if mlp_weights not in ("bf16", "fp8"):
            raise _lib.ZonosHipError(f"mlp_weights must be 'bf16' or 'fp8', not {mlp_weights!r}")
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
        return model

    @torch.inference_mode()
    def quantize_mlp_fp8(self) -> "Zonos":
        """Weight-only FP8 for fc1 / fc2 of every transformer block (zonos_amd/quant.py: E4M3 codes, one power-of-two scale per weight
        row).  Quantises on the device, OVERWRITES the bf16 parameters in place with the dequantised values and keeps the codes and
        exponents as buffers of the block's mlp (fc1_q, fc1_exp, fc2_q, fc2_exp; not part of the state dict).  Decode steps of 5 or
        more rows then stream the codes - half the bytes - and compute exactly what the bf16 kernels compute on the dequantised
        weights, which every other path keeps reading.  Lossy with respect to the checkpoint (|Wdq - w| <= 2^-4 |w|), exact with
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
        return self

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
        return HipEngine(self.backbone, [m.weight for m in self.embeddings], self.fused_heads.weight,
                         max_rows=2 * batch_size, double_out_proj=getattr(self.backbone, "ref_double_out_proj", True),
                         n_codebooks=self.autoencoder.num_codebooks, vocab_head=1025, vocab_embed=self.embeddings[0].weight.shape[0],
                         eos_id=self.eos_token_id, mask_id=self.masked_token_id)

    def engine(self, batch_size: int = 1) -> HipEngine:
        # (both handles are created and replaced under one lock: two threads arriving together must not each build an engine,
        # nor drop the spare another thread is about to take)
        with self._spare_guard:
            e = self._engine
            if e is None or e.max_rows < 2 * batch_size or e.device != self.device:
                self._engine = e = self._new_engine(batch_size)
                self._spare = None
            return e

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
        B = batch_size
        n = self._check_rows(prefix_conditioning, cfg_scale, B, conditioning_lengths)
        dev = self.device
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        # an engine's handle holds this generation's state: a third concurrent generate() call on one model queues here.  Engines are
        # sized by rows (engine(b) holds 2 b): one unguided utterance runs on engine(1), like a guided one
        eng = self._acquire_engine((n + 1) // 2)
        try:
            return self._generate_on(eng, dev, prefix_conditioning, audio_prefix_codes, max_new_tokens, cfg_scale, B, sampling_params, callback, seed, _trace,
                                     None if conditioning_lengths is None else [int(v) for v in conditioning_lengths])
        finally:
            eng.generating = False
            eng.lock.release()

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
        if self.device.type != "cuda":
            raise _lib.ZonosHipError("zonos_amd runs on MI355X only: move the model to a cuda device (no CPU fallback)")
        return n

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
        reqs = list(requests)
        nq = self.config.codebook_dimension
        guided, P = check_requests(reqs, nq, self.config.backbone.d_model, ragged_prefix, mixed_guidance)
        prefix_lens = None
        if ragged_prefix:
            prefix_lens, P = P, max(P)
        if guided is None:
            return self._generate_mixed(reqs, P, prefix_lens, _trace)
        if len(reqs) == 1:
            r = reqs[0]
            return [self.generate(r.conditioning, r.audio_prefix_codes, int(r.max_new_tokens), r.cfg_scale, 1, r.sampling_params, seed=r.seed,
                                  _trace=_trace)]
        B, dev = len(reqs), self.device
        cond, lengths = pad_conditionings([r.conditioning.to(dev) for r in reqs], 2.0 if guided else 1.0)
        self._check_rows(cond, 2.0 if guided else 1.0, B, lengths)
        if prefix_lens is not None:
            prefix = [r.audio_prefix_codes for r in reqs]          # per request, None or [1, nq, P_b]
        else:
            prefix = None if P == 0 else torch.cat([r.audio_prefix_codes.to(dev) for r in reqs], 0)
        table = (_lib.zn_row_params * B)()
        for b, r in enumerate(reqs):
            seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if r.seed is None else r.seed
            table[b].sp = _sampling_struct(r.sampling_params, seed)
            table[b].cfg_scale, table[b].max_new_tokens = float(r.cfg_scale), int(r.max_new_tokens)
        max_new = max(int(r.max_new_tokens) for r in reqs)
        eng = self._acquire_engine((cond.shape[0] + 1) // 2)
        try:
            with torch.cuda.device(dev):
                # zn_gen_begin's own cfg_scale and sampling parameters only fix the row layout: every sampler reads the table
                run = lambda: _drain(self._generation(eng, cond, prefix, max_new, 2.0 if guided else 1.0, B, reqs[0].sampling_params, None, 0, _trace,
                                                      torch.cuda.current_stream(dev), None, lengths, table, prefix_lens))
                outs = self._with_timeout_policy(run, caller_saw_frames=_trace is not None)
            return [o.to(dev) for o in outs]
        finally:
            eng.generating = False
            eng.lock.release()

    def _generate_mixed(self, reqs, P, prefix_lens, _trace) -> list[torch.Tensor]:
        """generate_batch(mixed_guidance=True) with both kinds of request present: a call of R rows in the unguided layout."""
        dev = self.device
        cond, lengths, first = pad_conditioning_rows([r.conditioning.to(dev) for r in reqs])
        R = cond.shape[0]
        self._check_rows(cond, 1.0, R, lengths)
        owner = [i for i, r in enumerate(reqs) for _ in range(r.conditioning.shape[0])]          # row -> request
        if prefix_lens is not None:
            prefix, prefix_lens = [reqs[i].audio_prefix_codes for i in owner], [prefix_lens[i] for i in owner]
        else:
            prefix = None if P == 0 else torch.cat([reqs[i].audio_prefix_codes.to(dev) for i in owner], 0)
        table = (_lib.zn_row_params * R)()
        for i, r in enumerate(reqs):
            seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if r.seed is None else r.seed
            for u in range(first[i], first[i] + r.conditioning.shape[0]):
                table[u].sp = _sampling_struct(r.sampling_params, seed)
                table[u].cfg_scale, table[u].max_new_tokens = float(r.cfg_scale), int(r.max_new_tokens)
                if r.conditioning.shape[0] == 2:
                    table[u].reserved[0], table[u].reserved[1] = first[i] + 1, first[i] + 2       # (cond_row + 1, uncond_row + 1)
        max_new = max(int(r.max_new_tokens) for r in reqs)
        eng = self._acquire_engine((R + 1) // 2)
        try:
            with torch.cuda.device(dev):
                run = lambda: _drain(self._generation(eng, cond, prefix, max_new, 1.0, R, reqs[0].sampling_params, None, 0, _trace,
                                                      torch.cuda.current_stream(dev), None, lengths, table, prefix_lens, first))
                outs = self._with_timeout_policy(run, caller_saw_frames=_trace is not None)
            return [o.to(dev) for o in outs]
        finally:
            eng.generating = False
            eng.lock.release()

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
        slots, sched_every, max_prompt, max_new_tokens = int(slots), int(sched_every), int(max_prompt), int(max_new_tokens)
        if not 1 <= slots <= MAX_BATCH_REQUESTS:
            raise ValueError(f"serve: slots must lie in 1..{MAX_BATCH_REQUESTS}, got {slots}")
        if sched_every < 1 or max_prompt < 1 or max_new_tokens < 1:
            raise ValueError(f"serve: sched_every={sched_every}, max_prompt={max_prompt}, max_new_tokens={max_new_tokens} must all be >= 1")
        if self.device.type != "cuda":
            raise _lib.ZonosHipError("zonos_amd runs on MI355X only: move the model to a cuda device (no CPU fallback)")
        dev = self.device
        return self._serve_gen(dev, torch.cuda.current_stream(dev), iter(requests), slots, max_prompt, max_new_tokens, None if guided is None else bool(guided), sched_every, _trace, _stats)

    def serve_stream(self, requests, slots: int = 8, max_prompt: int = 64, max_new_tokens: int = 86 * 30, guided: bool | None = True,
                     sched_every: int = 8, chunk_frames: int = 16, _stats: dict | None = None) -> Iterator[ServeChunk]:
        """`serve()` with audio as it happens: a generator of `ServeChunk(index, codes, wav, done, error)`.  The session is `serve()`'s -
        the same admissions, steps and retirements.  At a scheduling point every busy slot whose final frames (`release_limit` of its
        own column) have grown by at least `chunk_frames` since its last chunk yields them with the samples the DAC can decode from
        them, and every request retired there yields its last chunk (done=True): what `_finalise_row` keeps beyond the frames released.
        The windows of all slots are decoded in one ragged pass (`DACAutoencoder.stream_set`, zn_dac_decode_spans) on the session's
        stream.  For every request the concatenated codes equal the `ServeResult.codes` of `serve()` for the same source and settings,
        and the concatenated wav `autoencoder.decode()` of them, bit for bit.  A refused request yields
        ServeChunk(index, None, None, True, ValueError).  The engine is held as by `serve()`; `_stats` as there."""
        if int(chunk_frames) < 1:
            raise ValueError(f"serve_stream: chunk_frames must be >= 1, got {chunk_frames}")
        slots, sched_every, max_prompt, max_new_tokens = int(slots), int(sched_every), int(max_prompt), int(max_new_tokens)
        if not 1 <= slots <= MAX_BATCH_REQUESTS:
            raise ValueError(f"serve_stream: slots must lie in 1..{MAX_BATCH_REQUESTS}, got {slots}")
        if sched_every < 1 or max_prompt < 1 or max_new_tokens < 1:
            raise ValueError(f"serve_stream: sched_every={sched_every}, max_prompt={max_prompt}, max_new_tokens={max_new_tokens} must all be >= 1")
        if self.device.type != "cuda":
            raise _lib.ZonosHipError("zonos_amd runs on MI355X only: move the model to a cuda device (no CPU fallback)")
        dev = self.device
        return self._serve_gen(dev, torch.cuda.current_stream(dev), iter(requests), slots, max_prompt, max_new_tokens, None if guided is None else bool(guided), sched_every, None,
                               _stats, int(chunk_frames))

    def _serve_gen(self, dev, ts, source, slots, max_prompt, max_new_tokens, guided, sched_every, _trace, _stats=None, chunk_frames=None):
        """The session of serve() (chunk_frames None: yields ServeResult) and of serve_stream() (yields ServeChunk)."""
        nq, d, mask = self.config.codebook_dimension, self.config.backbone.d_model, self.masked_token_id
        mixed = guided is None                                         # rows in the unguided layout; a guided request holds two of them
        halves = 2 if guided else 1
        R = slots * halves
        slack = serve_slack(sched_every)
        width = max_prompt + max_new_tokens + nq + slack              # columns of a slot's row of the code buffer
        sched = SlotScheduler(slots, nq, sched_every)
        streaming = chunk_frames is not None
        ledger = StreamLedger(nq, chunk_frames, self.eos_token_id) if streaming else None
        dacs = self.autoencoder.stream_set(ts) if streaming else None
        eng = self._acquire_engine((R + 1) // 2)
        begun = False
        st = ts.cuda_stream
        try:
            with torch.inference_mode(), torch.cuda.device(dev), torch.cuda.stream(ts):
                ip = self.setup_cache(batch_size=R, max_seqlen=max_prompt + max_new_tokens + nq + slack)
                max_len = ip.max_seqlen
                delayed = torch.full((slots, nq, width), mask, dtype=torch.int32, device=dev)      # an idle slot's cells are never -1
                n_layer = self.config.backbone.n_layer
                kv_ptrs = (C.c_void_p * n_layer)(*[ip.key_value_memory_dict[i][0].data_ptr() for i in range(n_layer)])
                sp = _sampling_struct({}, 0)                           # (every sampler of a session reads its slot's entry)
                eng.call("zn_gen_begin", slots, kv_ptrs, max_len, ip.lengths_per_sample.data_ptr(), delayed.data_ptr(), width, 1, max_new_tokens,
                         2.0 if guided else 1.0, C.byref(sp), st)
                begun = True
                eng.call("zn_gen_open_slots", slack)

            def accept(r):
                if not isinstance(r, GenRequest):
                    raise ValueError(f"serve: expected a GenRequest or None, got {type(r).__name__}")
                c, a = r.conditioning, r.audio_prefix_codes
                if not hasattr(c, "shape") or (a is not None and not hasattr(a, "shape")):
                    raise ValueError("serve: conditioning and audio_prefix_codes must be tensors")
                L, P = check_serve_request(c.shape, None if a is None else a.shape, r.max_new_tokens, r.cfg_scale, nq=nq, d_model=d, guided=guided,
                                           max_len=max_len, width=width, slack=slack)
                try:
                    _sampling_struct(r.sampling_params, 0)
                except TypeError as e:
                    raise ValueError(f"serve: {e}") from None
                return P, int(r.max_new_tokens), (2 if mixed and float(r.cfg_scale) != 1.0 else 1)

            def record(kind, holders):
                if _trace is not None:
                    _trace.setdefault("logits", []).append(self._step_logits(eng, slots, nq))
                    _trace.setdefault("slots", []).append((kind, sched.step, list(holders)))

            def admit(admitted):
                # one entry per admitted row: (slot, request, conditioning rows of that slot).  A two-slot request of a mixed session gives
                # two entries, its conditional row into its owner slot and its unconditional one into the partner, both naming the pair.
                entries = []
                for slot, _, r in admitted:
                    c, f = r.conditioning.to(dev), sched.partner(slot)
                    if f is None:
                        entries.append((slot, r, c, None))
                    else:
                        entries += [(slot, r, c[0:1], (slot, f)), (f, r, c[1:2], (slot, f))]
                n = len(entries)
                Ls = [int(c.shape[1]) for _, _, c, _ in entries]
                Ps = [0 if r.audio_prefix_codes is None else int(r.audio_prefix_codes.shape[2]) for _, r, _, _ in entries]
                cond, _ = pad_conditionings([c for _, _, c, _ in entries], 2.0 if guided else 1.0)
                cond = cond.to(device=dev, dtype=torch.bfloat16).contiguous()
                codes = torch.full((n, nq, width - nq), mask, dtype=torch.int32, device=dev)
                for j, (_, r, _, _) in enumerate(entries):            # a slot's row: its prefix, its unknown cells, the mask token up to the width
                    if Ps[j]:
                        codes[j, :, :Ps[j]] = r.audio_prefix_codes[0].to(device=dev, dtype=torch.int32)
                    codes[j, :, Ps[j]:Ps[j] + int(r.max_new_tokens)] = -1
                rows = apply_delay_pattern(codes, mask).contiguous()  # [n, nq, width]
                adm = (_lib.zn_admit * n)()
                seeds = {}
                for j, (slot, r, _, pair) in enumerate(entries):
                    delayed[slot].copy_(rows[j])
                    if id(r) not in seeds:
                        seeds[id(r)] = int(torch.randint(0, 2 ** 62, (1,)).item()) if r.seed is None else r.seed
                    adm[j].slot, adm[j].row_len, adm[j].prefix_len = slot, Ls[j] + Ps[j] + 1, Ps[j]
                    adm[j].params.sp = _sampling_struct(r.sampling_params, seeds[id(r)])
                    adm[j].params.cfg_scale, adm[j].params.max_new_tokens = float(r.cfg_scale), int(r.max_new_tokens)
                    if pair is not None:
                        adm[j].params.reserved[0], adm[j].params.reserved[1] = pair[0] + 1, pair[1] + 1
                S = max(L + P + 1 for L, P in zip(Ls, Ps))
                meta = torch.tensor([Ls, Ps], dtype=torch.int32).to(dev)
                hidden = torch.empty(halves * n, S, d, dtype=torch.bfloat16, device=dev)
                row_len_dev = torch.empty(halves * n, dtype=torch.int32, device=dev)
                eng.call("zn_op_assemble_prefill", cond.data_ptr(), cond.shape[1], meta[0].data_ptr(), rows.data_ptr(), width, meta[1].data_ptr(), n,
                         halves * n, hidden.data_ptr(), S, row_len_dev.data_ptr(), st)
                eng.call("zn_gen_admit", adm, n, hidden.data_ptr(), S, st)
                held = [None] * slots
                for slot, index, _ in admitted:
                    held[slot] = index
                    if sched.partner(slot) is not None:
                        held[sched.partner(slot)] = index
                record("admit", held)
                for slot, index, r in admitted:
                    if streaming:
                        ledger.open(slot, 0 if r.audio_prefix_codes is None else int(r.audio_prefix_codes.shape[2]), int(r.max_new_tokens))
                    if _stats is not None:
                        _stats.setdefault("admitted_at", {})[index] = time.perf_counter()

            rem, own = (C.c_int32 * slots)(), (C.c_int32 * slots)()
            while True:
                out = []
                with torch.inference_mode(), torch.cuda.device(dev), torch.cuda.stream(ts):
                    admitted, refused = sched.pull(source, accept)
                    out += [ServeChunk(index, None, None, True, err) if streaming else ServeResult(index, None, err) for index, err in refused]
                    if admitted:
                        timed = _stats is not None and _stats.get("time_admissions")
                        if timed:
                            ts.synchronize()
                            t0 = time.perf_counter()
                        admit(admitted)
                        if timed:
                            ts.synchronize()
                            _stats["admit_seconds"] = _stats.get("admit_seconds", 0.0) + time.perf_counter() - t0
                        if _stats is not None:
                            _stats["admissions"] = _stats.get("admissions", 0) + 1
                            _stats["admitted"] = _stats.get("admitted", 0) + len(admitted)
                    stop = sched.finished()
                    if not stop and not sched.all_idle():
                        if _trace is None:
                            eng.call("zn_decode_steps", sched_every, st)
                            sched.advance()
                        else:
                            for _ in range(sched_every):
                                eng.call("zn_decode_steps", 1, st)
                                sched.advance(1)
                                record("step", sched.holders())
                        if _stats is not None:
                            _stats["steps"] = sched.step
                        eng.call("zn_gen_row_state", rem, own, st)
                        if [own[b] for b in range(slots)] != [sched.own_steps(b) for b in range(slots)]:
                            raise _lib.ZonosHipError(f"serve: the device counts {list(own)} steps per slot, the scheduler {[sched.own_steps(b) for b in range(slots)]}")
                        if streaming:                      # codebook 0 of the columns that decide a slot's EOS frame: one gather, one read-back
                            cells = ledger.cells(own)
                            if cells:
                                flat = [b * nq * width + c for b, lo, hi in cells for c in range(lo, hi)]
                                toks = delayed.view(-1)[torch.tensor(flat, dtype=torch.int64).to(dev)].cpu().tolist()
                                for b, lo, hi in cells:
                                    ledger.scan(b, lo, toks[:hi - lo])
                                    del toks[:hi - lo]
                        rows_host = {}
                        for b in sched.wants_eos(rem):
                            rows_host[b] = delayed[b:b + 1].cpu()
                            r = sched.rows[b]
                            sched.set_eos(b, self._finalise_row(rows_host[b], r.prefix_len, r.max_new_tokens, slots, nq)[1])
                        known = {b: sched.rows[b] for b in range(slots) if sched.rows[b] is not None}
                        tails = {}
                        for b, index, end in sched.due():
                            row = rows_host[b] if b in rows_host else delayed[b:b + 1].cpu()
                            codes, _, end_b = self._finalise_row(row, known[b].prefix_len, known[b].max_new_tokens, slots, nq)
                            assert end_b == end, (end_b, end)
                            held = [b] if known[b].partner is None else [b, known[b].partner]
                            if mixed and _trace is not None:
                                _trace.setdefault("retired", []).append((index, held, delayed[held].cpu()))
                            for slot in held:                          # a guided request of a mixed session leaves both of its rows at once
                                eng.call("zn_gen_retire", slot)
                            if streaming:
                                tails[index] = codes[..., ledger.close(b, codes.shape[2]):].to(dev)
                            else:
                                out.append(ServeResult(index, codes.to(dev), None))
                        if streaming:
                            # the frames that became final in the rows that run on, built on the device; then every window in one DAC pass
                            pieces = {known[b].index: map_codes(revert_delay_pattern(delayed[b:b + 1, :, lo:hi + nq].to(torch.int64)))
                                      for b, lo, hi in ledger.take(own)}
                            wavs = dacs.push({**pieces, **tails}, end=set(tails))
                            out += [ServeChunk(index, c, wavs[index], False, None) for index, c in pieces.items()]
                            out += [ServeChunk(index, c, wavs[index], True, None) for index, c in tails.items()]
                for res in out:
                    yield res
                if stop:
                    break
        finally:
            try:
                if begun:
                    ts.synchronize()
                    eng.call("zn_gen_end")
            finally:
                eng.generating = False
                eng.lock.release()

    def stream(self, prefix_conditioning: torch.Tensor, audio_prefix_codes: torch.Tensor = None, max_new_tokens: int = 86 * 30,
               cfg_scale: float = 2.0, sampling_params: dict = dict(min_p=0.1), seed: int | None = None, chunk_frames: int = 16,
               batch_size: int = 1) -> Iterator[StreamChunk]:
        """`generate()` + `autoencoder.decode()` as they happen: a generator of `StreamChunk(codes, wav)`.  Every `chunk_frames` decode steps
        it yields the frames that have become final (`release_limit`) and the samples the DAC can decode from them (`DACAutoencoder.stream`);
        the rest comes when the generation ends.  With the same arguments and seed, the concatenated codes equal `generate(...)` and the
        concatenated wav `autoencoder.decode(generate(...))`, bit for bit.  Batch size 1 (guided, or cfg_scale=1).

        The generation's engine and the device's persistent-kernel tenancy are held while the generator is alive; `close()`, leaving a for
        loop early or garbage collection releases them.  Every launch (decode steps and DAC) goes to the stream current when stream() is
        called.  A hand-off timeout raises: it is not repeated on the launches path, as the caller may already hold audio."""
        if batch_size != 1:
            raise ValueError(f"stream() generates one utterance at a time, got batch_size={batch_size}")
        if int(chunk_frames) < 1:
            raise ValueError(f"chunk_frames must be >= 1, got {chunk_frames}")
        n = self._check_rows(prefix_conditioning, cfg_scale, 1)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        dev = self.device
        return self._stream_gen(dev, torch.cuda.current_stream(dev), (n + 1) // 2, prefix_conditioning, audio_prefix_codes, max_new_tokens,
                                cfg_scale, sampling_params, seed, int(chunk_frames))

    def _stream_gen(self, dev, ts, rows, prefix_conditioning, audio_prefix_codes, max_new_tokens, cfg_scale, sampling_params, seed, chunk):
        nq, eos = self.config.codebook_dimension, self.eos_token_id
        eng = self._acquire_engine(rows)
        gen, held = None, [True]

        def release():
            if not held[0]:
                return
            held[0] = False
            try:
                if gen is not None:
                    with torch.cuda.device(dev), torch.cuda.stream(ts):
                        gen.close()                        # a stream left early: its steps drain, zn_gen_end
            finally:
                eng.generating = False
                eng.lock.release()
        try:
            # (each stretch between two yields runs with the generation's device and stream current, and leaves the caller's as it found them)
            with torch.inference_mode(), torch.cuda.device(dev), torch.cuda.stream(ts):
                dac = self.autoencoder.stream(ts)
                gen = self._generation(eng, prefix_conditioning, audio_prefix_codes, max_new_tokens, cfg_scale, 1, sampling_params, None, seed,
                                       None, ts, chunk)
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
            release()                                      # the generation has ended: the engine is free before the last chunk goes out
            if chunk_out is not None:
                yield chunk_out
        finally:
            release()

    def _generate_on(self, eng, dev, prefix_conditioning, audio_prefix_codes, max_new_tokens, cfg_scale, B, sampling_params, callback, seed, _trace,
                     cond_lengths=None):
        with torch.cuda.device(dev):
            run = lambda: self._generate_locked(eng, prefix_conditioning, audio_prefix_codes, max_new_tokens, cfg_scale, B, sampling_params, callback,
                                                seed, _trace, cond_lengths)
            return self._with_timeout_policy(run, caller_saw_frames=callback is not None or _trace is not None)

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

    def _generate_locked(self, eng, prefix_conditioning, audio_prefix_codes, max_new_tokens, cfg_scale, batch_size, sampling_params, callback, seed,
                         _trace, cond_lengths=None):
        return _drain(self._generation(eng, prefix_conditioning, audio_prefix_codes, max_new_tokens, cfg_scale, batch_size, sampling_params, callback,
                                       seed, _trace, torch.cuda.current_stream(self.device), None, cond_lengths)).to(self.device)

    def _generation(self, eng, prefix_conditioning, audio_prefix_codes, max_new_tokens, cfg_scale, batch_size, sampling_params, callback, seed,
                    _trace, ts, chunk, cond_lengths=None, row_table=None, prefix_lens=None, request_rows=None):
        """One generation on `eng` (its lock held by the caller), with every launch on torch stream `ts`.  A generator: with `chunk` it yields
        (delayed codes, last column written) every `chunk` decode steps (Zonos.stream), and it returns the final codes on the host.  With
        `row_table` (zn_row_params per utterance, generate_batch) it returns one tensor per utterance.  With `prefix_lens` (generate_batch's
        ragged_prefix; needs `row_table` and `cond_lengths`) `audio_prefix_codes` is a list of per-utterance prefixes (None or [1, nq, P_b]).
        With `request_rows` (generate_batch's mixed_guidance; needs `row_table`) the utterances are the rows of a mixed call: the loop checks
        its stop flag with the cadence of a call of len(request_rows) requests, and one tensor per request is returned, read from the row
        `request_rows` names for it."""
        dev = self.device
        B, nq = batch_size, self.config.codebook_dimension
        cadence = B if request_rows is None else len(request_rows)
        R = prefix_conditioning.shape[0]                          # 2B with guidance, B when cfg_scale == 1 (checked by generate)
        if prefix_lens is not None:
            P = max(prefix_lens)
            # every row runs every step of the call: the KV capacity follows the longest prefilled row plus the call's steps
            L_c = max(L + p for L, p in zip(cond_lengths, prefix_lens)) - P
        else:
            P = 0 if audio_prefix_codes is None else audio_prefix_codes.shape[2]
            L_c = prefix_conditioning.shape[1] if cond_lengths is None else max(cond_lengths)      # the KV capacity follows the longest VALID row
        audio_len = P + max_new_tokens
        seq_len = L_c + audio_len + nq
        ip = self.setup_cache(batch_size=R, max_seqlen=seq_len)
        codes = torch.full((B, nq, audio_len), -1, dtype=torch.int32, device=dev)
        if prefix_lens is not None:
            # row b is left-aligned in its own buffer row: its P_b prefix frames, its unknown cells (below), the mask token up to the width
            for b, a in enumerate(audio_prefix_codes):
                if prefix_lens[b]:
                    codes[b, :, :prefix_lens[b]] = a[0].to(device=dev, dtype=torch.int32)
        elif audio_prefix_codes is not None:
            codes[..., :P] = audio_prefix_codes.to(device=dev, dtype=torch.int32)
        if row_table is not None:
            # a row's cells beyond its own budget hold the mask token, as the delay pattern of a generation of that length leaves them:
            # they are never written, and the steps that run past the row's end embed what its own generation would have embedded
            for b in range(B):
                codes[b, :, (P if prefix_lens is None else prefix_lens[b]) + int(row_table[b].max_new_tokens):] = self.masked_token_id
        delayed = apply_delay_pattern(codes, self.masked_token_id).contiguous()       # [B, nq, audio_len + nq]
        t_total = delayed.shape[2]
        offset = P + 1
        st = ts.cuda_stream
        sp = _sampling_struct(sampling_params, seed)
        kv_ptrs = (C.c_void_p * self.config.backbone.n_layer)(*[ip.key_value_memory_dict[i][0].data_ptr() for i in range(self.config.backbone.n_layer)])
        eng.call("zn_gen_begin", B, kv_ptrs, ip.max_seqlen, ip.lengths_per_sample.data_ptr(), delayed.data_ptr(), t_total, offset,
                 max_new_tokens, float(cfg_scale), C.byref(sp), st)
        try:
            if row_table is not None:
                eng.call("zn_gen_set_rows", row_table, B)
            if prefix_lens is not None:
                eng.call("zn_gen_set_prefix_rows", (C.c_int32 * B)(*prefix_lens), B)
            offset = yield from self._decode_loop(eng, ip, delayed, prefix_conditioning, offset, t_total, B, nq, callback, _trace, st, chunk, cond_lengths,
                                                  prefix_lens, cadence)
        finally:
            # the device's persistent-kernel tenancy goes back once this generation's kernels have drained (include/zonos_hip.h)
            ts.synchronize()
            eng.call("zn_gen_end")
        if request_rows is not None:
            host = delayed.cpu()
            return [self._finalise_row(host[u:u + 1], P if prefix_lens is None else int(prefix_lens[u]), int(row_table[u].max_new_tokens), cadence, nq)[0]
                    for u in request_rows]
        if row_table is not None:
            return self._finalise_rows(delayed.cpu(), row_table, P if prefix_lens is None else prefix_lens, B, nq)       # the same one device->host copy
        out = revert_delay_pattern(delayed.to(torch.int64)).cpu()     # one device->host copy (model.py:511)
        return finalise_codes(out, offset, nq, self.eos_token_id)

    def _finalise_rows(self, delayed: torch.Tensor, row_table, P: int | Sequence[int], B: int, nq: int) -> list[torch.Tensor]:
        """generate_batch's results from the call's delayed codes (host): row b keeps its own P_b + max_new_tokens_b + nq columns and is
        finalised at the column its own loop would have ended at (`row_end_offset`, from its first codebook-0 EOS).  `P`: the call's audio
        prefix length, or one per row (ragged_prefix: a row's step index does not depend on its prefix, only its columns do)."""
        return [self._finalise_row(delayed[b:b + 1], P if isinstance(P, int) else int(P[b]), int(row_table[b].max_new_tokens), B, nq)[0] for b in range(B)]

    def _finalise_row(self, delayed_row: torch.Tensor, P_b: int, max_new_tokens: int, B: int, nq: int):
        """One row [1, nq, >= t_b] of a call of B utterances (or of a session of B slots): (its final codes, its first codebook-0 EOS column
        or None, the column its own loop ends at)."""
        offset0 = P_b + 1
        t_b = P_b + max_new_tokens + nq
        row = delayed_row[:, :, :t_b].to(torch.int64)
        hit = (row[0, 0, offset0 + 1:] == self.eos_token_id).nonzero()
        eos_column = offset0 + 1 + int(hit[0, 0]) if len(hit) else None
        end = row_end_offset(offset0, t_b, B, nq, eos_column)
        return finalise_codes(revert_delay_pattern(row), end, nq, self.eos_token_id), eos_column, end

    def _decode_loop(self, eng, ip, delayed, prefix_conditioning, offset, t_total, B, nq, callback, _trace, st, chunk=None, cond_lengths=None,
                     prefix_lens=None, cadence=None):
        """Prefill, first frame and the hot loop (model.py:421-509); a generator that returns the final column offset.  With `chunk`, the
        steps are enqueued at least every `chunk` steps and it yields (delayed, column offset written last) there."""
        if prefix_lens is not None:
            S = self._prefill_ragged(eng, delayed, prefix_conditioning, t_total, B, st, cond_lengths, prefix_lens)
        else:
            S = self._prefill_shared(eng, delayed, prefix_conditioning, offset, B, st, cond_lengths)
        return (yield from self._loop_after_prefill(eng, ip, delayed, S, offset, t_total, B, nq, callback, _trace, st, chunk, cadence))

    def _prefill_ragged(self, eng, delayed, prefix_conditioning, t_total, B, st, cond_lengths, prefix_lens) -> int:
        """generate_batch(ragged_prefix=True): row r = [cond_r[:L_b] ‖ embed(delayed_b[:, :P_b + 1]) ‖ zeros], b = r mod B, built for all rows
        by one kernel (zn_op_assemble_prefill); returns S, the longest row."""
        dev = self.device
        cond = prefix_conditioning.to(device=dev, dtype=torch.bfloat16).contiguous()
        R, L_c, d = cond.shape
        row_lens = [cond_lengths[r % B] + prefix_lens[r % B] + 1 for r in range(R)]
        S = max(row_lens)
        meta = torch.tensor([list(cond_lengths), list(prefix_lens)], dtype=torch.int32).to(dev)      # one host->device copy for both arrays
        hidden = torch.empty(R, S, d, dtype=torch.bfloat16, device=dev)
        row_len_dev = torch.empty(R, dtype=torch.int32, device=dev)
        eng.call("zn_op_assemble_prefill", cond.data_ptr(), L_c, meta[0].data_ptr(), delayed.data_ptr(), t_total, meta[1].data_ptr(), B, R,
                 hidden.data_ptr(), S, row_len_dev.data_ptr(), st)
        eng.call("zn_prefill_rows", hidden.data_ptr(), S, (C.c_int32 * R)(*row_lens), st)
        return S

    def _prefill_shared(self, eng, delayed, prefix_conditioning, offset, B, st, cond_lengths) -> int:
        """The prefill of a call whose utterances share one audio prefix length; returns S, the longest row."""
        dev = self.device
        # prefill (generation_utils.py:236-244): [cond ‖ uncond] conditioning + embed(delayed[..., :P+1]) for both halves; without
        # guidance the B conditional rows and the embedding once (generation_utils.py:237)
        emb = self.embed_codes(delayed[..., :offset], _eng=eng)
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

    def _loop_after_prefill(self, eng, ip, delayed, S, offset, t_total, B, nq, callback, _trace, st, chunk, cadence=None):
        """First frame and the hot loop (model.py:423-509), the prefill of S positions done.  `cadence`: the batch size whose stop-check
        cadence the loop follows (None: B; a mixed call has more utterance rows than requests)."""
        cadence = B if cadence is None else cadence
        eng.call("zn_sample_first", st)
        ip.seqlen_offset += S
        if _trace is not None:
            _trace.setdefault("logits", []).append(self._step_logits(eng, B, nq))
            if _trace.get("after_step") is not None:
                _trace["after_step"](-1, delayed, offset)
        # hot loop with the reference's stop-check cadence (tensor_ops.py:84-105)
        max_steps = t_total - offset
        frame = delayed[..., offset:offset + 1]
        pending, done = 0, ctypes_int()
        cpu_step_counter = 0
        # Without a callback the stop flag of check k is read after the steps up to check k + 1 have been enqueued (the device ->
        # host round trip leaves the critical path); a stop seen late rolls `offset` back to the check that saw it, and the
        # over-run steps have only written columns beyond that cut.
        deferred = callback is None and _trace is None
        begun_at = None                                            # offset at the check whose read-back is in flight
        for step_idx in range(max_steps):
            offset += 1
            cpu_step_counter += 1
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


def ctypes_int():
    return C.c_int32(0)
