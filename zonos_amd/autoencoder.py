"""`DACAutoencoder` — zonos/autoencoder.py:50-170 surface over the HIP DAC codec.

`decode(codes) -> float32 [B, 1, 512*T]`, `decode_to_int16` and `encode(wav) -> int64 [B, 9, T/512]` run in
libzonos_hip.so (fp32 arithmetic: the reference's CPU path disables autocast, autoencoder.py:139).  Weights use the
transformers `DacModel` state-dict names (the reference loads `descript/dac_44khz`, autoencoder.py:74 — a network
fetch, so here they come from a local safetensors file or a state dict).  `preprocess` pads on the left to a multiple
of 512 like the reference; its resampler restates torchaudio's `sinc_interp_hann` (torchaudio is not installed here:
that step is unpinned, identity at 44.1 kHz input).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math

import numpy as np
import threading

import torch

from . import _lib

# transformers DacConfig defaults = descript/dac_44khz (configuration_dac.py:55-70)
DAC_44KHZ = dict(n_codebooks=9, codebook_size=1024, codebook_dim=8, hidden_size=1024, decoder_hidden_size=1536,
                 encoder_hidden_size=64, upsampling_ratios=(8, 8, 4, 2), sampling_rate=44100)


def sinc_resample(wav: torch.Tensor, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> torch.Tensor:
    """torchaudio.functional.resample(..., resampling_method="sinc_interp_hann") as published (the call the reference
    makes at zonos/autoencoder.py:98 with the defaults): windowed-sinc polyphase filter applied as a strided conv1d.
    torchaudio is not installed in this environment, so this restatement is unpinned; equal rates return the input."""
    orig_freq, new_freq = int(orig_freq), int(new_freq)
    if orig_freq == new_freq:
        return wav
    g = math.gcd(orig_freq, new_freq)
    o, n = orig_freq // g, new_freq // g
    base = min(o, n) * rolloff
    width = math.ceil(lowpass_filter_width * o / base)
    idx = torch.arange(-width, width + o, dtype=torch.float64, device=wav.device)[None, None] / o
    t = torch.arange(0, -n, -1, dtype=torch.float64, device=wav.device)[:, None, None] / n + idx
    t = (t * base).clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kernels = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window * (base / o)
    kernels = kernels.to(torch.float32)
    shape = wav.shape
    x = wav.reshape(-1, shape[-1]).to(torch.float32)
    length = x.shape[-1]
    x = torch.nn.functional.pad(x, (width, width + o))
    y = torch.nn.functional.conv1d(x[:, None], kernels, stride=o).transpose(1, 2).reshape(x.shape[0], -1)
    y = y[..., : math.ceil(n * length / o)]
    return y.reshape(shape[:-1] + y.shape[-1:])


class DACAutoencoder:
    def __init__(self, state_dict: dict | None = None, config: dict | None = None, device=None):
        self.cfg = dict(DAC_44KHZ, **(config or {}))
        self.codebook_size = self.cfg["codebook_size"]
        self.num_codebooks = self.cfg["n_codebooks"]
        self.sampling_rate = self.cfg["sampling_rate"]
        self.hop = int(np.prod(self.cfg["upsampling_ratios"]))
        self._weights: dict | None = None
        self._h = None
        self._lock = threading.Lock()      # one handle = one workspace: concurrent encode/decode calls queue
        self.device = torch.device(device) if device is not None else None
        if state_dict is not None:
            self.load_state_dict(state_dict, device)

    @classmethod
    def from_local(cls, path: str, device="cuda") -> "DACAutoencoder":
        """Load a transformers DacModel checkpoint (model.safetensors) from disk."""
        from safetensors.torch import load_file
        return cls(load_file(path), device=device)

    def load_state_dict(self, sd: dict, device=None):
        dev = torch.device(device if device is not None else (self.device or "cuda"))
        keep = {k: v.detach().to(device=dev, dtype=torch.float32).contiguous() for k, v in sd.items()
                if k.startswith(("quantizer.quantizers.", "decoder.", "encoder."))}
        self._weights, self.device = keep, dev
        self._destroy()

    def to(self, device):
        if self._weights is not None:
            self.load_state_dict(self._weights, device)
        else:
            self.device = torch.device(device)
        return self

    def _destroy(self):
        if self._h is not None:
            _lib.load().zn_dac_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    def _handle(self):
        if self._h is not None:
            return self._h
        if self._weights is None:
            raise _lib.ZonosHipError("DACAutoencoder has no weights: the reference fetches descript/dac_44khz "
                                     "(zonos/autoencoder.py:74); offline, use DACAutoencoder.from_local(path) or pass a state dict")
        if self.device.type != "cuda":
            raise _lib.ZonosHipError("zonos_amd runs on MI355X only (no CPU fallback)")
        lib = _lib.load()
        zc = self._config(encoder="encoder.conv1.weight" in self._weights)
        names = sorted(self._weights)
        arr = (_lib.zn_dac_tensor * len(names))()
        for i, k in enumerate(names):
            arr[i].name, arr[i].data_dev, arr[i].numel = k.encode(), self._weights[k].data_ptr(), self._weights[k].numel()
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check_dac(lib.zn_dac_create(C.byref(zc), arr, len(names), C.byref(h)), None, "zn_dac_create")
        self._h = h
        return h

    def _config(self, encoder: bool = False) -> _lib.zn_dac_config:
        c = self.cfg
        zc = _lib.zn_dac_config(n_codebooks=c["n_codebooks"], codebook_size=c["codebook_size"], codebook_dim=c["codebook_dim"],
                                hidden_size=c["hidden_size"], decoder_hidden_size=c["decoder_hidden_size"], n_ratios=len(c["upsampling_ratios"]),
                                encoder_hidden_size=c["encoder_hidden_size"] if encoder else 0)
        for i, r in enumerate(c["upsampling_ratios"]):
            zc.ratios[i] = r
        return zc

    def span(self, c0: int, n: int, at_end: bool) -> tuple[int, int]:
        """zn_dac_span: the samples [s0, s1) that code frames [c0, c0 + n) of a longer sequence determine (`at_end`: c0 + n ends it).
        Host arithmetic only."""
        s0, s1 = C.c_int64(), C.c_int64()
        zc = self._config()
        _lib.check_dac(_lib.load().zn_dac_span(C.byref(zc), int(c0), int(n), int(bool(at_end)), C.byref(s0), C.byref(s1)), None, "zn_dac_span")
        return s0.value, s1.value

    def stream(self, stream: "torch.cuda.Stream | None" = None) -> "DACStream":
        """Incremental decode: `push(codes [B, 9, k]) -> wav [B, 1, m]` returns the samples the frames pushed so far determine, `flush()`
        the rest.  The concatenated outputs equal `decode(all codes)` bit for bit (below ~126 s, where decode() runs the three-term
        kernels).  `stream`: the torch stream every launch goes to (default: the current stream of each call)."""
        return DACStream(self, stream)

    def stream_set(self, stream: "torch.cuda.Stream | None" = None) -> "DACStreamSet":
        """Any number of independent incremental decodes, by key, served together: `push({key: codes [1, 9, k]}, end=keys)` decodes the
        windows of all keys that have something to emit in one ragged pass (zn_dac_decode_spans).  Per key, the concatenated outputs
        equal `decode(all codes of the key)` bit for bit, as with `stream()`."""
        return DACStreamSet(self, stream)

    def preprocess(self, wav: torch.Tensor, sr: int) -> torch.Tensor:
        """autoencoder.py:80-101: resample to 44.1 kHz, zero-pad on the LEFT to a multiple of 512 samples."""
        wav = sinc_resample(wav, sr, self.sampling_rate)
        left_pad = math.ceil(wav.shape[-1] / self.hop) * self.hop - wav.shape[-1]
        return torch.nn.functional.pad(wav, (left_pad, 0), value=0)

    @torch.inference_mode()
    def encode(self, wav: torch.Tensor) -> torch.Tensor:
        """autoencoder.py:103-117: preprocessed audio [B, 1, T] (or [B, T]) -> int64 codes [B, 9, T / 512]."""
        h = self._handle()
        if "encoder.conv1.weight" not in self._weights:
            raise _lib.ZonosHipError("this DACAutoencoder was built from decoder-only weights: encode() needs encoder.* and in_proj tensors")
        if wav.dim() == 3:
            if wav.shape[1] != 1:
                raise ValueError(f"expected mono audio [B, 1, T], got {tuple(wav.shape)}")
            wav = wav[:, 0]
        B, T = wav.shape
        if T < self.hop or T % self.hop:
            raise ValueError(f"audio length {T} is not a positive multiple of {self.hop}: call preprocess() first (autoencoder.py:99-100)")
        x = wav.to(device=self.device, dtype=torch.float32).contiguous()
        codes = torch.empty(B, self.num_codebooks, T // self.hop, dtype=torch.int32, device=self.device)
        with self._lock, torch.cuda.device(self.device):
            _lib.check_dac(_lib.load().zn_dac_encode(h, x.data_ptr(), B, T, codes.data_ptr(), _lib.stream_ptr()), h, "zn_dac_encode")
        return codes.to(torch.int64)

    @torch.inference_mode()
    def decode(self, codes: torch.Tensor) -> torch.Tensor:
        """autoencoder.py:119-140: codes [B, 9, T] (ints in [0, 1023]) -> float32 [B, 1, 512*T]."""
        h = self._handle()
        B, nq, T = codes.shape
        if nq != self.num_codebooks:
            raise ValueError(f"expected {self.num_codebooks} codebooks, got {nq}")
        c32 = codes.to(device=self.device, dtype=torch.int32).contiguous()
        wav = torch.empty(B, 1, self.hop * T, dtype=torch.float32, device=self.device)
        with self._lock, torch.cuda.device(self.device):
            _lib.check_dac(_lib.load().zn_dac_decode(h, c32.data_ptr(), B, T, wav.data_ptr(), _lib.stream_ptr()), h, "zn_dac_decode")
        return wav

    @torch.inference_mode()
    def decode_to_int16(self, codes: torch.Tensor) -> torch.Tensor:
        """autoencoder.py:142-170: clamp(wav * 32767, +-32767) -> int16 [512*T, 1] (batch 1)."""
        wav = self.decode(codes).squeeze(1)
        return torch.clamp(wav * 32767.0, -32767.0, 32767.0).to(torch.int16).squeeze(0).unsqueeze(1)


def span_lead(ae: DACAutoencoder) -> int:
    """Frames [c, ...) determine the samples from c * hop + lead on (c >= 1; the receptive field is shift-invariant by one hop per frame)."""
    return ae.span(1, 1 << 12, True)[0] - ae.hop


def window_step(span, hop: int, lead: int, c0: int, n: int, emitted: int, at_end: bool):
    """The arithmetic of one rolling-window decode, shared by `DACStream` and `DACStreamSet`.  The window holds frames [c0, c0 + n) and
    `emitted` samples have been returned; `span` is `DACAutoencoder.span`.  None when the window completes no new sample; otherwise
    (s0, s1, skip, keep_from): decode samples [s0, s1) of the window, return them from index `skip` on, and afterwards keep the frames
    from `keep_from` (>= c0) on - the earlier ones are read by no sample from s1 on."""
    if n == 0:
        return None
    s0, s1 = span(c0, n, at_end)
    if s1 <= emitted:
        return None
    if s0 > emitted:
        raise RuntimeError(f"DAC stream: window from frame {c0} starts at sample {s0}, past {emitted}")
    c = (s1 - lead) // hop if s1 >= hop + lead else 0
    return s0, s1, emitted - s0, max(c, c0)


class DACStream:
    """Rolling decode over `zn_dac_decode_span`: keeps on the device only the code frames that samples not yet returned still read
    (the decoder's receptive field, ~10 frames on each side at the 44.1 kHz ratios), and no activations: every call decodes its window
    from the codes, so an abandoned stream holds nothing but that window."""

    def __init__(self, ae: DACAutoencoder, stream=None):
        self.ae, self._stream = ae, stream
        self._win: torch.Tensor | None = None     # int32 [B, 9, n]: frames [c0, c0 + n)
        self._c0 = 0
        self._emitted = 0                         # samples returned so far
        self._closed = False
        self._lead = span_lead(ae)

    def _torch_stream(self):
        return self._stream if self._stream is not None else torch.cuda.current_stream(self.ae.device)

    def _ctx(self):
        """The device and the stream of every launch of a call."""
        st = contextlib.ExitStack()
        st.enter_context(torch.cuda.device(self.ae.device))
        st.enter_context(torch.cuda.stream(self._torch_stream()))
        return st

    @torch.inference_mode()
    def push(self, codes: torch.Tensor) -> torch.Tensor:
        """codes [B, 9, k] (the next k frames) -> float32 [B, 1, m]: the samples that became final (m may be 0)."""
        if self._closed:
            raise RuntimeError("DACStream.push() after flush()")
        B, nq, k = codes.shape
        if nq != self.ae.num_codebooks:
            raise ValueError(f"expected {self.ae.num_codebooks} codebooks, got {nq}")
        if self._win is not None and B != self._win.shape[0]:
            raise ValueError(f"batch size changed from {self._win.shape[0]} to {B}")
        with self._ctx():
            c32 = codes.to(device=self.ae.device, dtype=torch.int32)
            self._win = c32.contiguous() if self._win is None else torch.cat([self._win, c32], dim=2)
            return self._emit(False)

    @torch.inference_mode()
    def flush(self) -> torch.Tensor:
        """The samples that the end of the sequence completes: float32 [B, 1, m']."""
        if self._closed:
            raise RuntimeError("DACStream.flush() called twice")
        self._closed = True
        if self._win is None:
            return torch.empty(0, 1, 0, dtype=torch.float32, device=self.ae.device)
        with self._ctx():
            out = self._emit(True)
        self._win = None
        return out

    def _decode(self, win: torch.Tensor, c0: int, at_end: bool, m: int) -> torch.Tensor:
        """The device call: the m samples of the span of window `win` = frames [c0, c0 + n)."""
        ae = self.ae
        h = ae._handle()
        wav = torch.empty(win.shape[0], 1, m, dtype=torch.float32, device=ae.device)
        with ae._lock:
            _lib.check_dac(_lib.load().zn_dac_decode_span(h, win.data_ptr(), win.shape[0], c0, win.shape[2], int(at_end), wav.data_ptr(),
                                                          torch.cuda.current_stream(ae.device).cuda_stream), h, "zn_dac_decode_span")
        return wav

    def _emit(self, at_end: bool) -> torch.Tensor:
        ae, win = self.ae, self._win
        B, n = win.shape[0], win.shape[2]
        step = window_step(ae.span, ae.hop, self._lead, self._c0, n, self._emitted, at_end)
        if step is None:
            return torch.empty(B, 1, 0, dtype=torch.float32, device=ae.device)
        s0, s1, skip, keep = step
        out = self._decode(win, self._c0, at_end, s1 - s0)[..., skip:]
        self._emitted = s1
        if keep > self._c0:                        # drop the frames that no sample from s1 on reads
            self._win = win[..., keep - self._c0:].contiguous()
            self._c0 = keep
        return out


class _Window:
    """One key of a DACStreamSet: frames [c0, c0 + n) as int32 [1, 9, n], and the samples returned so far."""
    __slots__ = ("win", "c0", "emitted")

    def __init__(self):
        self.win, self.c0, self.emitted = None, 0, 0


class DACStreamSet:
    """Independent rolling windows by key (the slots of a `Zonos.serve_stream` session), decoded together: a `push` pads the windows of
    all keys that complete a sample into one [rows, 9, n_max] tensor and makes ONE `zn_dac_decode_spans` call, in which every row has its
    own place in its own sequence (frame 0, interior, or its end).  Per key the arithmetic is `DACStream`'s (`window_step`)."""

    def __init__(self, ae: DACAutoencoder, stream=None):
        self.ae, self._stream = ae, stream
        self._keys: dict = {}
        self._lead = span_lead(ae)

    _torch_stream = DACStream._torch_stream
    _ctx = DACStream._ctx

    def __len__(self):
        return len(self._keys)

    def __contains__(self, key):
        return key in self._keys

    def _decode_rows(self, codes: torch.Tensor, rows: list[tuple[int, int, bool]], t_max: int) -> torch.Tensor:
        """The device call: codes int32 [rows, 9, n_max], rows = [(c0, n, at_end)] -> float32 [rows, t_max], row r's span in front."""
        ae = self.ae
        h = ae._handle()
        wav = torch.empty(len(rows), t_max, dtype=torch.float32, device=ae.device)
        arr = (_lib.zn_dac_span_row * len(rows))(*[_lib.zn_dac_span_row(c0, n, int(e)) for c0, n, e in rows])
        with ae._lock:
            _lib.check_dac(_lib.load().zn_dac_decode_spans(h, codes.data_ptr(), codes.shape[2], arr, len(rows), wav.data_ptr(), t_max,
                                                           torch.cuda.current_stream(ae.device).cuda_stream), h, "zn_dac_decode_spans")
        return wav

    @torch.inference_mode()
    def push(self, chunks: dict, end=()) -> dict:
        """chunks {key: codes [1, 9, k]} (the key's next k frames; a new key starts a stream) -> {key: float32 [1, 1, m]} for every key
        of `chunks` and of `end`: the samples that became final.  Keys in `end` are flushed - their frames so far end their sequence -
        and forgotten.  A key whose window completes no sample takes no row of the call and gets m = 0."""
        ae, nq = self.ae, self.ae.num_codebooks
        end = set(end)
        for key, codes in chunks.items():
            if codes.dim() != 3 or codes.shape[0] != 1 or codes.shape[1] != nq:
                raise ValueError(f"key {key!r}: expected codes [1, {nq}, k], got {tuple(codes.shape)}")
        out, plan = {}, []
        with self._ctx():
            for key in list(chunks) + [k for k in end if k not in chunks]:
                w = self._keys.get(key)
                if key in chunks:
                    if w is None:
                        w = self._keys[key] = _Window()
                    c32 = chunks[key].to(device=ae.device, dtype=torch.int32)
                    w.win = c32.contiguous() if w.win is None else torch.cat([w.win, c32], dim=2)
                out[key] = torch.empty(1, 1, 0, dtype=torch.float32, device=ae.device)
                if w is None or w.win is None:
                    continue
                step = window_step(ae.span, ae.hop, self._lead, w.c0, w.win.shape[2], w.emitted, key in end)
                if step is not None:
                    plan.append((key, w, step))
            if plan:
                n_max = max(w.win.shape[2] for _, w, _ in plan)
                t_max = max(s1 - s0 for _, _, (s0, s1, _, _) in plan)
                if len(plan) == 1:
                    codes = plan[0][1].win
                else:                                 # (the cells beyond a row's n are never read: any valid code will do)
                    codes = torch.zeros(len(plan), nq, n_max, dtype=torch.int32, device=ae.device)
                    for r, (_, w, _) in enumerate(plan):
                        codes[r, :, :w.win.shape[2]] = w.win[0]
                wav = self._decode_rows(codes, [(w.c0, w.win.shape[2], key in end) for key, w, _ in plan], t_max)
                for r, (key, w, (s0, s1, skip, keep)) in enumerate(plan):
                    out[key] = wav[r:r + 1, None, skip:s1 - s0]
                    w.emitted = s1
                    if keep > w.c0:
                        w.win = w.win[..., keep - w.c0:].contiguous()
                        w.c0 = keep
            for key in end:
                self._keys.pop(key, None)
        return out

    def drop(self, key) -> None:
        """Forget a key without decoding its tail (an abandoned request)."""
        self._keys.pop(key, None)


_GLOBAL_DAC_AUTOENCODER = None


def preload_dac_autoencoder(device=None, warmup: bool = False, state_dict: dict | None = None) -> DACAutoencoder:
    """autoencoder.py:10-47 singleton."""
    global _GLOBAL_DAC_AUTOENCODER
    if _GLOBAL_DAC_AUTOENCODER is None:
        _GLOBAL_DAC_AUTOENCODER = DACAutoencoder(state_dict, device=device)
    return _GLOBAL_DAC_AUTOENCODER
