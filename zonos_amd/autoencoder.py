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
from .resample import check_rates, stage_step

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


RESAMPLE_MAX_ROWS = 64          # rows of one zn_resample_rows call (= zn_dac_decode_spans')


class Resampler:
    """A `zn_resampler` handle (include/zonos_hip.h "output resampling"; zonos_amd/resample.py is the specification): the filter table of
    orig_freq -> new_freq on the device, `zn_resample_span`'s stream arithmetic and the `zn_resample_rows` launch.  Equal rates give the
    identity, which exists for the PCM16 conversion alone."""

    def __init__(self, orig_freq: int, new_freq: int, device):
        self.orig_freq, self.new_freq = check_rates(orig_freq, new_freq)
        self.device, self.identity = torch.device(device), self.orig_freq == self.new_freq
        self._args = (self.orig_freq, self.new_freq, 6, 0.99)
        lib = _lib.load()
        self.o = self.n = 1
        if not self.identity:
            o, n = C.c_int32(), C.c_int32()
            _lib.check_resample(lib.zn_resample_plan(*self._args, C.byref(o), C.byref(n), None, None, None, 0, None, 0), None, "zn_resample_plan")
            self.o, self.n = o.value, n.value
        self._h = C.c_void_p()
        _lib.check_resample(lib.zn_resampler_create(*self._args, C.byref(self._h)), None, "zn_resampler_create")

    def destroy(self):
        if self._h is not None:
            _lib.load().zn_resampler_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def total(self, T: int) -> int:
        """ceil(n * T / o): the outputs of a signal of T samples."""
        return -((-self.n * int(T)) // self.o)

    def _span(self, avail: int, at_end: bool, j: int) -> tuple[int, int]:
        nf, fi = C.c_int64(), C.c_int64()
        _lib.check_resample(_lib.load().zn_resample_span(*self._args, int(avail), int(bool(at_end)), int(j), C.byref(nf), C.byref(fi)), None, "zn_resample_span")
        return nf.value, fi.value

    def n_final(self, avail: int, at_end: bool) -> int:
        """zn_resample_span: how many leading outputs are final with `avail` input samples known.  Host arithmetic only."""
        return int(avail) if self.identity else self._span(avail, at_end, 0)[0]

    def first_in(self, j: int) -> int:
        """zn_resample_span: the first input that the outputs from j on still read."""
        return int(j) if self.identity else self._span(0, False, j)[1]

    def rows(self, x: torch.Tensor, rows: list, out_max: int, pcm16: bool) -> torch.Tensor:
        """The device call: x fp32 [rows, in_max], rows = [(in0, in_len, out0, out_count, at_end)] -> fp32 or int16 [rows, out_max], row r's
        outputs in its first out_count cells.  The launch goes to the current stream."""
        if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous() or x.shape[0] != len(rows):
            raise ValueError(f"expected contiguous float32 [{len(rows)}, in_max], got {x.dtype} {tuple(x.shape)}")
        out = torch.empty(len(rows), out_max, dtype=torch.int16 if pcm16 else torch.float32, device=x.device)
        arr = (_lib.zn_resample_row * len(rows))(*[_lib.zn_resample_row(i0, n, o0, c, int(bool(e))) for i0, n, o0, c, e in rows])
        with torch.cuda.device(x.device):
            _lib.check_resample(_lib.load().zn_resample_rows(self._h, x.data_ptr(), x.shape[1], arr, len(rows), out.data_ptr(), out_max, int(bool(pcm16)),
                                                             torch.cuda.current_stream(x.device).cuda_stream), self._h, "zn_resample_rows")
        return out

    def whole(self, wav: torch.Tensor, pcm16: bool) -> torch.Tensor:
        """wav [..., T] (whole signals) -> [..., ceil(n T / o)], up to RESAMPLE_MAX_ROWS signals per launch."""
        shape, T = wav.shape, wav.shape[-1]
        x = wav.reshape(-1, T).to(dtype=torch.float32).contiguous()
        total = self.total(T)
        if x.shape[0] == 0 or total == 0:
            return torch.empty(shape[:-1] + (total,), dtype=torch.int16 if pcm16 else torch.float32, device=wav.device)
        parts = [self.rows(x[r:r + RESAMPLE_MAX_ROWS], [(0, T, 0, total, True)] * min(RESAMPLE_MAX_ROWS, x.shape[0] - r), total, pcm16)
                 for r in range(0, x.shape[0], RESAMPLE_MAX_ROWS)]
        return (parts[0] if len(parts) == 1 else torch.cat(parts)).reshape(shape[:-1] + (total,))


class _Tail:
    """The state of one resampled stream: the input tail [in0, in0 + len) as fp32 [B, len] that outputs not yet returned still read, and
    the outputs returned so far."""
    __slots__ = ("tail", "in0", "emitted")

    def __init__(self):
        self.tail, self.in0, self.emitted = None, 0, 0

    def plan(self, rs: Resampler, new: "torch.Tensor | None", at_end: bool):
        """With `new` fp32 [B, m] (or None) appended -> (window, out0, count, keep): `resample.stage_step` over zn_resample_span."""
        win = new if self.tail is None else (self.tail if new is None or new.shape[1] == 0 else torch.cat([self.tail, new], dim=1))
        avail = self.in0 + (0 if win is None else win.shape[1])
        out0, count, keep = stage_step(rs.n_final(avail, at_end), rs.first_in, self.in0, avail, self.emitted)
        return win, out0, count, keep

    def commit(self, win, count: int, keep: int) -> None:
        self.emitted += count
        self.tail = None if win is None else win[:, keep - self.in0:]
        self.in0 = keep


class DACAutoencoder:
    def __init__(self, state_dict: dict | None = None, config: dict | None = None, device=None):
        self.cfg = dict(DAC_44KHZ, **(config or {}))
        self.codebook_size = self.cfg["codebook_size"]
        self.num_codebooks = self.cfg["n_codebooks"]
        self.sampling_rate = self.cfg["sampling_rate"]
        self.hop = int(np.prod(self.cfg["upsampling_ratios"]))
        self._weights: dict | None = None
        self._h = None
        self._resamplers: dict = {}        # output rate -> Resampler
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
        for rs in self._resamplers.values():
            rs.destroy()
        self._resamplers.clear()

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

    def _resampler(self, sample_rate, pcm16: bool) -> "Resampler | None":
        """The output stage of `sample_rate` / `pcm16`: None where there is none (the codec's rate, fp32: today's outputs, untouched)."""
        rate = self.sampling_rate if sample_rate is None else check_rates(self.sampling_rate, sample_rate)[1]
        if rate == self.sampling_rate and not pcm16:
            return None
        if self.device is None or self.device.type != "cuda":
            raise _lib.ZonosHipError("zonos_amd runs on MI355X only (no CPU fallback)")
        with self._lock:
            rs = self._resamplers.get(rate)
            if rs is None:
                rs = self._resamplers[rate] = Resampler(self.sampling_rate, rate, self.device)
        return rs

    def stream(self, stream: "torch.cuda.Stream | None" = None, sample_rate: int | None = None, pcm16: bool = False) -> "DACStream":
        """Incremental decode: `push(codes [B, 9, k]) -> wav [B, 1, m]` returns the samples the frames pushed so far determine, `flush()`
        the rest.  The concatenated outputs equal `decode(all codes)` bit for bit (below ~126 s, where decode() runs the three-term
        kernels).  `stream`: the torch stream every launch goes to (default: the current stream of each call).  `sample_rate` / `pcm16`:
        the outputs are those of `decode(all codes, sample_rate, pcm16)`, likewise bit for bit (the stage holds back the few input samples
        that outputs not yet final still read)."""
        return DACStream(self, stream, self._resampler(sample_rate, pcm16), pcm16)

    def stream_set(self, stream: "torch.cuda.Stream | None" = None, sample_rate: int | None = None, pcm16: bool = False) -> "DACStreamSet":
        """Any number of independent incremental decodes, by key, served together: `push({key: codes [1, 9, k]}, end=keys)` decodes the
        windows of all keys that have something to emit in one ragged pass (zn_dac_decode_spans).  Per key, the concatenated outputs
        equal `decode(all codes of the key)` bit for bit, as with `stream()`.  `sample_rate` / `pcm16` as there: all keys' rows go through
        one zn_resample_rows call after the span decode."""
        return DACStreamSet(self, stream, self._resampler(sample_rate, pcm16), pcm16)

    @torch.inference_mode()
    def resample(self, wav: torch.Tensor, sample_rate: int | None, pcm16: bool = False) -> torch.Tensor:
        """The output stage of `decode(codes, sample_rate, pcm16)` on a waveform at the codec's rate: wav [..., T] -> float32 or int16
        [..., ceil(n T / o)] (zn_resample_rows; every signal whole).  No stage (codec rate, fp32) returns `wav`."""
        rs = self._resampler(sample_rate, pcm16)
        if rs is None:
            return wav
        with torch.cuda.device(self.device):
            return rs.whole(wav.to(self.device), pcm16)

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
    def decode(self, codes: torch.Tensor, sample_rate: int | None = None, pcm16: bool = False) -> torch.Tensor:
        """autoencoder.py:119-140: codes [B, 9, T] (ints in [0, 1023]) -> float32 [B, 1, 512*T].  `sample_rate`: resampled on the device
        to that rate (zonos_amd/resample.py), [B, 1, ceil(n 512 T / o)]; `pcm16`: int16, decode_to_int16's arithmetic."""
        rs = self._resampler(sample_rate, pcm16)
        h = self._handle()
        B, nq, T = codes.shape
        if nq != self.num_codebooks:
            raise ValueError(f"expected {self.num_codebooks} codebooks, got {nq}")
        c32 = codes.to(device=self.device, dtype=torch.int32).contiguous()
        wav = torch.empty(B, 1, self.hop * T, dtype=torch.float32, device=self.device)
        with self._lock, torch.cuda.device(self.device):
            _lib.check_dac(_lib.load().zn_dac_decode(h, c32.data_ptr(), B, T, wav.data_ptr(), _lib.stream_ptr()), h, "zn_dac_decode")
            if rs is not None:
                wav = rs.whole(wav, pcm16)
        return wav

    @torch.inference_mode()
    def decode_batch(self, codes: list, sample_rate: int | None = None, pcm16: bool = False) -> list:
        """Results of different lengths (what `generate_batch()` and `serve()` return): codes [1, 9, T_i] each -> a list of
        `decode(codes_i, sample_rate, pcm16)`, bit for bit.  Up to 64 items share one zn_dac_decode_spans pass (each row a whole sequence)
        and one zn_resample_rows call; a group with an item beyond the span decode's length limit is decoded item by item."""
        nq = self.num_codebooks
        for i, c in enumerate(codes):
            if c.dim() != 3 or c.shape[0] != 1 or c.shape[1] != nq or c.shape[2] < 1:
                raise ValueError(f"item {i}: expected codes [1, {nq}, T >= 1], got {tuple(c.shape)}")
        rs = self._resampler(sample_rate, pcm16)
        h, out = self._handle(), []
        for g0 in range(0, len(codes), RESAMPLE_MAX_ROWS):
            group = codes[g0:g0 + RESAMPLE_MAX_ROWS]
            Ts = [int(c.shape[2]) for c in group]
            n_max, t_max = max(Ts), self.hop * max(Ts)
            with self._lock, torch.cuda.device(self.device):
                c32 = torch.zeros(len(group), nq, n_max, dtype=torch.int32, device=self.device)     # (cells beyond T_i are never read)
                for r, c in enumerate(group):
                    c32[r, :, :Ts[r]] = c[0].to(device=self.device, dtype=torch.int32)
                wav = torch.empty(len(group), t_max, dtype=torch.float32, device=self.device)
                arr = (_lib.zn_dac_span_row * len(group))(*[_lib.zn_dac_span_row(0, T, 1) for T in Ts])
                rc = _lib.load().zn_dac_decode_spans(h, c32.data_ptr(), n_max, arr, len(group), wav.data_ptr(), t_max, _lib.stream_ptr())
                if rc != -4:                           # ZN_ERR_UNSUPPORTED: a window too long for the span kernels (below)
                    _lib.check_dac(rc, h, "zn_dac_decode_spans")
                    if rs is not None:
                        res = rs.rows(wav, [(0, self.hop * T, 0, rs.total(self.hop * T), True) for T in Ts], rs.total(t_max), pcm16)
                        out += [res[r:r + 1, None, :rs.total(self.hop * T)] for r, T in enumerate(Ts)]
                    else:
                        out += [wav[r:r + 1, None, :self.hop * T] for r, T in enumerate(Ts)]
            if rc == -4:
                out += [self.decode(c, sample_rate, pcm16) for c in group]
        return out

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

    def __init__(self, ae: DACAutoencoder, stream=None, resampler: "Resampler | None" = None, pcm16: bool = False):
        self.ae, self._stream = ae, stream
        self._rs, self._pcm16, self._tail = resampler, pcm16, _Tail()      # the output stage (None: the decoder's samples as they are)
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
        """codes [B, 9, k] (the next k frames) -> float32 [B, 1, m]: the samples that became final (m may be 0).  With an output stage:
        the stage's outputs that became final, float32 or int16."""
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
            return self._stage(self._emit(False), False)

    @torch.inference_mode()
    def flush(self) -> torch.Tensor:
        """The samples that the end of the sequence completes: float32 [B, 1, m']."""
        if self._closed:
            raise RuntimeError("DACStream.flush() called twice")
        self._closed = True
        if self._win is None:
            return torch.empty(0, 1, 0, dtype=torch.int16 if self._pcm16 else torch.float32, device=self.ae.device)
        with self._ctx():
            out = self._stage(self._emit(True), True)
        self._win = None
        return out

    def _stage(self, wav: torch.Tensor, at_end: bool) -> torch.Tensor:
        """The output stage on the samples that became final: one zn_resample_rows call of B equal rows over [tail ‖ wav]."""
        rs, st = self._rs, self._tail
        if rs is None:
            return wav
        win, out0, count, keep = st.plan(rs, wav[:, 0], at_end)
        if count:
            win = win.contiguous()
            out = rs.rows(win, [(st.in0, win.shape[1], out0, count, at_end)] * win.shape[0], count, self._pcm16)[:, None]
        else:
            out = torch.empty(wav.shape[0], 1, 0, dtype=torch.int16 if self._pcm16 else torch.float32, device=self.ae.device)
        st.commit(win, count, keep)
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
    __slots__ = ("win", "c0", "emitted", "tail")

    def __init__(self):
        self.win, self.c0, self.emitted = None, 0, 0
        self.tail = _Tail()                       # the output stage's state (unused without one)


class DACStreamSet:
    """Independent rolling windows by key (the slots of a `Zonos.serve_stream` session), decoded together: a `push` pads the windows of
    all keys that complete a sample into one [rows, 9, n_max] tensor and makes ONE `zn_dac_decode_spans` call, in which every row has its
    own place in its own sequence (frame 0, interior, or its end).  Per key the arithmetic is `DACStream`'s (`window_step`)."""

    def __init__(self, ae: DACAutoencoder, stream=None, resampler: "Resampler | None" = None, pcm16: bool = False):
        self.ae, self._stream = ae, stream
        self._rs, self._pcm16 = resampler, pcm16
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
            if self._rs is not None:
                out = self._stage(out, end)
            for key in end:
                self._keys.pop(key, None)
        return out

    def _stage(self, wavs: dict, end: set) -> dict:
        """The output stage over the samples that became final, all keys in ONE zn_resample_rows call: row r = [tail_r ‖ new samples_r]
        at its own place in its own signal; the keys in `end` emit their tails."""
        rs, dev = self._rs, self.ae.device
        out, plan = {}, []
        for key, wav in wavs.items():
            out[key] = torch.empty(1, 1, 0, dtype=torch.int16 if self._pcm16 else torch.float32, device=dev)
            w = self._keys.get(key)
            if w is None:
                continue
            win, out0, count, keep = w.tail.plan(rs, wav[:, 0], key in end)
            if count:
                plan.append((key, w, win, out0, count, keep))
            else:
                w.tail.commit(win, 0, keep)
        if plan:
            in_max, out_max = max(p[2].shape[1] for p in plan), max(p[4] for p in plan)
            if len(plan) == 1:
                x = plan[0][2].contiguous()
            else:                                     # (the cells beyond a row's in_len are never read)
                x = torch.zeros(len(plan), in_max, dtype=torch.float32, device=dev)
                for r, p in enumerate(plan):
                    x[r, :p[2].shape[1]] = p[2][0]
            res = rs.rows(x, [(w.tail.in0, win.shape[1], out0, count, key in end) for key, w, win, out0, count, _ in plan], out_max, self._pcm16)
            for r, (key, w, win, out0, count, keep) in enumerate(plan):
                out[key] = res[r:r + 1, None, :count]
                w.tail.commit(win, count, keep)
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
