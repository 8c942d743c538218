"""Output resampling: the specification (CPU only: numpy, and torch for the filter formula).  The device side is
zonos_amd/csrc/zn_resample_kernels.h behind `zn_resample_rows`; tests/test_resample_cpu.py and tests/test_gpu_resample.py hold the library to
this module.

`ResamplePlan(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99)`: with g = gcd, o = orig_freq / g, n = new_freq / g,
base = min(o, n) * rolloff and width = ceil(lowpass_filter_width * o / base), the table k fp32 [n, 2 * width + o] is the polyphase
windowed-sinc filter of `autoencoder.sinc_resample` (torchaudio's sinc_interp_hann), evaluated in float64 and rounded to fp32 once.
Phase p's support [lo_p, hi_p) is the smallest interval that holds every tap whose fp32 value is nonzero (the taps outside are the
clamped ends of the window: cos(pi / 2)^2 * sinc underflows to zero in fp32).

Output j = q * n + p of a signal x of T samples, 0 <= j < ceil(n * T / o), is ONE fp32 chain

    acc = 0;  for i = lo_p .. hi_p - 1 ascending:  acc = fma(k[p][i], x[q * o - width + i], acc)          (x = 0 outside [0, T))

and this chain is the definition: the value depends on j and the signal alone, so the whole-signal form, a span of a stream and a row of
a ragged batch compute the same bits (`resample_chain` is all three).  Against the exact sum the chain is off by at most gamma_m * A[j],
gamma_m = m u / (1 - m u), u = 2^-24, m = hi_p - lo_p, A[j] = sum |k| |x| (`resample_reference` returns both in float64).

Finality (`n_final`): y[j] is final once q * o - width + hi_p <= avail input samples exist, or when the signal has ended; the first input
it reads is max(0, q * o - width + lo_p) (`first_in`).  `ResampleStream` is the stream stage built on the two: it keeps only the input
tail that outputs not yet final still read, and the concatenation of what it returns equals the whole-signal result bit for bit.

`pcm16(y)`: clamp(y * 32767, +-32767) truncated toward zero - the arithmetic of `DACAutoencoder.decode_to_int16`.
"""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24


def gamma(m) -> "np.ndarray | float":
    """The bound factor of an m-term fp32 FMA chain."""
    m = np.asarray(m, dtype=np.float64)
    return m * U / (1.0 - m * U)


def check_rates(orig_freq, new_freq) -> tuple[int, int]:
    o, n = int(orig_freq), int(new_freq)
    if o < 1 or n < 1 or o != orig_freq or n != new_freq:
        raise ValueError(f"sample rates must be integers >= 1, got {orig_freq!r} -> {new_freq!r}")
    return o, n


def _fma32(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """fp32 fma(a, b, c), exactly: the product of two fp32 values is exact in float64; the sum is rounded to odd in float64 (TwoSum gives
    the rounding error), and a value rounded to odd at 53 bits rounds to fp32 as the exact value would."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    if fix.any():
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(np.float32)


class ResamplePlan:
    def __init__(self, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
        import torch
        orig_freq, new_freq = check_rates(orig_freq, new_freq)
        if int(lowpass_filter_width) < 1 or not 0.0 < float(rolloff) <= 1.0:
            raise ValueError(f"lowpass_filter_width {lowpass_filter_width} must be >= 1 and rolloff {rolloff} lie in (0, 1]")
        self.orig_freq, self.new_freq, self.lowpass_filter_width, self.rolloff = orig_freq, new_freq, int(lowpass_filter_width), float(rolloff)
        g = math.gcd(orig_freq, new_freq)
        self.o, self.n = o, n = orig_freq // g, new_freq // g
        self.base = base = min(o, n) * self.rolloff
        self.width = width = math.ceil(self.lowpass_filter_width * o / base)
        self.taps = 2 * width + o
        # autoencoder.py:39-45, operation for operation
        lfw = self.lowpass_filter_width
        idx = torch.arange(-width, width + o, dtype=torch.float64)[None, None] / o
        t = torch.arange(0, -n, -1, dtype=torch.float64)[:, None, None] / n + idx
        t = (t * base).clamp_(-lfw, lfw)
        window = torch.cos(t * math.pi / lfw / 2) ** 2
        t = t * math.pi
        kernels = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window * (base / o)
        self.table = kernels.to(torch.float32).numpy().reshape(n, self.taps).copy()            # fp32 [n, 2 * width + o]
        nz = self.table != 0
        self.lo = np.where(nz.any(1), nz.argmax(1), 0).astype(np.int64)
        self.hi = np.where(nz.any(1), self.taps - nz[:, ::-1].argmax(1), 0).astype(np.int64)
        self.m = self.hi - self.lo                                                           # support lengths

    def total(self, T: int) -> int:
        """ceil(n * T / o): the outputs of a signal of T samples."""
        return -((-self.n * int(T)) // self.o)

    def need(self, j: int) -> int:
        """Output j is final once this many input samples exist."""
        q, p = divmod(int(j), self.n)
        return q * self.o - self.width + int(self.hi[p])

    def reads_from(self, j: int) -> int:
        q, p = divmod(int(j), self.n)
        return q * self.o - self.width + int(self.lo[p])

    def n_final(self, avail: int, at_end: bool) -> int:
        """How many leading outputs are final with input samples [0, avail) known (at_end: they are the whole signal)."""
        if at_end:
            return self.total(avail)
        q = max(0, (avail + self.width - int(self.hi.max())) // self.o + 1)      # the frames before q are final in every phase
        j = q * self.n
        while self.need(j) <= avail:
            j += 1
        return j

    def first_in(self, j: int) -> int:
        """The first input that the outputs from j on still read."""
        return max(0, min(self.reads_from(jj) for jj in range(int(j), int(j) + self.n)))


def resample_chain(x, plan: ResamplePlan, in0: int = 0, out0: int = 0, count: int | None = None, at_end: bool = True) -> np.ndarray:
    """The definition, on a window: x fp32 [..., L] holds input samples [in0, in0 + L) of its signals (at_end: in0 + L is their end) ->
    fp32 [..., count]: outputs [out0, out0 + count).  Defaults: the whole signal.  ValueError when an output reads an input outside the
    window other than before sample 0 or past the end of an ended signal."""
    x = np.asarray(x, dtype=np.float32)
    L = x.shape[-1]
    if count is None:
        if not at_end:
            raise ValueError("count is required for a window that does not end its signal")
        count = plan.total(in0 + L) - out0
    if count < 0 or in0 < 0 or out0 < 0:
        raise ValueError(f"bad window: in0 = {in0}, out0 = {out0}, count = {count}")
    if at_end and out0 + count > plan.total(in0 + L):
        raise ValueError(f"outputs up to {out0 + count}: a signal of {in0 + L} samples has {plan.total(in0 + L)}")
    y = np.zeros(x.shape[:-1] + (count,), dtype=np.float32)
    o, n, width = plan.o, plan.n, plan.width
    for p in range(n):
        j = np.arange(out0 + (p - out0) % n, out0 + count, n, dtype=np.int64)          # the outputs of phase p
        if not len(j) or not plan.m[p]:
            continue
        first = (j // n) * o - width + plan.lo[p]                                       # absolute index of the support's first input
        last = first + plan.m[p]
        if (np.maximum(first, 0) < in0)[last > 0].any():
            raise ValueError(f"phase {p}: an output reads an input before the window's start {in0}")
        if not at_end and (last > in0 + L).any():
            raise ValueError(f"phase {p}: an output reads an input past the window's end {in0 + L}, which is not the signal's")
        acc = np.zeros(x.shape[:-1] + (len(j),), dtype=np.float32)
        for t in range(int(plan.m[p])):
            i = first + t - in0
            ok = (i >= 0) & (i < L)
            v = np.where(ok, x[..., np.clip(i, 0, max(L - 1, 0))] if L else np.float32(0), np.float32(0)).astype(np.float32)
            acc = _fma32(np.broadcast_to(plan.table[p, plan.lo[p] + t], acc.shape), v, acc)
        y[..., j - out0] = acc
    return y


def resample_reference(x, plan: ResamplePlan) -> tuple[np.ndarray, np.ndarray]:
    """(ref, A) float64 [..., ceil(n T / o)]: the same sum over the fp32 table in float64, and A[j] = sum |k| |x|."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    T = x.shape[-1]
    total = plan.total(T)
    k = plan.table.astype(np.float64)
    frames = -(-total // plan.n) if total else 0
    pad = np.zeros(x.shape[:-1] + (plan.width + frames * plan.o + plan.width + plan.o + T,), dtype=np.float64)
    pad[..., plan.width:plan.width + T] = x
    ref = np.zeros(x.shape[:-1] + (frames * plan.n,), dtype=np.float64)
    A = np.zeros_like(ref)
    for q in range(frames):
        seg = pad[..., q * plan.o:q * plan.o + plan.taps]
        ref[..., q * plan.n:(q + 1) * plan.n] = seg @ k.T
        A[..., q * plan.n:(q + 1) * plan.n] = np.abs(seg) @ np.abs(k).T
    return ref[..., :total], A[..., :total]


def pcm16(y) -> np.ndarray:
    """clamp(y * 32767, +-32767) truncated toward zero -> int16 (decode_to_int16's arithmetic, in fp32)."""
    s = np.asarray(y, dtype=np.float32) * np.float32(32767.0)
    return np.trunc(np.clip(s, np.float32(-32767.0), np.float32(32767.0))).astype(np.int16)


def stage_step(n_final: int, first_in, in0: int, avail: int, emitted: int):
    """The arithmetic of one push of a stream stage, shared by `ResampleStream` and the device stages of autoencoder.py: with `n_final`
    outputs final and `emitted` returned so far -> (out0, count, keep_from): compute outputs [out0, out0 + count) from the window, then
    keep the inputs from `keep_from` (in0 .. avail) on.  `first_in(j)`: the first input the outputs from j on read."""
    count = max(0, n_final - emitted)
    return emitted, count, min(max(in0, first_in(emitted + count)), avail)


class ResampleStream:
    """The stream stage in numpy: `push(x [..., k], at_end=False) -> y [..., m]`, the outputs that became final.  Keeps the input tail
    [in0, in0 + len(tail)) that outputs not yet returned still read."""

    def __init__(self, plan: ResamplePlan, pcm: bool = False):
        self.plan, self.pcm = plan, pcm
        self.tail: np.ndarray | None = None
        self.in0, self.emitted, self.closed = 0, 0, False

    def push(self, x, at_end: bool = False) -> np.ndarray:
        if self.closed:
            raise RuntimeError("ResampleStream.push() after the end")
        x = np.asarray(x, dtype=np.float32)
        win = x if self.tail is None else np.concatenate([self.tail, x], axis=-1)
        avail = self.in0 + win.shape[-1]
        out0, count, keep = stage_step(self.plan.n_final(avail, at_end), self.plan.first_in, self.in0, avail, self.emitted)
        y = resample_chain(win, self.plan, self.in0, out0, count, at_end)
        self.emitted += count
        self.tail, self.in0, self.closed = win[..., keep - self.in0:], keep, bool(at_end)
        return pcm16(y) if self.pcm else y
