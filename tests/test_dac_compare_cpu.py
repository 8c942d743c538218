"""The pointwise DAC comparator (zonos_amd.testing.pointwise_compare) on synthetic arrays: one wrong sample in a 2 x 153 600 waveform
passes the whole-waveform RMS bar of tests/test_gpu_dac.py and fails the comparator; the float64 oracle really runs in float64."""
import numpy as np
import torch

from oracle import zonos_oracle as zo
from zonos_amd import synth
from zonos_amd.testing import DAC_POINTWISE_FACTOR, DAC_SMALL, DAC_SMALL_CODEBOOK, dac_oracle_pair, pointwise_compare

RMS_TOL = 1e-4                 # tests/test_gpu_dac.py
B, N, HOP = 2, 153600, 512     # its B = 2, T = 300 case


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2)))


def _arrays():
    """A float64 "oracle" waveform, its fp32 counterpart (fp32-rounding-sized noise, max 2.5e-6: the figure measured for the 44.1 kHz config)
    and a "GPU" waveform with noise of twice that size."""
    t = np.arange(B * N, dtype=np.float64).reshape(B, 1, N)
    ref64 = 0.6 * np.sin(t * 0.031) * np.cos(t * 0.0007)
    n32 = synth.uniform(3, "cmp.n32", (B, 1, N), 2.5e-6).astype(np.float64)
    ngpu = synth.uniform(3, "cmp.ngpu", (B, 1, N), 5e-6).astype(np.float64)
    return torch.from_numpy(ref64), torch.from_numpy((ref64 + n32).astype(np.float32)), torch.from_numpy((ref64 + ngpu).astype(np.float32))


def test_one_wrong_sample_passes_rms_and_fails_the_comparator(capsys):
    ref64, ref32, gpu = _arrays()
    good = pointwise_compare(gpu, ref32, ref64, HOP, "synthetic")
    assert good.ok and 1.0 < good.ratio <= DAC_POINTWISE_FACTOR and 2e-6 < good.e32 < 3e-6
    bad_wav = gpu.clone()
    where = (1, 77 * HOP + 131)                            # one sample of one row
    bad_wav[where[0], 0, where[1]] += 1e-3
    assert _rms(bad_wav.numpy(), ref32.numpy()) <= RMS_TOL       # the old bar does not see it ...
    bad = pointwise_compare(bad_wav, ref32, ref64, HOP, "synthetic, one sample + 1e-3")
    assert not bad.ok and bad.index == where                     # ... the comparator does, and says where
    assert bad.err > 9e-4 and bad.ratio > 100 and bad.e32 == good.e32
    out = capsys.readouterr().out
    assert out.count("[dac pointwise") == 2 and f"mod 128 = {where[1] % 128}" in out and f"mod hop {HOP} = {where[1] % HOP}" in out


def test_comparator_rejects_non_finite_and_shape_mismatch():
    ref64, ref32, gpu = _arrays()
    nan = gpu.clone()
    nan[0, 0, 5] = float("nan")
    res = pointwise_compare(nan, ref32, ref64, HOP, "synthetic, NaN")
    assert not res.ok and res.index == (0, 5)
    try:
        pointwise_compare(gpu[..., :-1], ref32, ref64, HOP)
    except ValueError:
        pass
    else:
        raise AssertionError("a shorter waveform must not compare")


def test_float64_oracle_runs_in_float64():
    """dac_oracle_pair: the same oracle code with float64 weights returns float64, and the fp32 run differs from it by fp32-rounding-sized
    amounts, not by more (a silent down-cast inside the oracle would make the two equal; a broken cast would make them far apart).  Also
    the configuration limits of the kernels for the small configurations (Cin % 16 at every layer; final conv C % 4, C <= 120)."""
    for name, c in DAC_SMALL.items():
        ch = [c["hidden"], c["dec_hidden"]] + [c["dec_hidden"] >> (i + 1) for i in range(len(c["ratios"]))]
        assert all(x % 16 == 0 for x in ch) and ch[-1] % 4 == 0 and ch[-1] <= 120, (name, ch)
        assert c["dec_hidden"] % (1 << len(c["ratios"])) == 0 and all(r >= 2 and r % 2 == 0 for r in c["ratios"])
        dw = synth.dac_state_dict(4321, encoder=False, codebook_size=DAC_SMALL_CODEBOOK, **c)
        codes = torch.from_numpy(synth.randint(1, f"cmp.codes.{name}", (2, 9, 5), DAC_SMALL_CODEBOOK))
        ref32, ref64 = dac_oracle_pair(dw, codes, c["ratios"])
        hop = int(np.prod(c["ratios"]))
        assert ref32.shape == ref64.shape == (2, 1, 5 * hop) and ref64.dtype == torch.float64
        e32 = float((ref32.double() - ref64).abs().max())
        assert 0 < e32 < 2e-5, (name, e32)
        assert torch.equal(ref32, zo.dac_decode(dw, codes, ratios=c["ratios"]))
