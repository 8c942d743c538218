"""GPU parity of DACAutoencoder.decode (zn_dac_decode through the C ABI) against the golden waveforms recorded
from transformers DacModel.decode (tests/golden/dac.npz) and against the CPU oracle.  Bar (BASELINE.json
north_star): waveform RMS error <= 1e-4 in fp32."""
import numpy as np
import pytest
import torch

from oracle import zonos_oracle as zo
from zonos_amd import synth
from zonos_amd.autoencoder import DACAutoencoder
from zonos_amd.testing import DAC_SMALL, DAC_SMALL_CODEBOOK, build_small_dac, dac_oracle_pair, dac_pointwise

pytestmark = pytest.mark.gpu
RMS_TOL = 1e-4


@pytest.fixture(scope="module")
def dac():
    dw = synth.dac_state_dict(4321)
    return DACAutoencoder(dw, device="cuda:0"), dw


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2)))


def test_dac_decode_vs_transformers_golden(golden_dir, dac):
    ae, _ = dac
    g = np.load(f"{golden_dir}/dac.npz")
    for T in (16, 40):
        codes = torch.from_numpy(synth.randint(4321, f"codes{T}", (1, 9, T), 1024)).to("cuda:0")
        wav = ae.decode(codes)
        assert wav.shape == (1, 1, 512 * T) and wav.dtype == torch.float32
        ref = g[f"wav_{T}"]
        err = _rms(wav[:, 0].cpu().numpy(), ref)
        print(f"\n[dac T={T}] RMS err vs transformers DacModel {err:.3g} (signal RMS {float(np.sqrt(np.mean(ref ** 2))):.3g}), max|d| {np.abs(wav[:, 0].cpu().numpy() - ref).max():.3g}")
        assert err <= RMS_TOL


def test_dac_decode_vs_oracle_batch_and_length(dac):
    """B = 2 ragged-content batch at T = 300 (crosses every tile boundary: 300*512 = 153600 samples) vs the oracle."""
    ae, dw = dac
    codes = torch.from_numpy(synth.randint(7, "codes.b", (2, 9, 300), 1024))
    wav = ae.decode(codes.to("cuda:0")).cpu()
    ref = zo.dac_decode(dw, codes)
    assert wav.shape == ref.shape == (2, 1, 153600)
    err = _rms(wav.numpy(), ref.numpy())
    print(f"\n[dac B=2 T=300] RMS err vs oracle {err:.3g}, max|d| {(wav - ref).abs().max().item():.3g}")
    assert err <= RMS_TOL
    # batch rows are independent: row 1 alone reproduces row 1 of the batch
    solo = ae.decode(codes[1:2].to("cuda:0")).cpu()
    assert torch.equal(solo[0], wav[1])


def test_dac_edge_lengths_and_int16(dac):
    ae, dw = dac
    for T in (1, 2, 5):      # shorter than every halo / tile
        codes = torch.from_numpy(synth.randint(11, f"codes.e{T}", (1, 9, T), 1024))
        wav = ae.decode(codes.to("cuda:0")).cpu()
        ref = zo.dac_decode(dw, codes)
        assert _rms(wav.numpy(), ref.numpy()) <= RMS_TOL, T
    codes = torch.from_numpy(synth.randint(11, "codes.i16", (1, 9, 12), 1024))
    got = ae.decode_to_int16(codes.to("cuda:0")).cpu()
    ref = zo.dac_decode_to_int16(dw, codes)
    assert got.shape == ref.shape == (12 * 512, 1) and got.dtype == torch.int16
    assert (got.int() - ref.int()).abs().max().item() <= 4      # 1e-4 * 32767 ~ 3.3 LSB


def test_dac_linearity_property_full_length(dac):
    """Size-independent property at the BASELINE length (T = 861, 440 832 samples): decode is deterministic and
    a time-shifted code sequence gives the time-shifted waveform away from the edges (convolutions are shift-equivariant)."""
    ae, _ = dac
    codes = torch.from_numpy(synth.randint(5, "codes.full", (1, 9, 861), 1024)).to("cuda:0")
    w1 = ae.decode(codes)
    w2 = ae.decode(codes)
    assert torch.equal(w1, w2)
    assert w1.shape == (1, 1, 440832) and bool(torch.isfinite(w1).all()) and float(w1.abs().max()) <= 1.0
    shifted = ae.decode(codes[..., 100:])                  # drop the first 100 frames
    a, b = w1[0, 0, (100 + 40) * 512:(861 - 40) * 512], shifted[0, 0, 40 * 512:(761 - 40) * 512]
    assert _rms(a.cpu().numpy(), b.cpu().numpy()) <= 1e-5


def test_encode_vs_transformers_golden(golden_dir):
    """DACAutoencoder.encode (HIP encoder convs + residual VQ) vs transformers DacModel.encode goldens.  fp32 MFMA convs
    sum in a different order than oneDNN, so a latent may differ in its last bits and a nearest-code decision at a
    near-tie may flip (and with it that frame's later codebooks: the VQ is residual).  Bars: first codebook >= 99 % equal,
    all codes >= 95 % equal; decoding our codes and the reference's codes gives waveforms within 2e-2 RMS of each other
    relative to the signal RMS wherever a frame's codes agree (reported)."""
    g = np.load(f"{golden_dir}/dac_encode.npz")
    seed = int(g["seed"])
    dac = DACAutoencoder(synth.dac_state_dict(seed), device="cuda:0")
    tot = eq = 0
    for T in (512 * 6, 512 * 23):
        wav = synth.test_waveform(seed, f"encwav{T}", T).to("cuda:0")
        codes = dac.encode(wav).cpu().numpy()
        ref = g[f"codes_{T}"].astype(np.int64)
        assert codes.shape == ref.shape and codes.dtype == np.int64
        first = float((codes[:, 0] == ref[:, 0]).mean())
        allc = float((codes == ref).mean())
        print(f"\n[DAC encode T={T}] first codebook equal {first:.4f}, all codes equal {allc:.4f}")
        assert first >= 0.99 and allc >= 0.95
        tot += codes.size; eq += int((codes == ref).sum())
    print(f"[DAC encode] {eq}/{tot} codes equal to transformers'")


def test_encode_batch_and_roundtrip_properties():
    """Batch rows are independent (each equals its solo encode); encode(preprocess(x)) has ceil(len/512) frames with the
    padding on the left; decode(encode(x)) returns 512 samples per frame."""
    dac = DACAutoencoder(synth.dac_state_dict(4321), device="cuda:0")
    wav = synth.test_waveform(7, "rt", 512 * 9, batch=3).to("cuda:0")
    codes = dac.encode(wav)
    assert codes.shape == (3, 9, 9) and int(codes.min()) >= 0 and int(codes.max()) <= 1023
    for b in range(3):
        assert torch.equal(dac.encode(wav[b:b + 1]), codes[b:b + 1])
    x = synth.test_waveform(7, "odd", 5000)[0]              # [1, 5000]
    pre = dac.preprocess(x, 44100)
    assert pre.shape[-1] == 512 * 10 and bool((pre[..., :120] == 0).all()) and torch.equal(pre[..., 120:], x)
    c = dac.encode(pre.unsqueeze(0).to("cuda:0"))
    assert c.shape == (1, 9, 10)
    assert dac.decode(c).shape == (1, 1, 5120)
    with pytest.raises(ValueError, match="multiple of 512"):
        dac.encode(x.unsqueeze(0))


def test_encode_two_seconds_vs_oracle(dac):
    """2 s of audio (173 frames, every encoder tile boundary crossed) vs the CPU oracle: codes >= 99 % identical (a
    near-tie flip redirects the frame's later codebooks), first codebook >= 99.5 %."""
    ae, dw = dac
    T = 512 * 173
    wav = synth.test_waveform(12, "two_s", T)
    ref = zo.dac_encode(dw, wav).numpy()
    got = ae.encode(wav.to("cuda:0")).cpu().numpy()
    first, allc = float((got[:, 0] == ref[:, 0]).mean()), float((got == ref).mean())
    print(f"\n[DAC encode 2 s] first codebook equal {first:.4f}, all codes equal {allc:.4f}")
    assert first >= 0.995 and allc >= 0.99


def test_clip_beyond_the_32_bit_offsets_takes_the_fp32_kernels(dac):
    """The three-term kernels address one batch element's activations with 32-bit byte offsets: beyond 126 s of audio (11 000 frames here)
    zn_dac_decode runs the fp32 kernels.  Size-independent check: the head of the long decode equals the decode of the head of the codes
    (a different kernel family: within 1e-5 RMS) away from the cut."""
    ae, _ = dac
    codes = torch.from_numpy(synth.randint(9, "codes.long", (1, 9, 11000), 1024)).to("cuda:0")
    long = ae.decode(codes)
    assert long.shape == (1, 1, 11000 * 512) and bool(torch.isfinite(long).all())
    head = ae.decode(codes[..., :200])
    a, b = long[0, 0, :160 * 512].cpu().numpy(), head[0, 0, :160 * 512].cpu().numpy()
    assert _rms(a, b) <= 1e-5
    tail = ae.decode(codes[..., -200:])
    a, b = long[0, 0, -160 * 512:].cpu().numpy(), tail[0, 0, -160 * 512:].cpu().numpy()
    assert _rms(a, b) <= 1e-5


# ------------------------------------------------------------------------------------------------ pointwise bars, small configurations
# Every case below is held to a single-sample bar against the float64 oracle (zonos_amd.testing.dac_pointwise: max|gpu - oracle64| <=
# 8 x max|oracle32 - oracle64|), on both kernel families: the three-term kernels (default) and the fp32 kernels (ZONOS_DAC_CONV=fp32 when the
# handle is created).  Small configurations (zonos_amd.testing.DAC_SMALL) reach what the 44.1 kHz one never does: Cout below a tile,
# the NT = 2 / 3 / 4 variants and the pad-to-128 branch of the fp32 family, strides 6 and 10, frames of 6 ... 120 rows against 128-row tiles.

FULL_RATIOS = (8, 8, 4, 2)
FAMILIES = ("three_term", "fp32")
SMALL_CASES = [(1, 1), (1, 2), (2, 23), (3, 70)]
POINTWISE_CASES = [(n, b, t) for n in DAC_SMALL for (b, t) in SMALL_CASES] + [("FULL", 1, 24), ("FULL", 2, 40)]


class _Handles:
    """One DACAutoencoder per (configuration, kernel family) and one oracle pair per case, made on first use and shared by the tests below."""

    def __init__(self):
        self.ae, self.refs = {}, {}

    def get(self, name, family):
        if (name, family) not in self.ae:
            if name == "FULL":
                dw = synth.dac_state_dict(4321, encoder=False)
                ae, ratios, size = DACAutoencoder(dw, device="cuda:0"), FULL_RATIOS, 1024
            else:
                ae, dw, ratios = build_small_dac(name)
                size = DAC_SMALL_CODEBOOK
            with pytest.MonkeyPatch.context() as mp:       # zn_dac_create reads the variable: set only around the handle's creation
                if family == "fp32":
                    mp.setenv("ZONOS_DAC_CONV", "fp32")
                else:
                    mp.delenv("ZONOS_DAC_CONV", raising=False)
                ae._handle()
            self.ae[name, family] = (ae, dw, ratios, size)
        return self.ae[name, family]

    def oracle(self, key, dw, codes, ratios):
        if key not in self.refs:
            self.refs[key] = dac_oracle_pair(dw, codes, ratios)
        return self.refs[key]


@pytest.fixture(scope="module")
def handles():
    return _Handles()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name,B,T", POINTWISE_CASES, ids=[f"{n}-B{b}-T{t}" for n, b, t in POINTWISE_CASES])
def test_dac_pointwise_vs_float64_oracle(handles, name, B, T, family):
    ae, dw, ratios, size = handles.get(name, family)
    codes = torch.from_numpy(synth.randint(31, f"pw.{name}.{B}.{T}", (B, 9, T), size))
    wav = ae.decode(codes.to("cuda:0")).cpu()
    hop = int(np.prod(ratios))
    assert wav.shape == (B, 1, hop * T) and wav.dtype == torch.float32
    assert bool(torch.isfinite(wav).all()) and float(wav.abs().max()) <= 1.0
    res = dac_pointwise(wav, dw, codes, ratios, f"{name} {family} B={B} T={T}", refs=handles.oracle((name, B, T), dw, codes, ratios))
    assert res.ok, res.line(f"{name} {family} B={B} T={T}", hop)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name,B,T", [("S2", 3, 70), ("FULL", 4, 40)])
def test_dac_batch_rows_equal_solo_decodes(handles, name, B, T, family):
    """Every row of a batch, decoded alone, is that row of the batch bit for bit.  At FULL the solo decode takes the 128-row tile kernel at
    the last block and the batch the 256-row one (zn_conv3_launch: `big`); an output's accumulation order does not depend on the tile height."""
    ae, _, ratios, size = handles.get(name, family)
    codes = torch.from_numpy(synth.randint(37, f"rows.{name}", (B, 9, T), size)).to("cuda:0")
    batch = ae.decode(codes)
    assert batch.shape == (B, 1, int(np.prod(ratios)) * T)
    for b in range(B):
        solo = ae.decode(codes[b:b + 1])
        assert torch.equal(solo[0], batch[b]), (name, family, b, (solo[0] - batch[b]).abs().max().item())


def _constant_codes(name, B, T, size):
    col = torch.from_numpy(synth.randint(41, f"period.{name}", (B, 9, 1), size))          # a different column per batch row
    assert all(not torch.equal(col[0], col[b]) for b in range(1, B))
    return col.expand(B, 9, T).contiguous()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", ["S1", "S2", "FULL"])
def test_dac_constant_codes_give_bit_periodic_frames(handles, name, family):
    """The same code column in every frame: away from the clip's ends every layer's activations are periodic in time with the layer's
    cumulative stride, and an output element's arithmetic order does not depend on where it sits in a tile (K chunk, then tap, then the six
    products in dac_conv3_kernel; tap, then channel in dac_final_kernel), so the interior frames of the waveform are bit-identical: a row
    staged or read wrongly at a tile seam breaks that, with no tolerance involved.  The interior comes from the reference alone: the frames
    whose float64-oracle output equals the middle frame's within 1e-12 (S1, S2: at least 40 of the 96 frames, required here; FULL: the fixed
    [12, 36) of 48 frames, B = 4, so that blocks 2 and 3 run the 256-row kernels)."""
    ae, dw, ratios, size = handles.get(name, family)
    hop = int(np.prod(ratios))
    if name == "FULL":
        B, T, lo, hi = 4, 48, 12, 36
        codes = _constant_codes(name, B, T, size)
    else:
        B, T = 2, 96
        codes = _constant_codes(name, B, T, size)
        _, ref64 = handles.oracle((name, "period"), dw, codes, ratios)
        f = ref64.view(B, T, hop)
        same = ((f - f[:, T // 2:T // 2 + 1]).abs().amax(dim=(0, 2)) <= 1e-12).tolist()
        lo = hi = T // 2
        while lo > 0 and same[lo - 1]:
            lo -= 1
        while hi < T and same[hi]:
            hi += 1
        print(f"\n[dac periodic {name}] oracle interior frames [{lo}, {hi})")
        assert hi - lo >= 40, (name, lo, hi)
    wav = ae.decode(codes.to("cuda:0")).cpu()
    assert wav.shape == (B, 1, hop * T)
    frames = wav.view(B, T, hop)
    want = frames[:, lo:lo + 1].expand(B, hi - lo, hop)
    if not torch.equal(frames[:, lo:hi], want):
        bad = (frames[:, lo:hi] != want).nonzero()
        b, fr, s = (int(v) for v in bad[0])
        pos = (lo + fr) * hop + s
        raise AssertionError(f"{name} {family}: {len(bad)} samples of the interior differ from frame {lo}; first at row {b} sample {pos} "
                             f"(mod 128 = {pos % 128}, mod 256 = {pos % 256}), |d| {float((frames[b, lo + fr, s] - frames[b, lo, s]).abs()):.3g}")
    assert float(frames[:, lo].abs().max()) > 1e-3         # not a silent waveform
