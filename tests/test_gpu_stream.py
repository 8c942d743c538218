"""Streaming on the GPU: DACAutoencoder.stream() (zn_dac_decode_span) against decode(), and Zonos.stream() against generate() +
autoencoder.decode(), bit for bit."""
import pytest
import torch

from zonos_amd import synth
from zonos_amd.autoencoder import DACAutoencoder
from zonos_amd.testing import DAC_SMALL_CODEBOOK, build_model, build_small_dac

pytestmark = pytest.mark.gpu
GREEDY = {"temperature": 0.0}
DEV = "cuda:0"


@pytest.fixture(scope="module")
def dac():
    return DACAutoencoder(synth.dac_state_dict(4321, encoder=False), device=DEV)


def _chunkings(T):
    irregular, k, i = [], 0, 0
    while k < T:
        step = (1, 7, 2, 23, 5, 64, 3)[i % 7]
        irregular.append(min(step, T - k))
        k += irregular[-1]
        i += 1
    return {"all": [T], "ones": [1] * T, "16": [16] * (T // 16) + ([T % 16] if T % 16 else []), "irregular": irregular}


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("T", [1, 3, 9, 10, 11, 40, 300, 861])
def test_dac_stream_equals_decode(dac, B, T):
    codes = torch.from_numpy(synth.randint(17 + T, f"stream.codes{B}", (B, 9, T), 1024)).to(DEV)
    ref = dac.decode(codes)
    for name, sizes in _chunkings(T).items():
        if name == "ones" and T > 300 and B > 1:
            continue                                       # (861 one-frame pushes once, at B = 1)
        st = dac.stream()
        parts, k = [], 0
        for n in sizes:
            parts.append(st.push(codes[..., k:k + n]))
            k += n
        parts.append(st.flush())
        assert all(p.shape[:2] == (B, 1) for p in parts)
        got = torch.cat(parts, dim=2)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        assert torch.equal(got, ref), (name, T, B, (got - ref).abs().max().item())
        if T >= 40 and name != "all":
            assert sum(p.shape[2] for p in parts[:-1]) > 0, name            # audio before the end


@pytest.fixture(scope="module")
def small_dacs():
    return {name: build_small_dac(name, device=DEV)[0] for name in ("S1", "S2")}


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("T", [1, 3, 30, 96])
@pytest.mark.parametrize("name", ["S1", "S2"])
def test_dac_stream_equals_decode_small_ratios(small_dacs, name, B, T):
    """The span windows' device side (launch_conv3_win, the ioff / Tin arguments of dac_final_kernel) at ratios (6, 2) and (2, 6, 10): frames
    of 12 and 120 samples, strides 6 and 10, output channels below a tile."""
    ae = small_dacs[name]
    codes = torch.from_numpy(synth.randint(23 + T, f"stream.{name}.codes{B}", (B, 9, T), DAC_SMALL_CODEBOOK)).to(DEV)
    ref = ae.decode(codes)
    assert ref.shape == (B, 1, ae.hop * T)
    for cname, sizes in _chunkings(T).items():
        st = ae.stream()
        parts, k = [], 0
        for n in sizes:
            parts.append(st.push(codes[..., k:k + n]))
            k += n
        parts.append(st.flush())
        assert all(p.shape[:2] == (B, 1) for p in parts)
        got = torch.cat(parts, dim=2)
        assert got.shape == ref.shape, (name, cname, got.shape, ref.shape)
        assert torch.equal(got, ref), (name, cname, T, B, (got - ref).abs().max().item())
        if T >= 96 and cname != "all":
            assert sum(p.shape[2] for p in parts[:-1]) > 0, cname            # audio before the end


def _cond(cfg, seed, cfg_scale):
    rows = 1 if cfg_scale == 1 else 2
    return synth.conditioning(seed, "cond", rows, 6, cfg["d_model"]).to(DEV)


def _check_stream(model, cond, cfg_scale, max_new, sampling, seed, prefix=None, chunk=16):
    kw = dict(audio_prefix_codes=prefix, max_new_tokens=max_new, cfg_scale=cfg_scale, sampling_params=sampling, seed=seed)
    ref = model.generate(cond, **kw)
    ref_wav = model.autoencoder.decode(ref)
    chunks = list(model.stream(cond, chunk_frames=chunk, **kw))
    assert chunks and all(c.codes.shape[2] or c.wav.shape[2] for c in chunks)
    codes = torch.cat([c.codes for c in chunks], dim=2)
    wav = torch.cat([c.wav for c in chunks], dim=2)
    assert codes.dtype == torch.int64 and codes.device == ref.device
    assert torch.equal(codes, ref), (codes.shape, ref.shape)
    assert wav.shape == ref_wav.shape and torch.equal(wav, ref_wav)
    return chunks, ref


@pytest.fixture(scope="module")
def tiny(dac):
    model, _ = build_model(synth.TINY_CFG, 77, DEV, dac=dac)
    return model


@pytest.mark.parametrize("cfg_scale", [2.0, 1.0], ids=["guided", "cfg1"])
@pytest.mark.parametrize("sampling", ["greedy", "sampled"])
@pytest.mark.parametrize("prefix", [False, True], ids=["noprefix", "prefix"])
def test_tiny_stream_equals_generate_at_max_tokens(tiny, cfg_scale, sampling, prefix):
    """Reaching max_new_tokens (EOS suppressed), chunks of 16 and of 5 frames."""
    eng = tiny.engine(1)
    pre = torch.from_numpy(synth.randint(77, "prefix", (1, 9, 5), 1024)).to(DEV) if prefix else None
    sp = GREEDY if sampling == "greedy" else dict(min_p=0.1)
    eng.call("zn_debug_eos_bias", float("-inf"))
    try:
        chunks, ref = _check_stream(tiny, _cond(synth.TINY_CFG, 77, cfg_scale), cfg_scale, 70, sp, 1234, pre)
        assert ref.shape[2] == 70 + (5 if prefix else 0)
        assert len(chunks) >= 3 and chunks[0].codes.shape[2] < ref.shape[2]          # frames come out before the end
        _check_stream(tiny, _cond(synth.TINY_CFG, 77, cfg_scale), cfg_scale, 40, sp, 99, pre, chunk=5)
    finally:
        eng.call("zn_debug_eos_bias", 0.0)


@pytest.mark.parametrize("cfg_scale", [2.0, 1.0], ids=["guided", "cfg1"])
@pytest.mark.parametrize("step", [0, 3, 10, 30, 45])
def test_tiny_stream_forced_eos(tiny, cfg_scale, step):
    """Codebook-0 EOS forced at a decode step: the stop frame and what the boundary search keeps.  Step 0 at 48 new tokens is the short
    clip whose search window misses the EOS frame (generate() returns it)."""
    eng = tiny.engine(1)
    eng.call("zn_debug_force_eos", step)
    try:
        for prefix in (None, torch.from_numpy(synth.randint(77, "prefix", (1, 9, 5), 1024)).to(DEV)):
            _, ref = _check_stream(tiny, _cond(synth.TINY_CFG, 77, cfg_scale), cfg_scale, 48, GREEDY, 5, prefix)
            assert ref.shape[2] < 48 + (0 if prefix is None else 5)
    finally:
        eng.call("zn_debug_force_eos", -1)


def test_hybrid_stream_equals_generate(dac):
    model, _ = build_model(synth.HYBRID_TINY_CFG, 3, DEV, dac=dac)
    eng = model.engine(1)
    eng.call("zn_debug_eos_bias", float("-inf"))
    try:
        _check_stream(model, _cond(synth.HYBRID_TINY_CFG, 3, 2.0), 2.0, 60, dict(min_p=0.1), 42)
    finally:
        eng.call("zn_debug_eos_bias", 0.0)
    eng.call("zn_debug_force_eos", 20)
    try:
        _check_stream(model, _cond(synth.HYBRID_TINY_CFG, 3, 1.0), 1.0, 60, GREEDY, 42)
    finally:
        eng.call("zn_debug_force_eos", -1)


def test_stream_argument_errors(tiny):
    cond = _cond(synth.TINY_CFG, 77, 2.0)
    with pytest.raises(ValueError):
        tiny.stream(torch.cat([cond, cond]), batch_size=2)
    with pytest.raises(ValueError):
        tiny.stream(cond, chunk_frames=0)


@pytest.fixture(scope="module")
def full(dac):
    model, _ = build_model(synth.FULL_CFG, 1234, DEV, dac=dac)
    return model


def test_full_10s_greedy_stream(full):
    """Zonos-v0.1 dims, 10 s (861 frames) greedy with EOS suppressed: identical to generate() + decode(), no hand-off timeout, and a
    stream left after its first chunk frees the engine for a generate() that matches a fresh run on the persistent path."""
    cond = _cond(synth.FULL_CFG, 1234, 2.0)
    eng = full.engine(1)
    eng.call("zn_debug_eos_bias", float("-inf"))
    try:
        chunks, ref = _check_stream(full, cond, 2.0, 861, GREEDY, 7)
        assert ref.shape[2] == 861 and len(chunks) > 40
        c = full.handoff_counters()
        assert c["repeated_generations"] == 0 and c["engine"]["handoff_timeouts"] == 0, c
        fresh = full.generate(cond, max_new_tokens=200, sampling_params=GREEDY, seed=7)
        g = full.stream(cond, max_new_tokens=200, sampling_params=GREEDY, seed=7)
        first = next(g)
        assert first.codes.shape[2] > 0
        g.close()
        assert not getattr(eng, "generating", False) and eng.lock.acquire(blocking=False)
        eng.lock.release()
        for c0 in full.stream(cond, max_new_tokens=200, sampling_params=GREEDY, seed=7):
            break                                          # a for loop left early
        del c0
        again = full.generate(cond, max_new_tokens=200, sampling_params=GREEDY, seed=7)
        assert eng.lib.zn_decode_path(eng.h) == 1, "the generation after the abandoned streams takes the persistent kernels"
        assert torch.equal(again, fresh)
        assert full.handoff_counters()["engine"]["handoff_timeouts"] == 0
    finally:
        eng.call("zn_debug_eos_bias", 0.0)
