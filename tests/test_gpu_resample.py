"""Output resampling on the GPU: zn_resample_rows against the float64 reference under the derived bound and against the
specification's chain bit for bit; spans, ragged rows and PCM16; and the Python surface - decode(), decode_batch(), DACAutoencoder.stream(),
stream_set(), Zonos.stream() and Zonos.serve_stream() with `sample_rate` / `pcm16` - against decode(codes, sample_rate, pcm16), bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from zonos_amd import _lib, resample as R, synth
from zonos_amd.autoencoder import DACAutoencoder, DACStream, Resampler
from zonos_amd.testing import DAC_SMALL_CODEBOOK, build_model, build_small_dac

from test_gpu_serve import _hooks, _requests, _row_len
from test_gpu_stream import _chunkings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATES = [(44100, 48000), (44100, 24000), (44100, 22050), (44100, 16000), (44100, 8000), (3, 2), (2, 3)]
IDS = [f"{a}to{b}" for a, b in RATES]
TINY = 2.0 ** -149
GREEDY = {"temperature": 0.0}


def lengths(plan):
    w, o = plan.width, plan.o
    return sorted({T for T in (1, w - 1, w, w + 1, o - 1, o, o + 1, 512, 1573) if T >= 1})


@pytest.fixture(scope="module")
def plans():
    return {r: R.ResamplePlan(*r) for r in RATES}


@pytest.fixture(scope="module")
def resamplers():
    return {r: Resampler(*r, DEV) for r in RATES}


@pytest.fixture(scope="module")
def stage_ae():
    return DACAutoencoder(device=DEV)                          # (no weights: the stage alone runs)


def library_table(rates):
    lib = _lib.load()
    o, n, w = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.zn_resample_plan(*rates, 6, 0.99, C.byref(o), C.byref(n), C.byref(w), None, None, 0, None, 0) == 0
    lo, hi = (C.c_int32 * n.value)(), (C.c_int32 * n.value)()
    table = np.zeros((n.value, 2 * w.value + o.value), dtype=np.float32)
    assert lib.zn_resample_plan(*rates, 6, 0.99, None, None, None, lo, hi, n.value, table.ctypes.data_as(C.POINTER(C.c_float)), table.size) == 0
    return table, np.array(lo[:]), np.array(hi[:])


def signals(T, seed):
    """rows: uniform [-1, 1], uniform [-3, 3], unit impulses at 0, T - 1 and the middle, a constant."""
    rng = np.random.default_rng(seed)
    x = np.zeros((6, T), dtype=np.float32)
    x[0] = rng.uniform(-1, 1, T)
    x[1] = rng.uniform(-3, 3, T)
    x[2, 0] = x[3, T - 1] = x[4, T // 2] = 1.0
    x[5] = 0.75
    return x


@pytest.mark.parametrize("rates", RATES, ids=IDS)
def test_kernel_against_float64_reference_and_table(plans, resamplers, rates):
    P, rs = plans[rates], resamplers[rates]
    table, lo, hi = library_table(rates)
    assert np.array_equal(lo, P.lo) and np.array_equal(hi, P.hi)
    lib_plan = R.ResamplePlan(*rates)
    lib_plan.table = table                                                       # the reference runs over the LIBRARY's own table
    for T in lengths(P):
        x = signals(T, 31 * T + rates[1])
        got = rs.whole(torch.from_numpy(x).to(DEV), False).cpu().numpy()
        total = P.total(T)
        assert got.shape == (6, total) and got.dtype == np.float32
        ref, A = R.resample_reference(x, lib_plan)
        j = np.arange(total)
        m = (hi - lo)[j % P.n]
        err = np.abs(got.astype(np.float64) - ref)
        bound = R.gamma(m) * A + TINY
        print(f"{rates} T={T}: max err/bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), (T, float((err / bound).max()))
        # unit impulses: the outputs ARE table entries (phase and tap indexing)
        for row, s in ((2, 0), (3, T - 1), (4, T // 2)):
            i = s - (j // P.n) * P.o + P.width
            ok = (i >= 0) & (i < P.taps)
            want = np.where(ok, table[j % P.n, np.clip(i, 0, P.taps - 1)], np.float32(0))
            assert np.array_equal(got[row], want), (T, s)
        # and the whole chain is the specification's, bit for bit
        assert np.array_equal(got[:2].view(np.int32), R.resample_chain(x[:2], lib_plan).view(np.int32)), T


def _stream_through(ae, rs, x, sizes, pcm):
    """The output stage of a DACStream over chunks of x [B, T]."""
    st = DACStream(ae, None, rs, pcm)
    parts, k = [], 0
    for s in sizes:
        parts.append(st._stage(x[:, None, k:k + s], False))
        k += s
    early = sum(p.shape[2] for p in parts)
    parts.append(st._stage(x[:, None, k:k], True))
    return torch.cat(parts, dim=2)[:, 0], early


def _span_chunkings(T):
    irregular, k, i = [], 0, 0
    while k < T:
        step = (1, 7, 0, 2, 23, 5, 0, 64, 3)[i % 9]
        irregular.append(min(step, T - k))
        k += irregular[-1]
        i += 1
    return {"all": [T], "ones": [1] * T, "irregular": irregular + [0]}


@pytest.mark.parametrize("rates", RATES, ids=IDS)
def test_spans_equal_the_whole_signal(plans, resamplers, stage_ae, rates):
    P, rs = plans[rates], resamplers[rates]
    for T in lengths(P):
        x = torch.from_numpy(signals(T, 7 * T + rates[1])[:2] * 0.5).to(DEV)
        for pcm in (False, True):
            whole = rs.whole(x, pcm)
            for name, sizes in _span_chunkings(T).items():
                if pcm and name == "ones":
                    continue                                   # (the stage's arithmetic does not depend on the output format)
                got, early = _stream_through(stage_ae, rs, x, sizes, pcm)
                assert got.dtype == whole.dtype and got.shape == whole.shape and torch.equal(got, whole), (T, name, pcm)
                if T >= 512:
                    assert early > 0


@pytest.mark.parametrize("rates", [(44100, 48000), (44100, 8000), (2, 3)], ids=["44100to48000", "44100to8000", "2to3"])
def test_ragged_rows_equal_each_row_alone(plans, resamplers, rates):
    P, rs = plans[rates], resamplers[rates]
    sig = [torch.from_numpy(np.random.default_rng(5 + i).uniform(-1, 1, T).astype(np.float32)).to(DEV)
           for i, T in enumerate((1573, 900, 2000, 40, 1200))]
    # (signal, first output, outputs or None = to what is final, at_end): a start, an interior span, an end span, a whole short signal, one output
    spec = [(0, 0.0, None, False), (1, 0.3, None, False), (2, 0.6, None, True), (3, 0.0, None, True), (4, 0.4, 1, False)]
    rows, wins = [], []
    for r, (s, frac, count, at_end) in enumerate(spec):
        T = sig[s].shape[0]
        final = P.n_final(T, at_end)
        out0 = int(frac * final)
        spec[r] = (s, out0, count, at_end)
        count = final - out0 if count is None else count
        in0 = P.first_in(out0)
        in1 = T if at_end else max(P.need(j) for j in range(out0 + max(0, count - P.n), out0 + count))
        rows.append((in0, in1 - in0, out0, count, at_end))
        wins.append(sig[s][in0:in1])
        assert count >= 1
    in_max, out_max = max(r[1] for r in rows) + 5, max(r[3] for r in rows) + 9
    x = torch.full((5, in_max), float("nan"), device=DEV)                   # NaN in every cell beyond a row's in_len
    for r, w in enumerate(wins):
        x[r, :w.shape[0]] = w
    for pcm in (False, True):
        out = torch.full((5, out_max), -7, dtype=torch.int16 if pcm else torch.float32, device=DEV)
        arr = (_lib.zn_resample_row * 5)(*[_lib.zn_resample_row(a, b, c, d, int(e)) for a, b, c, d, e in rows])
        _lib.check_resample(_lib.load().zn_resample_rows(rs._h, x.data_ptr(), in_max, arr, 5, out.data_ptr(), out_max, int(pcm),
                                                         torch.cuda.current_stream().cuda_stream), rs._h, "zn_resample_rows")
        for r, (s, out0, _, _) in enumerate(spec):
            count = rows[r][3]
            alone = rs.rows(wins[r][None].contiguous(), [rows[r]], count, pcm)[0]
            assert torch.equal(out[r, :count], alone), (r, pcm)
            assert bool((out[r, count:] == -7).all()), "the cells beyond out_count keep the sentinel"
            whole = rs.whole(sig[s][None], pcm)[0]
            assert torch.equal(alone, whole[out0:out0 + count]), "a row is a span of its whole signal"
            assert not pcm or alone.dtype == torch.int16


@pytest.mark.parametrize("rates", [(44100, 48000), (44100, 16000), (3, 2)], ids=["44100to48000", "44100to16000", "3to2"])
def test_pcm16_is_pcm16_of_the_fp32_output(resamplers, rates):
    rs = resamplers[rates]
    x = signals(1573, 3)[:2] * np.float32(0.6)
    x[0, 100:140], x[0, 300:340], x[1, 7], x[1, 9] = 1.5, -1.5, 1.5, -1.5
    xd = torch.from_numpy(x).to(DEV)
    f32, i16 = rs.whole(xd, False).cpu().numpy(), rs.whole(xd, True).cpu().numpy()
    assert i16.dtype == np.int16 and np.array_equal(i16, R.pcm16(f32))
    assert i16.max() == 32767 and i16.min() == -32767, "the clamp is reached"
    want = torch.clamp(torch.from_numpy(f32) * 32767.0, -32767.0, 32767.0).to(torch.int16).numpy()
    assert np.array_equal(i16, want), "decode_to_int16's arithmetic"


def test_identity_rate_converts_only(resamplers):
    rs = Resampler(44100, 44100, DEV)
    x = torch.from_numpy(signals(700, 11)[:2] * np.float32(1.2)).to(DEV)
    assert torch.equal(rs.whole(x, False), x)
    assert np.array_equal(rs.whole(x, True).cpu().numpy(), R.pcm16(x.cpu().numpy()))


# ------------------------------------------------------------------------------------------------ the Python surface
AUDIO = [(48000, True), (16000, False), (None, True)]


@pytest.fixture(scope="module")
def daes():
    out = {name: build_small_dac(name, device=DEV)[0] for name in ("S1", "S2")}
    out["default"] = DACAutoencoder(synth.dac_state_dict(4321, encoder=False), device=DEV)
    return out


def _codes(name, seed, tag, shape):
    return torch.from_numpy(synth.randint(seed, tag, shape, 1024 if name == "default" else DAC_SMALL_CODEBOOK)).to(DEV)


def test_decode_with_a_rate_is_the_stage_on_decode(daes):
    ae = daes["S2"]
    codes = _codes("S2", 5, "rs.decode", (2, 9, 30))
    wav = ae.decode(codes)
    assert torch.equal(ae.decode(codes, None, False), wav) and torch.equal(ae.decode(codes, ae.sampling_rate), wav)
    assert ae.resample(wav, None) is wav
    for rate, pcm in AUDIO + [(8000, True)]:
        got = ae.decode(codes, rate, pcm)
        P = R.ResamplePlan(ae.sampling_rate, rate or ae.sampling_rate)
        total = wav.shape[2] if rate is None else P.total(wav.shape[2])
        assert got.shape == (2, 1, total) and got.dtype == (torch.int16 if pcm else torch.float32)
        assert torch.equal(got, ae.resample(wav, rate, pcm))
        if rate is not None:
            want = R.resample_chain(wav.cpu().numpy(), P)
            assert np.array_equal(got.cpu().numpy(), R.pcm16(want) if pcm else want), "the specification's bits"
    assert torch.equal(ae.decode_to_int16(codes[:1]), ae.decode(codes[:1], None, True)[0, 0][:, None])


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("T", [1, 3, 30, 96])
@pytest.mark.parametrize("name", ["S1", "S2", "default"])
def test_dac_stream_with_a_rate_equals_decode(daes, name, B, T):
    ae = daes[name]
    codes = _codes(name, 41 + T, f"rs.stream.{name}.{B}", (B, 9, T))
    for rate, pcm in AUDIO:
        ref = ae.decode(codes, rate, pcm)
        for cname, sizes in _chunkings(T).items():
            st = ae.stream(None, rate, pcm)
            parts, k = [], 0
            for n in sizes:
                parts.append(st.push(codes[..., k:k + n]))
                k += n
            early = sum(p.shape[2] for p in parts)
            parts.append(st.flush())
            assert all(p.shape[:2] == (B, 1) and p.dtype == ref.dtype for p in parts)
            got = torch.cat(parts, dim=2)
            assert got.shape == ref.shape and torch.equal(got, ref), (name, cname, rate, pcm)
            if T >= 30 and cname != "all":
                assert early > 0, (name, cname, "audio before the end")


@pytest.mark.parametrize("name", ["S1", "default"])
def test_stream_set_with_a_rate_equals_decode(daes, name):
    ae = daes[name]
    lengths_ = {"a": 40, "b": 96, "c": 9}
    codes = {k: _codes(name, 300 + T, f"rs.set.{k}", (1, 9, T)) for k, T in lengths_.items()}
    for rate, pcm in AUDIO:
        ss = ae.stream_set(None, rate, pcm)
        parts, at, calls = {k: [] for k in codes}, {k: 0 for k in codes}, 0
        step = {"a": 7, "b": 16, "c": 3}
        ended = set()
        while len(ended) < 3:
            chunks, end = {}, set()
            for k in codes:
                if k in ended or (k == "c" and calls < 2):                 # "c" starts later and ends first: early
                    continue
                chunks[k] = codes[k][..., at[k]:at[k] + step[k]]
                at[k] += step[k]
                if at[k] >= lengths_[k]:
                    end.add(k)
            for k, w in ss.push(chunks, end=end).items():
                parts[k].append(w)
            ended |= end
            calls += 1
        assert len(ss) == 0
        for k in codes:
            got, ref = torch.cat(parts[k], dim=2), ae.decode(codes[k], rate, pcm)
            assert got.shape == ref.shape and got.dtype == ref.dtype and torch.equal(got, ref), (name, k, rate, pcm)
            assert sum(p.shape[2] for p in parts[k][:-1]) > 0 or lengths_[k] < 30


@pytest.mark.parametrize("name", ["S2", "default"])
def test_decode_batch_equals_decode_per_item(daes, name):
    ae = daes[name]
    items = [_codes(name, 70 + T, "rs.batch", (1, 9, T)) for T in (1, 7, 40)]
    for rate, pcm in [(None, False)] + AUDIO:
        got = ae.decode_batch(items, rate, pcm)
        assert len(got) == 3
        for c, g in zip(items, got):
            ref = ae.decode(c, rate, pcm)
            assert g.shape == ref.shape and g.dtype == ref.dtype and torch.equal(g, ref), (name, c.shape, rate, pcm)
    with pytest.raises(ValueError):
        ae.decode_batch([items[0][0]])
    with pytest.raises(ValueError):
        ae.decode(items[0], 0)


@pytest.fixture(scope="module")
def tiny(daes):
    return build_model(synth.TINY_CFG, 77, DEV, dac=daes["default"])[0]


@pytest.mark.parametrize("cfg_scale", [2.0, 1.0], ids=["guided", "cfg1"])
def test_zonos_stream_with_a_rate(tiny, cfg_scale):
    cond = synth.conditioning(77, "cond", 1 if cfg_scale == 1 else 2, 6, synth.TINY_CFG["d_model"]).to(DEV)
    eng = tiny.engine(1)
    eng.call("zn_debug_eos_bias", float("-inf"))
    try:
        kw = dict(max_new_tokens=40, cfg_scale=cfg_scale, sampling_params=GREEDY, seed=99)
        ref = tiny.generate(cond, **kw)
        chunks = list(tiny.stream(cond, chunk_frames=5, sample_rate=48000, pcm16=True, **kw))
    finally:
        eng.call("zn_debug_eos_bias", 0.0)
    assert ref.shape[2] == 40 and len(chunks) >= 3
    assert torch.equal(torch.cat([c.codes for c in chunks], dim=2), ref)
    wav, want = torch.cat([c.wav for c in chunks], dim=2), tiny.autoencoder.decode(ref, 48000, True)
    assert wav.dtype == torch.int16 and wav.shape == want.shape and torch.equal(wav, want)
    assert sum(c.wav.shape[2] for c in chunks[:-1]) > 0
    with pytest.raises(ValueError):
        tiny.stream(cond, sample_rate=0)


def test_zonos_serve_stream_with_a_rate(tiny):
    """Three requests through two slots."""
    reqs = _requests("transformer", True, [6, 9, 4], [20, 44, 33], [0, 5, 0], base=960)
    max_prompt, max_new = max(_row_len(r) - 1 for r in reqs), max(int(r.max_new_tokens) for r in reqs)
    with _hooks(tiny, 2, "transformer"):
        served = {r.index: r for r in tiny.serve(iter(reqs), slots=2, max_prompt=max_prompt, max_new_tokens=max_new)}
        got = {}
        for ch in tiny.serve_stream(iter(reqs), slots=2, max_prompt=max_prompt, max_new_tokens=max_new, chunk_frames=8, sample_rate=48000, pcm16=True):
            assert ch.error is None
            got.setdefault(ch.index, []).append(ch)
    assert set(got) == set(served) == {0, 1, 2}
    for i, chs in got.items():
        assert chs[-1].done and sum(c.done for c in chs) == 1
        codes = torch.cat([c.codes for c in chs], dim=2)
        assert torch.equal(codes, served[i].codes)
        wav, want = torch.cat([c.wav for c in chs], dim=2), tiny.autoencoder.decode(codes, 48000, True)
        assert wav.dtype == torch.int16 and wav.shape == want.shape and torch.equal(wav, want), i
    assert any(sum(c.wav.shape[2] for c in chs[:-1]) > 0 for chs in got.values())
