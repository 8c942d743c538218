"""Zonos.serve_stream(): audio chunks per request of a served batch.  Bit for bit: per request, the concatenated codes
are the codes serve() returns for the same source and settings, and the concatenated wav is autoencoder.decode() of them."""
import pytest
import torch

from zonos_amd import synth
from zonos_amd.autoencoder import DACAutoencoder
from zonos_amd.model import GenRequest
from zonos_amd.serving import ServeChunk
from zonos_amd.testing import build_model

from test_gpu_serve import CFGS, NQ, SEEDS, _hooks, _requests, _row_len, _utt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def dac():
    return DACAutoencoder(synth.dac_state_dict(4321, encoder=False), device=DEV)


@pytest.fixture(scope="module")
def models(dac):
    built = {}

    def get(name):
        if name not in built:
            built[name] = build_model(CFGS[name], SEEDS[name], DEV, dac=dac, peaky=True)[0]
        return built[name]
    return get


def _sizes(source):
    reqs = [r for r in source if isinstance(r, GenRequest)]
    return max(_row_len(r) - 1 for r in reqs), max(int(r.max_new_tokens) for r in reqs)


def _serve(model, source, slots, guided, sched_every=8, **kw):
    max_prompt, max_new = _sizes(source)
    kw = {"max_prompt": max_prompt, "max_new_tokens": max_new, **kw}
    return {res.index: res for res in model.serve(iter(source), slots=slots, guided=guided, sched_every=sched_every, **kw)}


def _stream(model, source, slots, guided, chunk_frames, sched_every=8, **kw):
    """serve_stream() to its end -> {index: [ServeChunk]}; one done chunk per request, and it is the last."""
    max_prompt, max_new = _sizes(source)
    kw = {"max_prompt": max_prompt, "max_new_tokens": max_new, **kw}
    out = {}
    for ch in model.serve_stream(iter(source), slots=slots, guided=guided, sched_every=sched_every, chunk_frames=chunk_frames, **kw):
        assert isinstance(ch, ServeChunk)
        got = out.setdefault(ch.index, [])
        assert not (got and got[-1].done), f"request {ch.index}: a chunk after its done chunk"
        got.append(ch)
    assert all(chs[-1].done and sum(c.done for c in chs) == 1 for chs in out.values())
    return out


def _check(model, served, chunks):
    """The contract, per request -> how many requests got audio before their last chunk."""
    early = 0
    assert set(served) == set(chunks)
    for i, res in served.items():
        chs = chunks[i]
        if res.error is not None:
            assert len(chs) == 1 and chs[0].codes is None and chs[0].wav is None and chs[0].done and isinstance(chs[0].error, ValueError)
            assert str(chs[0].error) == str(res.error)
            continue
        assert all(c.error is None and c.codes.dtype == torch.int64 and c.codes.device == res.codes.device and c.wav.dtype == torch.float32
                   and c.codes.shape[:2] == (1, NQ) and c.wav.shape[:2] == (1, 1) for c in chs)
        codes = torch.cat([c.codes for c in chs], dim=2)
        assert torch.equal(codes, res.codes), f"request {i}: codes {tuple(codes.shape)} differ from serve()'s {tuple(res.codes.shape)}"
        wav = torch.cat([c.wav for c in chs], dim=2)
        ref = model.autoencoder.decode(res.codes)
        assert wav.shape == ref.shape and torch.equal(wav, ref), f"request {i}: wav differs from decode() of its codes"
        early += any(c.wav.shape[2] > 0 for c in chs[:-1])
    return early


@pytest.mark.parametrize("arch", ["transformer", "hybrid"])
@pytest.mark.parametrize("guided", [True, False], ids=["guided", "cfg1"])
def test_chunks_concatenate_to_serve_and_decode(models, arch, guided):
    """Five requests through three slots, EOS suppressed; serve() before and after the streaming sessions gives the same results."""
    model = models(arch)
    reqs = _requests(arch, guided, [6, 9, 4, 7, 5], [20, 60, 33, 41, 52], [0, 5, 0, 3, 0], base=900, stochastic=(1,))
    with _hooks(model, 3, arch):
        served = _serve(model, reqs, 3, guided)
        assert [tuple(served[i].codes.shape) for i in range(5)] == [(1, NQ, n + p) for n, p in zip([20, 60, 33, 41, 52], [0, 5, 0, 3, 0])]
        for chunk_frames in (8, 16):
            chunks = _stream(model, reqs, 3, guided, chunk_frames)
            assert _check(model, served, chunks) >= 1, "some request must hear audio before it retires"
            assert max(len(c) for c in chunks.values()) >= (4 if chunk_frames == 8 else 3)
        again = _serve(model, reqs, 3, guided)
    for i in served:
        assert torch.equal(served[i].codes, again[i].codes), f"serve() after a streaming session: request {i} differs"


@pytest.mark.parametrize("step", [0, 3, 30])
@pytest.mark.parametrize("arch", ["transformer", "hybrid"])
def test_forced_eos_at_an_own_step(models, arch, step):
    """Three requests admitted together (own step = session step) and EOS forced in codebook 0 at that step: every result is shorter
    than its budget, the EOS frame is never released early, and the tail comes with the last chunk."""
    model = models(arch)
    budgets, prefixes = [40, 60, 50], [0, 5, 3]
    reqs = _requests(arch, True, [6, 9, 4], budgets, prefixes, base=930)
    with _hooks(model, 3, arch, force=step):
        served = _serve(model, reqs, 3, True)
        chunks = _stream(model, reqs, 3, True, 8)
        _check(model, served, chunks)
    for i in range(3):
        assert served[i].codes.shape[2] < budgets[i] + prefixes[i], (i, served[i].codes.shape)


def test_a_refused_request_and_a_none_item(models):
    model = models("transformer")
    d = CFGS["transformer"]["d_model"]
    reqs = _requests("transformer", True, [6, 10, 3], [24, 30, 28], [5, 0, 1], base=960)
    too_long = GenRequest(_utt(965, 6, d).to(DEV), sampling_params=dict(temperature=0.0), cfg_scale=2.0, max_new_tokens=90)
    wrong = GenRequest(_utt(966, 6, d, 1).to(DEV), sampling_params=dict(temperature=0.0), cfg_scale=1.0, max_new_tokens=5)
    source = [reqs[0], too_long, None, reqs[1], None, wrong, None, reqs[2]]
    with _hooks(model, 2, "transformer"):
        served = _serve(model, source, 2, True, max_prompt=12, max_new_tokens=30)
        chunks = _stream(model, source, 2, True, 8, max_prompt=12, max_new_tokens=30)
        assert isinstance(served[1].error, ValueError) and isinstance(served[3].error, ValueError)
        _check(model, served, chunks)
        assert sorted(chunks) == [0, 1, 2, 3, 4], "the session goes on after a refusal"


def test_leaving_early_releases_the_engine(models):
    model = models("transformer")
    cond = _utt(977, 7, CFGS["transformer"]["d_model"]).to(DEV)
    reqs = _requests("transformer", True, [6, 10, 3], [40, 44, 30], [5, 0, 1], base=970)
    with _hooks(model, 2, "transformer"):
        before = model.generate(cond, max_new_tokens=10, cfg_scale=2.0, sampling_params=dict(temperature=0.0)).cpu()
        gen = model.serve_stream(iter(reqs), slots=2, max_prompt=12, max_new_tokens=44, guided=True, chunk_frames=8)
        first = next(gen)
        assert first.error is None and first.index in (0, 1) and not first.done
        eng = model.engine(2)
        assert eng.generating, "the engine is held while the generator is alive"
        gen.close()
        assert not eng.generating and eng.lock.acquire(blocking=False)
        eng.lock.release()
        after = model.generate(cond, max_new_tokens=10, cfg_scale=2.0, sampling_params=dict(temperature=0.0)).cpu()
    assert torch.equal(before, after)
    with pytest.raises(ValueError):
        model.serve_stream(iter(reqs), chunk_frames=0)
