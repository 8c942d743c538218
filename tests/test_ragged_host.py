"""Utterances of different prompt lengths in one generate() call - the parts that need no GPU: the padding helper
(conditioning.pad_conditionings), generate()'s `conditioning_lengths` checks (they raise before any device call) and the 2-rank gloo
run of parallel.generate_sharded over conditionings of different lengths."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from zonos_amd import _lib, parallel, synth
from zonos_amd.conditioning import pad_conditionings


def _conds(lengths, halves, d=8):
    return [torch.arange(halves * L * d, dtype=torch.float32).view(halves, L, d) + 1000.0 * (i + 1) for i, L in enumerate(lengths)]


def test_pad_conditionings_guided_row_order_padding_and_lengths():
    lengths = [5, 2, 7]
    conds = [c.to(torch.bfloat16) for c in _conds(lengths, 2)]
    out, lens = pad_conditionings(conds, cfg_scale=2.0)
    assert lens == lengths and out.shape == (6, 7, 8) and out.dtype == torch.bfloat16
    for i, (c, L) in enumerate(zip(conds, lengths)):
        assert torch.equal(out[i, :L], c[0]) and torch.equal(out[3 + i, :L], c[1])          # [cond_0..cond_2, uncond_0..uncond_2]
        assert (out[i, L:] == 0).all() and (out[3 + i, L:] == 0).all()                      # right-padded with zeros


def test_pad_conditionings_without_guidance():
    lengths = [3, 6]
    conds = _conds(lengths, 1)
    out, lens = pad_conditionings(conds, cfg_scale=1.0)
    assert lens == lengths and out.shape == (2, 6, 8)
    assert torch.equal(out[0, :3], conds[0][0]) and (out[0, 3:] == 0).all() and torch.equal(out[1], conds[1][0])
    with pytest.raises(ValueError):
        pad_conditionings(_conds(lengths, 2), cfg_scale=1.0)           # [cond ‖ uncond] rows without guidance
    with pytest.raises(ValueError):
        pad_conditionings(conds, cfg_scale=2.0)                        # one row per utterance with guidance
    with pytest.raises(ValueError):
        pad_conditionings([], cfg_scale=2.0)


def test_generate_checks_conditioning_lengths_before_any_device_call():
    """The model sits on the CPU: a call that passed the checks would reach the device check ("MI355X only"); the length checks come
    first and raise ValueError."""
    from zonos_amd.testing import build_model
    model, _ = build_model(synth.TINY_CFG, 77, "cpu")
    d = synth.TINY_CFG["d_model"]
    c4 = synth.conditioning(77, "cond", 4, 6, d)
    kw = dict(max_new_tokens=4, cfg_scale=2.0, batch_size=2)
    with pytest.raises(ValueError, match="batch_size=2 lengths"):
        model.generate(c4, conditioning_lengths=[6], **kw)
    with pytest.raises(ValueError, match="batch_size=2 lengths"):
        model.generate(c4, conditioning_lengths=[6, 6, 6, 6], **kw)        # one length per utterance, not per row
    with pytest.raises(ValueError, match=r"1\.\.6"):
        model.generate(c4, conditioning_lengths=[6, 0], **kw)
    with pytest.raises(ValueError, match=r"1\.\.6"):
        model.generate(c4, conditioning_lengths=[7, 3], **kw)
    with pytest.raises(ValueError, match="lengths"):
        model.generate(c4[:2], conditioning_lengths=[6, 3, 2], max_new_tokens=4, cfg_scale=1.0, batch_size=2)
    with pytest.raises(_lib.ZonosHipError, match="MI355X only"):
        model.generate(c4, conditioning_lengths=[6, 3], **kw)
    with pytest.raises(_lib.ZonosHipError, match="MI355X only"):
        model.generate(c4[:2], conditioning_lengths=(4, 6), max_new_tokens=4, cfg_scale=1.0, batch_size=2)


# ---------------------------------------------------------------------------------------------- 2 ranks over gloo
LENGTHS = [3, 5, 3, 3, 4, 3, 6, 3, 3, 3, 3, 3]        # utterance i -> rank i % 2; batch 3: rank 0 gets (3, 3, 4) then (6, 3, 3), rank 1 (5, 3, 3) then (3, 3, 3)


def _cond(i):
    return torch.full((2, LENGTHS[i], 4), float(i + 1))


def _solo(cond):
    """Deterministic stand-in for one utterance: content derived from its VALID conditioning only."""
    seed = int(cond.abs().sum().item() * 1000) % 9973
    return torch.randint(0, 1024, (1, 9, 5), generator=torch.Generator().manual_seed(seed), dtype=torch.int64)


def _fake_generate_batch(cond, b, lengths=None):
    """Batched stand-in.  It records how it was called in the codes' last column: 0 = two arguments (one length), 1 = with lengths."""
    assert cond.shape[0] == 2 * b
    if lengths is None:
        lens = [cond.shape[1]] * b
    else:
        assert len(lengths) == b and max(lengths) == cond.shape[1] and len(set(lengths)) > 1, lengths
        for j, L in enumerate(lengths):
            assert (cond[j, L:] == 0).all() and (cond[b + j, L:] == 0).all()                  # zero padding behind the valid positions
        lens = lengths
    singles = [_solo(torch.stack([cond[j, :lens[j]], cond[b + j, :lens[j]]])) for j in range(b)]
    flag = torch.full((b, 9, 1), 0 if lengths is None else 1, dtype=torch.int64)
    return torch.cat([torch.cat(singles, dim=0), flag], dim=2)


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        out = parallel.generate_sharded(_fake_generate_batch, [_cond(i) for i in range(len(LENGTHS))], gather=True, batch_size=3)
        q.put((rank, [o.tolist() for o in out]))
    finally:
        dist.destroy_process_group()


def test_two_rank_sharding_over_conditionings_of_different_lengths():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    # groups: rank 0 utterances (0, 2, 4) lengths (3, 3, 4) and (6, 8, 10) lengths (6, 3, 3): with lengths; rank 1 (1, 3, 5) lengths (5, 3, 3): with
    # lengths, (7, 9, 11) lengths (3, 3, 3): the two-argument call
    ragged = {0, 2, 4, 6, 8, 10, 1, 3, 5}
    want = []
    for i in range(len(LENGTHS)):
        codes = torch.cat([_solo(_cond(i))[0], torch.full((9, 1), 1 if i in ragged else 0, dtype=torch.int64)], dim=1)
        want.append(codes.tolist())
    assert results[0] == want and results[1] == want               # utterance order, each from its own valid conditioning
