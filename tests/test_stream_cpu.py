"""CPU checks of streaming (no GPU): the span planner zn_dac_span against the decoder it plans for, restated by the CPU oracle, and the
finality rule of Zonos.stream (release_limit) over every prefix of delayed-code trajectories with the reference's EOS masking."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import zonos_oracle as zo
from zonos_amd import _lib, synth
from zonos_amd.codebook_pattern import apply_delay_pattern, revert_delay_pattern
from zonos_amd.model import finalise_codes, map_codes, release_limit

NQ, EOS, MASK = 9, 1024, 1025


@pytest.fixture(scope="module")
def lib():
    from zonos_amd import build
    build.build(verbose=False)
    return _lib.load()


def span(lib, ratios, c0, n, at_end):
    zc = _lib.zn_dac_config(n_codebooks=9, codebook_size=1024, codebook_dim=8, hidden_size=64, decoder_hidden_size=64, n_ratios=len(ratios))
    for i, r in enumerate(ratios):
        zc.ratios[i] = r
    s0, s1 = C.c_int64(), C.c_int64()
    assert lib.zn_dac_span(C.byref(zc), c0, n, int(at_end), C.byref(s0), C.byref(s1)) == 0
    return s0.value, s1.value


def decode_latent(dw, z, ratios):
    """oracle.zonos_oracle.dac_decode from the latent z [B, hidden, T] on (its first step, dac_from_codes, is per frame)."""
    h = F.conv1d(z, dw["decoder.conv1.weight"], dw["decoder.conv1.bias"], padding=3)
    for bi, s in enumerate(ratios):
        b = f"decoder.block.{bi}."
        h = F.conv_transpose1d(zo.snake(h, dw[b + "snake1.alpha"]), dw[b + "conv_t1.weight"], dw[b + "conv_t1.bias"], stride=s,
                               padding=math.ceil(s / 2))
        for u, dil in ((1, 1), (2, 3), (3, 9)):
            h = zo.dac_residual_unit(dw, b + f"res_unit{u}.", h, dil)
    h = F.conv1d(zo.snake(h, dw["decoder.snake1.alpha"]), dw["decoder.conv2.weight"], dw["decoder.conv2.bias"], padding=3)
    return torch.tanh(h).float()


# the receptive field follows the ratios: the 44.1 kHz ones and a shorter, different stack (narrow channels keep the CPU decodes fast)
@pytest.mark.parametrize("ratios,T", [((8, 8, 4, 2), 40), ((4, 2), 48)], ids=["8-8-4-2", "4-2"])
def test_span_matches_windowed_oracle_decode(lib, ratios, T):
    dw = synth.dac_state_dict(99, encoder=False, hidden=64, dec_hidden=64, ratios=ratios)
    hop = int(np.prod(ratios))
    codes = torch.from_numpy(synth.randint(99, "span.codes", (1, 9, T), 1024))
    with torch.no_grad():
        whole = zo.dac_decode(dw, codes, ratios=ratios)[0, 0].double()
    # the same decode from the latent, with autograd: which latent frames a sample reads
    z = zo.dac_from_codes(dw, codes).detach().requires_grad_(True)
    wz = decode_latent(dw, z, ratios)[0, 0]
    assert torch.equal(wz.detach().double(), whole)

    def reads(s):
        with torch.enable_grad():
            g, = torch.autograd.grad(wz[s], z, retain_graph=True)
        nz = (g[0].abs().sum(0) != 0).nonzero()[:, 0]
        return int(nz.min()), int(nz.max())

    with torch.no_grad():
        windows = [(0, T, True), (0, T - 1, False), (0, 1, True), (0, 3, True), (0, 5, False), (0, 12, False), (0, 25, False), (3, 4, True),
                   (2, 30, False), (7, 21, False), (10, T - 10, True), (17, 12, False), (25, 9, False), (T - 11, 11, True), (T - 3, 3, True),
                   (5, T - 6, False), (1, 26, False)]
        nonempty = 0
        for c0, n, at_end in windows:
            assert at_end or c0 + n < T                # a window that is not the end is followed by frames in the whole decode
            s0, s1 = span(lib, ratios, c0, n, at_end)
            assert 0 <= s0 <= s1 <= (c0 + n) * hop
            if c0 == 0:
                assert s0 == 0, (c0, n, at_end, s0)
            if at_end:
                assert s1 == (c0 + n) * hop, (c0, n, s1)
            if s1 == s0:
                continue
            nonempty += 1
            # the window decoded on its own: zero padding at both of its ends, which are true edges only at frame 0 / with at_end
            win = zo.dac_decode(dw, codes[..., c0:c0 + n], ratios=ratios)[0, 0].double()
            base = c0 * hop
            ref = whole if c0 + n == T else zo.dac_decode(dw, codes[..., :c0 + n], ratios=ratios)[0, 0].double()   # (a sequence ending at c0 + n)
            inside = (win[s0 - base:s1 - base] - ref[s0:s1]).abs().max().item()
            assert inside <= 2e-6, (c0, n, at_end, inside)
            # tight, not merely safe: the sample on either side of the range reads a frame outside the window.  (At the edge of the receptive
            # field that frame's weight is ~1e-11 with these weights: the sample's VALUE moves below fp32 resolution, so the dependency
            # itself is what is checked, through autograd.)
            if not at_end:
                assert reads(s1)[1] >= c0 + n, (c0, n, "right", s1, reads(s1))
                assert reads(s1 - 1)[1] < c0 + n
            if c0 > 0:
                assert reads(s0 - 1)[0] < c0, (c0, n, "left", s0, reads(s0 - 1))
                assert reads(s0)[0] >= c0
        assert nonempty >= 6
    # windows shorter than the look-ahead hold no complete sample until the sequence ends there
    assert span(lib, ratios, 0, 1, False)[1] == 0 and span(lib, ratios, 5, 2, False)[0] == span(lib, ratios, 5, 2, False)[1]
    assert span(lib, ratios, 0, 1, True) == (0, hop)


def test_span_rejects_bad_arguments(lib):
    zc = _lib.zn_dac_config(n_ratios=2)
    zc.ratios[0], zc.ratios[1] = 8, 3
    s0, s1 = C.c_int64(), C.c_int64()
    assert lib.zn_dac_span(C.byref(zc), 0, 4, 0, C.byref(s0), C.byref(s1)) < 0      # odd stride
    zc.ratios[1] = 2
    assert lib.zn_dac_span(C.byref(zc), -1, 4, 0, C.byref(s0), C.byref(s1)) < 0
    assert lib.zn_dac_span(C.byref(zc), 0, 0, 0, C.byref(s0), C.byref(s1)) < 0
    assert lib.zn_dac_decode_span(None, None, 1, 0, 4, 0, None, None) < 0


# ---------------------------------------------------------------------------------------------------- finality rule
def run_loop(tokens: np.ndarray, max_new: int, prefix: np.ndarray | None = None):
    """The reference's loop bookkeeping (zonos/model.py:467-509 as oracle.zonos_oracle.generate restates it) replayed on a scripted token
    stream instead of a model: tokens [calls, 9] before EOS masking, call 0 the prefill's.  Returns the delayed buffer after each call with
    the column written last, and the column offset the loop ends at."""
    P = 0 if prefix is None else prefix.shape[2]
    codes = torch.full((1, NQ, P + max_new), -1, dtype=torch.int64)
    if prefix is not None:
        codes[..., :P] = torch.from_numpy(prefix)
    delayed = apply_delay_pattern(codes, MASK)
    t_total = delayed.shape[2]
    offset = P + 1
    col = delayed[:, :, offset]
    col.copy_(torch.where(col == -1, torch.from_numpy(tokens[0]).long()[None], col))
    states = [(delayed.clone(), offset)]
    max_steps = t_total - offset
    remaining, stopping, cb, call = max_steps, False, torch.arange(NQ), 1
    for step_idx in range(max_steps):
        offset += 1
        if offset >= t_total:
            break
        nxt = torch.from_numpy(tokens[call]).long() if call < len(tokens) else torch.zeros(NQ, dtype=torch.long)
        call += 1
        if int(nxt[0]) == EOS:
            remaining, stopping = min(remaining, NQ), True
        if stopping:
            eos_idx = min(NQ - remaining, NQ - 1)
            nxt = torch.where(cb < eos_idx, MASK, torch.where(cb == eos_idx, EOS, nxt))
        c = delayed[0, :, offset]
        c.copy_(torch.where(c == -1, nxt, c))
        remaining -= 1
        states.append((delayed.clone(), offset))
        if step_idx % 16 == 15 and remaining <= 0:
            break
        if step_idx % 8 == 7 and max(0, 10 - (step_idx + 1)) < 5 and remaining <= 0:
            break
    return states, offset


def check_release(states, end_offset):
    final = finalise_codes(revert_delay_pattern(states[-1][0]), end_offset, NQ, EOS)
    released = 0
    for delayed, offset in states:                         # every prefix: the columns written so far, later ones still -1 / mask
        cb0 = delayed[0, 0, 1:offset + 1]
        hit = (cb0 == EOS).nonzero()
        eos_frame = int(hit[0, 0]) if len(hit) else None
        limit = release_limit(offset, NQ, eos_frame)
        assert limit >= released                           # monotone
        assert limit <= final.shape[2], (offset, limit, final.shape)
        if limit > released:
            got = revert_delay_pattern(delayed[..., released:limit + NQ])
            assert torch.equal(map_codes(got), final[..., released:limit]), (offset, released, limit)
            released = limit
    return final, released


def test_finality_rule_on_the_golden_eos_trajectories(golden_dir):
    g = np.load(f"{golden_dir}/tiny_eos.npz")
    pre = synth.randint(int(g["seed"]), "prefix", (1, 9, int(g["prefix_len"])), 1024)
    cases = [(k, g[f"tokens_{k[4:]}"], int(g["max_new"]), None) for k in g.files if k.startswith("out_")]
    cases += [(k, g[f"ptokens_{k[5:]}"], int(g["p_max_new"]), pre) for k in g.files if k.startswith("pout_")]
    short_seen = False
    for key, tokens, max_new, prefix in cases:
        states, end = run_loop(tokens[:, 0].astype(np.int64), max_new, prefix)
        final, released = check_release(states, end)
        assert np.array_equal(final.numpy(), g[key].astype(np.int64)), key      # the replay is the reference's bookkeeping
        # the EOS frame itself is never released before the end; short clips keep it (the search window misses it)
        short_seen |= released < final.shape[2] and bool((final[0, 0] == 0).any())
    assert short_seen


@pytest.mark.parametrize("seed", range(40))
def test_finality_rule_on_random_trajectories(seed):
    rng = np.random.default_rng(seed)
    max_new = int(rng.integers(1, 90))
    calls = max_new + NQ + 2
    tokens = rng.integers(0, 1024, size=(calls, NQ)).astype(np.int64)
    if rng.random() < 0.8:                                 # codebook 0 samples EOS at some step (or never: the clip runs to max_new)
        tokens[int(rng.integers(0, calls)), 0] = EOS
    prefix = rng.integers(0, 1024, size=(1, NQ, int(rng.integers(1, 12)))) if rng.random() < 0.3 else None
    states, end = run_loop(tokens, max_new, prefix)
    final, released = check_release(states, end)
    assert released <= final.shape[2]
