"""The ragged span decode on the GPU: zn_dac_decode_spans (rows with their own windows, one pass over the decoder) against decode() of
each row's whole sequence and against zn_dac_decode_span(batch = 1) on the row alone, and DACAutoencoder.stream_set() against decode().
Every comparison is torch.equal: a sample's bits depend neither on the tile it falls in nor on the other rows of the launch."""
import ctypes as C

import pytest
import torch

from zonos_amd import _lib, synth
from zonos_amd.autoencoder import DACAutoencoder
from zonos_amd.testing import DAC_SMALL_CODEBOOK, build_small_dac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 12345.0
ZN_ERR_ARG = -1

# rows (c0, n, at_end) of one call, and each row's span in frames (a transcription of the span planner run on the CPU): a true left edge,
# interior windows, true right edges and a whole one-frame clip in every set
SETS = {
    "default": ([(0, 1, 1), (0, 12, 0), (5, 30, 0), (20, 11, 1), (37, 24, 0), (7, 64, 0), (0, 3, 1), (12, 25, 1)],
                [1, 2.7, 11.4, 1.7, 5.4, 45.4, 3, 15.7]),
    "S1": ([(0, 1, 1), (0, 16, 0), (5, 30, 0), (3, 40, 0), (30, 20, 1), (7, 64, 0), (12, 25, 1)],
           [1, 2.4, 2.8, 12.8, 6.4, 36.8, 11.4]),
    "S2": ([(0, 1, 1), (0, 40, 0), (7, 64, 0), (25, 71, 0), (20, 40, 1), (12, 60, 1), (0, 3, 1)],
           [1, 13.1, 10.2, 17.2, 13.1, 33.1, 3]),
}
EMPTY_ROW = {"default": (40, 8, 1), "S1": (0, 12, 0)}
TAIL = 9          # frames that follow an interior window in its row's sequence


@pytest.fixture(scope="module")
def daes():
    out = {"default": (DACAutoencoder(synth.dac_state_dict(4321, encoder=False), device=DEV), 1024)}
    for name in ("S1", "S2"):
        out[name] = (build_small_dac(name, device=DEV)[0], DAC_SMALL_CODEBOOK)
    return out


@pytest.fixture(scope="module")
def cases(daes):
    """Per set and row: the row's own random sequence, its window, its span and the two references (computed once, never modified)."""
    out = {}
    for name, (rows, frames) in SETS.items():
        ae, cb = daes[name]
        rr = []
        for i, ((c0, n, at_end), fr) in enumerate(zip(rows, frames)):
            T = c0 + n + (0 if at_end else TAIL)
            seq = torch.from_numpy(synth.randint(500 + i, f"spans.{name}.row{i}", (1, 9, T), cb)).to(DEV)
            s0, s1 = ae.span(c0, n, at_end)
            assert s1 > s0, (name, i)                      # precondition: a row whose span is empty is an argument error
            assert abs((s1 - s0) / ae.hop - fr) <= 0.051, (name, i, (s1 - s0) / ae.hop, fr)
            win = seq[..., c0:c0 + n].to(torch.int32).contiguous()
            whole = ae.decode(seq)[0, 0, s0:s1].clone()
            single = torch.empty(1, s1 - s0, dtype=torch.float32, device=DEV)
            h = ae._handle()
            _lib.check_dac(_lib.load().zn_dac_decode_span(h, win.data_ptr(), 1, c0, n, at_end, single.data_ptr(), _lib.stream_ptr()), h, "span")
            rr.append(dict(row=(c0, n, at_end), win=win, m=s1 - s0, whole=whole, single=single[0].clone()))
        torch.cuda.synchronize()
        out[name] = rr
    return out


def _call(ae, cb, rows, wins, n_max=None, t_max=None, pad_seed=99, n_rows=None):
    """One zn_dac_decode_spans call: codes padded to n_max with valid codes drawn from another seed, wav pre-filled with a sentinel."""
    n_max = max(w.shape[2] for w in wins) if n_max is None else n_max
    t_max = max(ae.span(*r)[1] - ae.span(*r)[0] for r in rows) + 7 if t_max is None else t_max
    R = len(rows)
    codes = torch.from_numpy(synth.randint(pad_seed, "spans.pad", (max(R, 1), 9, n_max), cb)).to(torch.int32).to(DEV)
    for r, w in enumerate(wins):
        k = min(w.shape[2], n_max)
        codes[r, :, :k] = w[0, :, :k]
    wav = torch.full((max(R, 1), t_max), SENTINEL, dtype=torch.float32, device=DEV)
    arr = (_lib.zn_dac_span_row * max(R, 1))(*[_lib.zn_dac_span_row(*r) for r in rows])
    h = ae._handle()
    rc = _lib.load().zn_dac_decode_spans(h, codes.data_ptr(), n_max, arr, R if n_rows is None else n_rows, wav.data_ptr(), t_max, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, wav, (_lib.load().zn_dac_last_error(h) or b"").decode()


def _check(ae, cb, rr):
    rc, wav, err = _call(ae, cb, [c["row"] for c in rr], [c["win"] for c in rr])
    assert rc == 0, err
    for r, c in enumerate(rr):
        got = wav[r, :c["m"]]
        assert torch.equal(got, c["single"]), (r, c["row"], (got - c["single"]).abs().max().item())
        assert torch.equal(got, c["whole"]), (r, c["row"], (got - c["whole"]).abs().max().item())
        assert bool((wav[r, c["m"]:] == SENTINEL).all()), (r, c["row"], "written beyond the row's span")


@pytest.mark.parametrize("variant", ["listed", "reversed", "single"])
@pytest.mark.parametrize("name", ["default", "S1", "S2"])
def test_spans_equal_decode_and_single_row_span(daes, cases, name, variant):
    ae, cb = daes[name]
    rr = cases[name]
    if variant == "single":
        for c in rr:
            _check(ae, cb, [c])
    else:
        _check(ae, cb, rr if variant == "listed" else rr[::-1])


@pytest.mark.parametrize("name", ["default", "S1"])
def test_spans_refusals_launch_nothing(daes, cases, name):
    ae, cb = daes[name]
    rr = cases[name]
    rows, wins = [c["row"] for c in rr], [c["win"] for c in rr]
    bad = EMPTY_ROW[name]
    assert ae.span(*bad)[1] <= ae.span(*bad)[0]
    empty_win = torch.zeros(1, 9, bad[1], dtype=torch.int32, device=DEV)

    def refused(rc, wav, err, row=None):
        assert rc == ZN_ERR_ARG, (rc, err)
        assert bool((wav == SENTINEL).all()), "a refused call must launch nothing"
        if row is not None:
            assert f"row {row}" in err, err

    refused(*_call(ae, cb, rows + [bad], wins + [empty_win], t_max=ae.hop * 70), row=len(rows))
    refused(*_call(ae, cb, [bad] + rows, [empty_win] + wins, t_max=ae.hop * 70), row=0)
    # n_r > n_max: row 5 holds 64 frames
    refused(*_call(ae, cb, rows, wins, n_max=63), row=5)
    # s1_r - s0_r > t_max
    big = max(range(len(rr)), key=lambda r: rr[r]["m"])
    refused(*_call(ae, cb, rows, wins, t_max=rr[big]["m"] - 1), row=big)
    refused(*_call(ae, cb, rows, wins, n_rows=0))
    refused(*_call(ae, cb, rows * 9, wins * 9, n_rows=65))
    assert _lib.load().zn_dac_decode_spans(None, None, 1, None, 1, None, 1, None) < 0
    _check(ae, cb, rr[:3])                                 # the handle still works


def _chunks(T, start):
    sizes, k, i = [], 0, start
    while k < T:
        step = (1, 7, 2, 23, 5, 64, 3)[i % 7]              # test_gpu_stream.py's irregular chunking, each key at its own phase
        sizes.append(min(step, T - k))
        k += sizes[-1]
        i += 1
    return sizes


@pytest.mark.parametrize("name,lengths", [("default", (40, 96, 7)), ("S2", (96, 130, 1))])
def test_stream_set_equals_decode(daes, name, lengths):
    """Three keys pushed in irregular chunks, started at different calls; one ends mid-way while the others run on."""
    ae, cb = daes[name]
    clips = {k: torch.from_numpy(synth.randint(40 + k, f"set.{name}.{k}", (1, 9, T), cb)).to(DEV) for k, T in enumerate(lengths)}
    refs = {k: ae.decode(c) for k, c in clips.items()}
    plan = {k: _chunks(c.shape[2], k) for k, c in clips.items()}
    start = {0: 0, 1: 2, 2: 1}                             # the call at which a key's first chunk goes in
    pos = {k: 0 for k in clips}
    parts = {k: [] for k in clips}
    before_end = {k: 0 for k in clips}
    ss = ae.stream_set()
    call = 0
    while any(pos[k] < clips[k].shape[2] for k in clips):
        chunks, end = {}, set()
        for k, c in clips.items():
            i = call - start[k]
            if 0 <= i < len(plan[k]):
                n = plan[k][i]
                chunks[k] = c[..., pos[k]:pos[k] + n]
                pos[k] += n
                if i == len(plan[k]) - 1:
                    end.add(k)
        out = ss.push(chunks, end=end)
        assert set(out) == set(chunks)
        for k, w in out.items():
            assert w.shape[:2] == (1, 1) and w.dtype == torch.float32
            parts[k].append(w)
            if k not in end:
                before_end[k] += w.shape[2]
            else:
                assert k not in ss
        call += 1
    assert len(ss) == 0
    for k, c in clips.items():
        got = torch.cat(parts[k], dim=2)
        assert got.shape == refs[k].shape and torch.equal(got, refs[k]), (name, k)
        if c.shape[2] >= 96:
            assert before_end[k] > 0, (name, k)
    assert min(len(plan[k]) + start[k] for k in clips) < call, "one key ends while the others run"
