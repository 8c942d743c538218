"""Output resampling without a GPU: the library's host side (zn_resample_plan, zn_resample_span, the refusals of
zn_resample_rows) against zonos_amd/resample.py, the module's fp32 chain against `sinc_resample`, and the stream stage's `cat == whole`."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from zonos_amd import _lib, resample as R
from zonos_amd.autoencoder import sinc_resample

# o -> n under test, as rates (the plan divides by the gcd): 147->160, 147->80, 2->1, 441->160, 441->80 and the hand-checkable 3->2, 2->3
RATES = [(44100, 48000), (44100, 24000), (44100, 22050), (44100, 16000), (44100, 8000), (3, 2), (2, 3)]
IDS = [f"{a}to{b}" for a, b in RATES]
SUPPORT_MAX = {48000: (13, 161), 24000: (23, 171), 22050: (25, 28), 16000: (34, 475), 8000: (67, 509)}
TINY = 2.0 ** -149


def lengths(plan):
    w, o = plan.width, plan.o
    return sorted({T for T in (1, w - 1, w, w + 1, o - 1, o, o + 1, 512, 1573) if T >= 1})


@pytest.fixture(scope="module")
def lib():
    from zonos_amd import build
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def plans():
    return {r: R.ResamplePlan(*r) for r in RATES}


def lib_plan(lib, orig, new):
    o, n, w = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.zn_resample_plan(orig, new, 6, 0.99, C.byref(o), C.byref(n), C.byref(w), None, None, 0, None, 0) == 0
    lo, hi = (C.c_int32 * n.value)(), (C.c_int32 * n.value)()
    table = np.zeros((n.value, 2 * w.value + o.value), dtype=np.float32)
    assert lib.zn_resample_plan(orig, new, 6, 0.99, None, None, None, lo, hi, n.value, table.ctypes.data_as(C.POINTER(C.c_float)), table.size) == 0
    return o.value, n.value, w.value, np.array(lo[:]), np.array(hi[:]), table


def uniform(T, seed, scale=1.0):
    return (np.random.default_rng(seed).uniform(-1.0, 1.0, T) * scale).astype(np.float32)


@pytest.mark.parametrize("rates", RATES, ids=IDS)
def test_library_plan_equals_the_modules(lib, plans, rates):
    P = plans[rates]
    o, n, w, lo, hi, table = lib_plan(lib, *rates)
    g = math.gcd(*rates)
    assert (o, n) == (rates[0] // g, rates[1] // g) == (P.o, P.n) and w == P.width == math.ceil(6 * o / (min(o, n) * 0.99))
    assert table.shape == P.table.shape == (n, 2 * w + o)
    k = np.abs(P.table.astype(np.float64))
    assert (np.abs(table.astype(np.float64) - P.table) <= 2.0 ** -23 * k + TINY).all()
    assert np.array_equal(lo, P.lo) and np.array_equal(hi, P.hi), "equal supports"
    # the supports are what they say: nonzero at both ends, zero outside
    for p in range(n):
        assert table[p, lo[p]] != 0 and table[p, hi[p] - 1] != 0 and not table[p, :lo[p]].any() and not table[p, hi[p]:].any()
    if rates[1] in SUPPORT_MAX and rates[0] == 44100:
        assert (int(P.m.max()), P.taps) == SUPPORT_MAX[rates[1]]
        assert P.m.max() * n * 4 <= 22 * 1024, "the device table [tap][phase] over the supports"


def test_hand_checkable_plans(plans):
    """3 -> 2 and 2 -> 3: base = 1.98, width = ceil(6 o / 1.98); phase 0's centre tap (t = 0) is base / o, and a constant comes out as
    (nearly) itself: every phase's taps sum to 1 within the window's ripple."""
    for rates, width in (((3, 2), 10), ((2, 3), 7)):
        P = plans[rates]
        assert (P.o, P.n, P.width) == (*rates, width)
        assert P.table[0, P.width] == np.float32(P.base / P.o)
        assert np.abs(P.table.astype(np.float64).sum(1) - 1.0).max() < 2e-2


@pytest.mark.parametrize("rates", RATES, ids=IDS)
def test_library_span_equals_brute_force_over_the_supports(lib, plans, rates):
    P = plans[rates]
    o, n, w = P.o, P.n, P.width
    horizon = 3 * o + 2 * w
    j_max = P.total(horizon) + 3 * n
    need = np.array([(j // n) * o - w + P.hi[j % n] for j in range(j_max + n)])
    reads = np.array([(j // n) * o - w + P.lo[j % n] for j in range(j_max + n)])
    for at_end in (0, 1):
        for avail in range(horizon + 1):
            nf, fi = C.c_int64(), C.c_int64()
            assert lib.zn_resample_span(*rates, 6, 0.99, avail, at_end, -1, C.byref(nf), C.byref(fi)) == 0
            if at_end:
                want = -((-n * avail) // o)
            else:
                not_final = np.nonzero(need > avail)[0]
                want = int(not_final[0])                                   # the leading outputs whose every input exists
                assert want <= -((-n * avail) // o), "a stream never runs ahead of the whole signal's length"
            assert nf.value == want == P.n_final(avail, bool(at_end)), (avail, at_end)
            first = max(0, int(reads[want:want + n].min()))
            assert fi.value == first == P.first_in(want), (avail, at_end)
            assert fi.value >= max(0, int(reads[want:].min())), "no later output reads an earlier input"
            if not at_end:
                assert avail - fi.value <= 2 * w + o, "the tail a stream keeps is bounded by the filter"
    # held back: an output is final at most `width` inputs beyond its own position (+1: the position rounds down)
    pos = np.array([(j // n) * o + ((j % n) * o) // n for j in range(j_max)])
    assert (need[:j_max] - pos <= w + 1).all()


@pytest.mark.parametrize("rates", RATES, ids=IDS)
def test_chain_against_sinc_resample(plans, rates):
    P = plans[rates]
    for T in lengths(P):
        x = uniform(T, 1000 + T)
        y = R.resample_chain(x, P)
        ref = sinc_resample(torch.from_numpy(x)[None, None], *rates)[0, 0].numpy()
        assert y.shape == ref.shape == (math.ceil(P.n * T / P.o),)
        ref64, A = R.resample_reference(x, P)
        m = P.m[np.arange(len(y)) % P.n]
        assert (np.abs(y.astype(np.float64) - ref64) <= R.gamma(m) * A + TINY).all(), ("chain vs float64", T)
        assert (np.abs(y.astype(np.float64) - ref.astype(np.float64)) <= 2 * R.gamma(m) * A + TINY).all(), ("chain vs sinc_resample", T)


def chunkings(T):
    irregular, k, i = [], 0, 0
    while k < T:
        step = (1, 7, 0, 2, 23, 5, 0, 0, 64, 3)[i % 10]                       # with empty pushes
        irregular.append(min(step, T - k))
        k += irregular[-1]
        i += 1
    return {"all": [T], "ones": [1] * T, "irregular": irregular + [0]}


@pytest.mark.parametrize("pcm", [False, True], ids=["f32", "pcm16"])
@pytest.mark.parametrize("rates", RATES, ids=IDS)
def test_stream_stage_concatenates_to_the_whole(plans, rates, pcm):
    P = plans[rates]
    for T in lengths(P):
        if T > 512 and rates[0] != 44100:
            continue
        x = uniform(T, 2000 + T, 1.5).reshape(1, T)
        whole = R.resample_chain(x, P)
        whole = R.pcm16(whole) if pcm else whole
        for name, sizes in chunkings(T).items():
            if name == "ones" and T > 512:
                continue
            st, parts, k, held = R.ResampleStream(P, pcm), [], 0, 0
            for s in sizes:
                parts.append(st.push(x[:, k:k + s]))
                k += s
                held = max(held, st.tail.shape[-1])
            early = sum(p.shape[-1] for p in parts)
            parts.append(st.push(x[:, k:k], at_end=True))
            got = np.concatenate(parts, axis=-1)
            assert got.dtype == whole.dtype and np.array_equal(got, whole), (T, name)
            assert held <= 2 * P.width + P.o
            if T >= 512:
                assert early > 0, "outputs before the end"
            with pytest.raises(RuntimeError):
                st.push(x[:, :0])


def test_pcm16_is_decode_to_int16s_arithmetic():
    y = np.array([0.0, 1.0, -1.0, 1.5, -1.5, 0.5, -0.5, 3.0518e-5, -3.0518e-5, 0.99999, 2.0 ** -20], dtype=np.float32)
    want = torch.clamp(torch.from_numpy(y) * 32767.0, -32767.0, 32767.0).to(torch.int16).numpy()
    assert np.array_equal(R.pcm16(y), want)
    assert R.pcm16(y)[:5].tolist() == [0, 32767, -32767, 32767, -32767]
    big = uniform(4096, 5, 1.2)
    assert np.array_equal(R.pcm16(big), torch.clamp(torch.from_numpy(big) * 32767.0, -32767.0, 32767.0).to(torch.int16).numpy())


def test_fma_emulation_is_exact():
    """_fma32 against exact rational arithmetic rounded once, on operands chosen to sit near fp32 rounding ties."""
    from fractions import Fraction
    rng = np.random.default_rng(9)
    a = rng.uniform(-1, 1, 400).astype(np.float32)
    b = rng.uniform(-1, 1, 400).astype(np.float32)
    c = (rng.uniform(-1, 1, 400) * 2.0 ** rng.integers(-30, 3, 400)).astype(np.float32)
    a[:8] = np.float32(1 + 2.0 ** -23)
    b[:8] = np.float32(1 + 2.0 ** -23)                                        # (1 + u')^2 = 1 + 2u' + u'^2: a tie broken by the last term
    c[:8] = np.array([0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -47, -2.0 ** -46, 1, -1, 2.0 ** -60], dtype=np.float32)
    got = R._fma32(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))                                         # float(): correctly rounded to 53 bits; walk to the nearest fp32
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.int32)) & 1))
        assert got[i] == best, (i, a[i], b[i], c[i])


def _row(in0, in_len, out0, count, at_end):
    return _lib.zn_resample_row(in0, in_len, out0, count, int(at_end))


def test_refusals(lib, plans):
    msg = lambda h=None: lib.zn_resampler_last_error(h).decode()
    # rates < 1
    for bad in ((0, 48000), (44100, 0), (-1, 5)):
        assert lib.zn_resample_plan(*bad, 6, 0.99, None, None, None, None, None, 0, None, 0) == -1 and "rates" in msg()
        assert lib.zn_resample_span(*bad, 6, 0.99, 10, 0, -1, None, None) == -1
        h = C.c_void_p()
        assert lib.zn_resampler_create(*bad, 6, 0.99, C.byref(h)) == -1 and not h.value
        with pytest.raises(ValueError):
            R.ResamplePlan(*bad)
    assert lib.zn_resample_plan(44100, 48000, 0, 0.99, None, None, None, None, None, 0, None, 0) == -1
    assert lib.zn_resample_plan(44100, 48000, 6, 1.5, None, None, None, None, None, 0, None, 0) == -1
    assert lib.zn_resample_plan(44100, 44101, 6, 0.99, None, None, None, None, None, 0, None, 0) == -4, "a table beyond the limit"
    lo = (C.c_int32 * 4)()
    assert lib.zn_resample_plan(44100, 48000, 6, 0.99, None, None, None, lo, None, 4, None, 0) == -1 and "phases" in msg()
    # rows: creating a handle and refusing a call touch no device
    P = plans[(44100, 48000)]
    h = C.c_void_p()
    assert lib.zn_resampler_create(44100, 48000, 6, 0.99, C.byref(h)) == 0 and h.value
    try:
        call = lambda rows, n, in_max=4096, out_max=8192: lib.zn_resample_rows(h, None, in_max, rows, n, None, out_max, 0, None)
        one = (_lib.zn_resample_row * 1)(_row(0, 1000, 0, 10, False))
        assert call(one, 0) == -1 and "1..64" in msg(h)
        many = (_lib.zn_resample_row * 65)(*[_row(0, 1000, 0, 10, False)] * 65)
        assert call(many, 65) == -1 and "1..64" in msg(h)
        assert call(None, 1) == -1
        T = 1000
        final = P.n_final(T, False)
        ok = (_lib.zn_resample_row * 1)(_row(0, T, 0, final, False))
        assert call(ok, 1) == -1 and msg(h) == "zn_resample_rows: bad argument", "a legal window gets as far as the NULL buffers"
        # one output too many for a window that is not the signal's end
        over = (_lib.zn_resample_row * 2)(_row(0, T, 0, final, False), _row(0, T, 0, final + 1, False))
        assert call(over, 2) == -1 and "row 1" in msg(h) and "window ends" in msg(h)
        with pytest.raises(ValueError):
            R.resample_chain(np.zeros(T, np.float32), P, 0, 0, final + 1, at_end=False)
        # ... which the end of the signal allows, up to the signal's own length
        total = P.total(T)
        assert call((_lib.zn_resample_row * 1)(_row(0, T, 0, total, True)), 1) == -1 and msg(h) == "zn_resample_rows: bad argument"
        assert call((_lib.zn_resample_row * 1)(_row(0, T, 0, total + 1, True)), 1) == -1 and "row 0" in msg(h) and "has" in msg(h)
        # a window that starts after an input that the first output reads
        j0 = 700
        first = P.first_in(j0)
        good = (_lib.zn_resample_row * 1)(_row(first, T - first, j0, final - j0, False))
        assert call(good, 1) == -1 and msg(h) == "zn_resample_rows: bad argument"
        late = (_lib.zn_resample_row * 3)(_row(0, T, 0, final, False), _row(first, T - first, j0, final - j0, False), _row(first + 1, T - first - 1, j0, final - j0, False))
        assert call(late, 3) == -1 and "row 2" in msg(h) and "window starts" in msg(h)
        with pytest.raises(ValueError):
            R.resample_chain(np.zeros(T - first - 1, np.float32), P, first + 1, j0, final - j0, at_end=False)
        # the rows' own sizes
        assert call(ok, 1, in_max=T - 1) == -1 and "in_max" in msg(h)
        assert call(ok, 1, out_max=final - 1) == -1 and "out_max" in msg(h)
        assert call((_lib.zn_resample_row * 1)(_row(-1, T, 0, 1, False)), 1) == -1 and "row 0" in msg(h)
        # nothing to compute launches nothing and needs no buffers
        assert call((_lib.zn_resample_row * 2)(_row(0, T, 0, 0, False), _row(5, 0, 3, 0, True)), 2) == 0
    finally:
        assert lib.zn_resampler_destroy(h) == 0
    assert lib.zn_resampler_destroy(None) == 0
    assert lib.zn_resample_rows(None, None, 1, None, 1, None, 1, 0, None) == -1


def test_python_surface_refuses_bad_rates_without_a_device():
    from zonos_amd.autoencoder import DACAutoencoder
    ae = DACAutoencoder(device="cpu")
    assert ae._resampler(None, False) is None and ae._resampler(44100, False) is None, "the codec's rate in fp32 is no stage at all"
    for bad in (0, -8000, 22050.5):
        with pytest.raises(ValueError):
            ae._resampler(bad, False)
    with pytest.raises(_lib.ZonosHipError):
        ae._resampler(48000, False)
