"""The channelizer without a GPU: its reference (tests/channelizer_ref.py) against the project's oracle DDC and against
closed forms, the row arithmetic and the argument checks of the C ABI, and the float32 model that sets the GPU tolerance."""
import ctypes as C

import numpy as np
import pytest

import channelizer_ref as CR
import spectrum_ref as R


@pytest.fixture(scope="module")
def lcg19(O):
    packed = O.lcg_bytes(6 << 19, 12345)
    return packed, R.to_complex(O, packed)


@pytest.mark.parametrize("half", [0, 1])
def test_reference_is_the_oracles_ddc(O, half):
    """Channel k of the reference IS the oracle's tuned receiver: NCO word k 2^32 / M, decimate-by-D FIR
    h = [0, w[L-1], .., w[0]]; its output s + L/D equals y[s][k] to 1e-6 of the largest value (the oracle returns
    float32), rows 0 .. 59 / 119 of 2^16 samples.  Pins indexing, the sign of frequency, the hop M/2 sign and the row <-> sample relation."""
    M, P = 1024, 4
    D = M // 2 if half else M
    L = P * M
    packed = O.lcg_bytes(6 << 16, 12345)
    x = R.to_complex(O, packed)
    w = CR.kaiser_prototype(M, P)
    ref = CR.channelizer_ref(x, M, D, w)
    h = np.concatenate([[0.0], w[::-1]]).astype(np.float32)
    assert ref.shape[0] == ((1 << 16) - L) // D + 1
    for k in (0, 1, 37, M // 2, M - 2, M - 1):
        y = O.ddc_chain(packed, [(D, h)], freg=k * 2 ** 32 // M, mix=True).astype(np.float64)
        y = y[0::2] + 1j * y[1::2]
        got = y[L // D:]                 # output m takes in sample m D: the stream's last row has no such output
        assert got.size == ref.shape[0] - 1 == (120 if half else 60)
        e = float(np.max(np.abs(got - ref[:got.size, k])) / np.max(np.abs(ref[:got.size, k])))
        print(f"D {D} channel {k}: {e:.2e} over {got.size} rows")
        assert e <= 1e-6, (D, k, e)


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("k0", [5, 300])
def test_tone_on_a_channel_centre(O, k0, half):
    """A 24-bit tone A exp(+2 pi i k0 n / M) -> the constant A sum(w) in channel k0, every row (both hops, odd and even
    k0); the neighbours read what the prototype's response says, A |W(2 pi (k0 - k) / M)|; I and Q swapped -> the conjugate
    spectrum mirrored: channel M - k0."""
    M, P, A = 1024, 4, 0.5
    D = M // 2 if half else M
    n = 1 << 15
    w = CR.kaiser_prototype(M, P)
    packed = R.tone_packed(O, n, M, [(A, k0)])
    y = CR.channelizer_ref(R.to_complex(O, packed), M, D, w)
    q = 2.0 ** -23                                              # quantisation of the tone, summed over |w|
    want = A * float(np.sum(w.astype(np.float64)))
    assert np.max(np.abs(y[:, k0] - want)) <= q * np.sum(np.abs(w)) * 2
    nn = np.arange(w.size)
    for dk in (-2, -1, 1, 2, 7):
        resp = abs(np.sum(w * np.exp(2j * np.pi * ((-dk * nn) % M) / M)))       # |W| at the tone as seen from k0 + dk
        assert np.max(np.abs(np.abs(y[:, (k0 + dk) % M]) - A * resp)) <= q * np.sum(np.abs(w)) * 2, dk
    sw = packed.reshape(-1, 6)[:, [3, 4, 5, 0, 1, 2]].reshape(-1)               # x -> j conj(x)
    ys = CR.channelizer_ref(R.to_complex(O, sw), M, D, w)
    assert np.max(np.abs(np.abs(ys[:, M - k0]) - want)) <= q * np.sum(np.abs(w)) * 2
    assert np.max(np.abs(ys[:, k0])) <= 1e-3 * want


def test_rows_arithmetic_over_ragged_cuts(pkg):
    rng = np.random.default_rng(5)
    for M, P, D in CR.combos():
        L = P * M
        before = 0
        for _ in range(60):
            n = int(rng.integers(0, 3 * L // 8)) * 8
            want = max(0, (before + n - L) // D + 1) - max(0, (before - L) // D + 1)
            assert pkg.channelizer_rows(M, D, L, before, n) == want, (M, P, D, before, n)
            before += n
    assert pkg.channelizer_rows(4096, 4096, 16384, 0, 1 << 28) == (1 << 16) - 3
    assert pkg.channelizer_rows(512, 512, 2048, 0, 1 << 20) == 0             # unsupported sizes answer 0


def test_argument_errors_without_a_device(pkg):
    L = pkg.ddc_lib()
    w = np.ones(16384, np.float32)
    pw = w.ctypes.data_as(C.POINTER(C.c_float))

    def create(nchan=1024, hop=1024, proto=pw, plen=4096, first=0, count=1024, flags=0):
        h = C.c_void_p()
        rc = L.pddc_channelizer_create(C.byref(h), 0, nchan, hop, proto, plen, first, count, flags)
        if rc == 0:
            L.pddc_channelizer_destroy(h)
        return rc

    bad = [dict(nchan=512, hop=512, plen=2048, count=512), dict(nchan=3000, hop=3000, plen=3000, count=3000),
           dict(nchan=8192, hop=8192, plen=8192, count=8192), dict(plen=3 * 1024), dict(plen=1024 + 8), dict(plen=0),
           dict(plen=16 * 1024), dict(nchan=4096, hop=4096, plen=8 * 4096, count=4096), dict(hop=256), dict(hop=2048),
           dict(hop=0), dict(first=-1), dict(first=1024), dict(count=0), dict(count=1025), dict(flags=1),
           dict(proto=None)]
    for kw in bad:
        assert create(**kw) == pkg.PDDC_EINVAL, kw
    assert L.pddc_channelizer_create(None, 0, 1024, 1024, pw, 4096, 0, 1024, 0) == pkg.PDDC_EINVAL
    import torch
    if not torch.cuda.is_available():
        assert create() == pkg.PDDC_ENODEV
        assert create(nchan=4096, hop=2048, plen=16384, first=4095, count=4096) == pkg.PDDC_ENODEV
        with pytest.raises(pkg.PddcError) as e:
            pkg.Channelizer(1024, pkg.channelizer_prototype(1024, 4))
        assert e.value.code == pkg.PDDC_ENODEV
    assert L.pddc_channelizer_process(None, None, 8, None, 0, None, None) == pkg.PDDC_EINVAL
    assert L.pddc_channelizer_set_range(None, 0, 1) == pkg.PDDC_EINVAL
    assert L.pddc_channelizer_reset(None) == pkg.PDDC_EINVAL
    assert L.pddc_channelizer_next_rows(None, 1 << 20) == 0
    assert L.pddc_channelizer_destroy(None) == 0


def test_default_prototype(pkg):
    for M, P in ((1024, 1), (1024, 8), (4096, 4)):
        w = pkg.channelizer_prototype(M, P)
        assert w.dtype == np.float32 and w.size == M * P
        assert np.array_equal(w, CR.kaiser_prototype(M, P))
        assert abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-6 and np.array_equal(w, w[::-1])
    w = pkg.channelizer_prototype(1024, 8).astype(np.float64)
    n = np.arange(w.size)
    resp = lambda f: abs(np.sum(w * np.exp(-2j * np.pi * f * n / 1024)))        # f in channel spacings
    assert resp(0.5) > 0.4 and resp(1.0) < 1e-3 and resp(1.5) < 1e-4           # -6 dB near the edge, stop band beyond


def test_float32_model_against_double(lcg19):
    """e = max |y - ref| / max |ref| over all rows and channels of the independent float32 model (complex64, float32
    fold, scipy.fft) against the double reference, for every (M, P, D) and the Kaiser and the random prototype.  This
    measurement sets the GPU tolerance: TOL = 7 x the worst case (the panorama's margin, for another factorisation and
    another order of the fold).  The worst case may not exceed channelizer_ref.MODEL_WORST, the figure TOL was derived from."""
    _, x = lcg19
    worst = 0.0
    for M, P, D in CR.combos():
        for name, w in (("kaiser", CR.kaiser_prototype(M, P)), ("random", CR.random_prototype(M, P))):
            ref = CR.channelizer_ref(x, M, D, w)
            e = CR.err(CR.channelizer_model_f32(x, M, D, w), ref)
            print(f"M {M} P {P} D {D} {name}: {e:.3e} over {ref.shape[0]} rows")
            worst = max(worst, e)
    print(f"worst {worst:.3e}, 7 x worst {7 * worst:.3e}, TOL {CR.TOL:.3e}")
    assert 7 * worst <= 3e-6
    assert worst <= 1.005 * CR.MODEL_WORST      # (three digits were written down)


def test_weak_channel_model(O):
    """A tone of 0.7 on one channel's centre and one 80 dB below it on another's (channelizer_ref.weak_channels: eight
    placements per M), 41 rows, the Kaiser prototype, every (M, P, D): the independent float32 model's error on the weak
    channel relative to that channel's own reference value, the worst row.  Its worst is WEAK_MODEL_WORST, which sets the
    GPU test's TOL_WEAK_CHAN = 7 x that.  On the reference alone: the weak channel stands 80 dB below the strong one
    within 0.01 dB in every row (the rest is the 24-bit quantisation of the two tones)."""
    worst = 0.0
    for M, P, D in CR.combos():
        w = CR.kaiser_prototype(M, P)
        e = 0.0
        for ks, kw in CR.weak_channels(M):
            assert min((ks - kw) % M, (kw - ks) % M) >= 8 and CR.far_channel(M, ks, kw) not in (ks, kw)
            x = R.to_complex(O, CR.weak_packed(O, M, P, D, ks, kw))
            ref = CR.channelizer_ref(x, M, D, w)
            assert ref.shape == (CR.WEAK_ROWS, M)
            dist = 20 * np.log10(np.abs(ref[:, ks]) / np.abs(ref[:, kw]))
            assert np.max(np.abs(dist - 80.0)) <= 0.01, (M, P, D, ks, kw)
            e = max(e, CR.weak_err(CR.channelizer_model_f32(x, M, D, w), ref, kw))
        print(f"float32 model, weak channel, M {M} P {P} D {D}: {e:.2e}")
        worst = max(worst, e)
    print(f"worst {worst:.3e}, WEAK_MODEL_WORST {CR.WEAK_MODEL_WORST:.1e}, TOL_WEAK_CHAN {CR.TOL_WEAK_CHAN:.2e}")
    assert worst <= 1e-3                               # beyond that the inputs would be badly chosen
    assert CR.WEAK_MODEL_WORST / 2 < worst <= CR.WEAK_MODEL_WORST
    assert CR.TOL_WEAK_CHAN == 7 * CR.WEAK_MODEL_WORST
