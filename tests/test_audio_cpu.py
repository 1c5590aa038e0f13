"""The audio resampler without a GPU: its reference (tests/audio_ref.py) against the cut and on tones; the host arithmetic
of the C ABI (ratio, output counts); the float32 model that sets the GPU tolerance; the argument checks."""
import ctypes as C

import numpy as np
import pytest

import audio_ref as AR


def test_ratio_helper(pkg):
    assert pkg.audio_ratio(80e6, 512, 16, 48000) == (3072, 625)
    assert pkg.audio_ratio(80e6, 2048, 1, 8000) == (128, 625)
    assert pkg.audio_ratio(80e6, 512, 4, 39062.5) == (1, 1)
    for bad in ((80e6, 512, 16, 500), (80e6 + 1, 512, 16, 48000), (80e6, 512, 16, 0)):     # M > 16 L; L, M > 2^24; no rate
        with pytest.raises(pkg.PddcError):
            pkg.audio_ratio(*bad)


def test_output_counts_for_every_cut(pkg):
    """pddc_audio_outputs equals the reference's count, ceil(N L / M) outputs after N inputs, for every cut of 1000 inputs
    into two batches; given unreduced it is the same; deep in a stream (2^60 inputs before) it still adds up."""
    for L, M in ((3072, 625), (128, 625), (1, 1), (3, 1), (1, 3)):
        total = -(-1000 * L // M)
        assert pkg.audio_outputs(L, M, 0, 1000) == total == AR.outputs(L, M, 0, 1000)
        for a in range(1001):
            first, second = pkg.audio_outputs(L, M, 0, a), pkg.audio_outputs(L, M, a, 1000 - a)
            assert first == AR.outputs(L, M, 0, a) and second == AR.outputs(L, M, a, 1000 - a), (L, M, a)
            assert first + second == total
        assert pkg.audio_outputs(7 * L, 7 * M, 123, 456) == pkg.audio_outputs(L, M, 123, 456)
        deep = 1 << 60
        assert pkg.audio_outputs(L, M, deep, 1000) == AR.outputs(L, M, deep, 1000)
    assert pkg.audio_outputs(0, 1, 0, 10) == 0 and pkg.audio_outputs(1, (1 << 24) + 1, 0, 10) == 0
    assert pkg.audio_outputs(1, 16, 0, 1) == 1 and pkg.audio_outputs(1, 16, 1, 15) == 0 and pkg.audio_outputs(1, 16, 16, 1) == 1


def test_reference_is_cut_invariant():
    """audio_ref and the float32 model give the same values when the series is cut at 0, 1, 2 and ragged lengths, batches
    shorter than T - 1 and batches without an output included; the count is ceil(n L / M)."""
    x = AR.parity_inputs(9)[:5, :600]
    cuts = [0, 1, 2, 30, 0, 31, 255, 256]
    cuts.append(600 - sum(cuts))
    for (L, M), (P, T) in (((3072, 625), (128, 64)), ((1, 16), (128, 64)), ((3, 1), (32, 1)), ((128, 625), (1024, 8))):
        g = AR.parity_prototype(L, M, P, T)
        for fn in (AR.audio_ref, AR.audio_model32):
            one = fn(x, L, M, P, T, g)
            assert one.shape == (5, -(-600 * L // M))
            assert np.array_equal(one, fn(x, L, M, P, T, g, cuts))
    # many receivers take the matrix form of the same sum: the values of the loop to rounding
    xm = np.repeat(x, 13, axis=0)
    g = AR.parity_prototype(3072, 625, 128, 32)
    assert np.max(np.abs(AR.audio_ref(xm, 3072, 625, 128, 32, g)[::13] - AR.audio_ref(x, 3072, 625, 128, 32, g))) < 1e-14


def test_an_impulse_gives_the_interpolated_prototype():
    """x = delta at input 0: y[k] = the piecewise-linear interpolation of g at (n_k + r_k / L) P, in double"""
    L, M, P, T = 5, 3, 32, 4
    g = AR.kaiser_audio_prototype(P, T, 0.4)
    x = np.zeros((1, 40), np.float32)
    x[0, 0] = 1.0
    y = AR.audio_ref(x, L, M, P, T, g)[0]
    gg = np.concatenate([g.astype(np.float64), [0.0]])
    for k in range(y.size):
        pos = k * M / L * P                          # t P + q + alpha with t = n_k
        want = np.interp(pos, np.arange(P * T + 1), gg) if pos <= P * T else 0.0
        assert abs(y[k] - want) < 1e-12, k


@pytest.mark.parametrize("L,M,P,T", [(3072, 625, 128, 32), (3, 1, 128, 32), (128, 625, 128, 64)])
def test_tone_quality_of_the_reference(pkg, L, M, P, T):
    """Tones of 300, 1000 and 2700 Hz at amplitude 0.5 through the reference with the package's prototype for the ratio
    (cutoff 0.45 min(1, L / M)): 6000 inputs, the first 400 outputs dropped, least-squares fit of the tone at the output
    rate; the residual lies >= 80 dB below the tone.  The input rates: 9765.625 Hz (3072/625, and 3/1), 39062.5 Hz (128/625)."""
    rate_in = 80e6 / 2048 if (L, M) == (128, 625) else 80e6 / 8192
    rate_out = rate_in * L / M
    g = pkg.audio_prototype(P, T, 0.45 * min(1.0, L / M))
    assert g.dtype == np.float32 and g.size == P * T and abs(float(g.astype(np.float64).sum()) - P) < 1e-3
    assert np.array_equal(g, AR.kaiser_audio_prototype(P, T, 0.45 * min(1.0, L / M)))
    i = np.arange(6000)
    for f in (300.0, 1000.0, 2700.0):
        x = (0.5 * np.cos(2 * np.pi * f * i / rate_in + 0.3)).astype(np.float32)[None, :]
        y = AR.audio_ref(x, L, M, P, T, g)[0][400:]
        k = np.arange(400, 400 + y.size)
        A = np.stack([np.cos(2 * np.pi * f * k / rate_out), np.sin(2 * np.pi * f * k / rate_out)], axis=1)
        c, *_ = np.linalg.lstsq(A, y, rcond=None)
        res = y - A @ c
        amp = float(np.hypot(*c))
        down = 20 * np.log10(amp / np.sqrt(2) / np.sqrt(np.mean(res ** 2)))
        print(f"{L}/{M} P {P} T {T}: {f:.0f} Hz comes out at {amp:.5f}, residual {down:.1f} dB below it")
        # (2700 Hz lies on the decimating prototype's band edge, 3600 Hz at -6 dB: 0.47 there, 0.5 elsewhere)
        assert 0.4 < amp < 0.51 and down >= 80.0, (f, amp, down)


def test_pcm_reference():
    s = 32767.0
    y = np.array([(h + 0.5) / s for h in range(-5, 6)] + [1.5, -1.5, np.inf, -np.inf, np.nan, 0.0, 1.0, -1.0], np.float32)
    p = AR.pcm_ref(y, s)
    want = np.rint((y[:11] * np.float32(s)).astype(np.float64)).astype(np.int16)           # ties to even
    assert p.dtype == np.int16 and list(p[:11]) == list(want)
    assert list(p[11:]) == [32767, -32768, 32767, -32768, 0, 0, 32767, -32767]
    assert list(AR.pcm_ref(np.array([0.5, 1.5, 2.5, -0.5, -1.5], np.float32), 1.0)) == [0, 2, 2, 0, -2]


def test_float32_model_against_double():
    """The measurement that sets TOL_AUDIO: the float32 model against the double reference on the GPU parity test's very
    inputs (|x| <= 1), every ratio with every (P, T).  TOL = 7 x the worst case; a re-measurement may not exceed the
    written worst case by more than 0.5 %."""
    worst = {}
    for nrx in (9, 1024):
        x = AR.parity_inputs(nrx)
        assert float(np.max(np.abs(x))) <= 1.0
        for L, M in AR.RATIOS:
            for P, T in AR.SHAPES:
                g = AR.parity_prototype(L, M, P, T)
                e = float(np.max(np.abs(AR.audio_model32(x, L, M, P, T, g).astype(np.float64) - AR.audio_ref(x, L, M, P, T, g))))
                worst[(P, T)] = max(worst.get((P, T), 0.0), e)
    for k, v in worst.items():
        print(f"(P, T) = {k}: worst |model32 - ref| {v:.3e}")
    w = max(worst.values())
    print(f"worst {w:.3e} (written {AR.MODEL_WORST_AUDIO:.3e}, TOL_AUDIO {AR.TOL_AUDIO:.3e})")
    assert w <= 1.005 * AR.MODEL_WORST_AUDIO
    assert AR.TOL_AUDIO == 7 * AR.MODEL_WORST_AUDIO


def test_argument_errors_without_a_device(pkg):
    L = pkg.ddc_lib()
    good = dict(nrx=4, L=3072, M=625, phases=128, taps=32, scale=32767.0)

    def create(proto="ok", null_out=False, **kw):
        a = dict(good, **kw)
        n = max(a["phases"] * a["taps"], 1) if a["phases"] > 0 and a["taps"] > 0 else 1
        g = np.full(min(n, 1 << 20), 0.01, np.float32)
        if callable(proto):
            proto(g)
        h = C.c_void_p()
        rc = L.pddc_audio_create(None if null_out else C.byref(h), 0, a["nrx"], a["L"], a["M"], a["phases"], a["taps"],
                                 None if proto is None else g.ctypes.data_as(C.POINTER(C.c_float)), a["scale"])
        if rc == 0:
            L.pddc_audio_destroy(h)
        return rc

    def poke(i, v):
        def f(g):
            g[i] = v
        return f

    nan, inf = float("nan"), float("inf")
    bad = [dict(nrx=0), dict(nrx=-1), dict(nrx=1025), dict(L=0), dict(M=0), dict(L=(1 << 24) + 1), dict(M=(1 << 24) + 1, L=1 << 23),
           dict(L=1, M=17), dict(L=1000, M=16001), dict(phases=16), dict(phases=2048, taps=1), dict(phases=96), dict(phases=0),
           dict(taps=0), dict(taps=65), dict(phases=1024, taps=9), dict(phases=256, taps=33), dict(scale=0.0), dict(scale=-1.0),
           dict(scale=nan), dict(scale=inf), dict(proto=None), dict(proto=poke(0, nan)), dict(proto=poke(4095, inf)),
           dict(proto=poke(17, -inf)), dict(null_out=True)]
    for kw in bad:
        assert create(**kw) == pkg.PDDC_EINVAL, kw
    import torch
    if not torch.cuda.is_available():
        assert create() == pkg.PDDC_ENODEV
        assert create(nrx=1024, L=1, M=16, phases=1024, taps=8, scale=1e-30) == pkg.PDDC_ENODEV
        assert create(L=1 << 24, M=1 << 24, phases=32, taps=1) == pkg.PDDC_ENODEV
        with pytest.raises(pkg.PddcError) as e:
            pkg.Audio(4, 3072, 625)
        assert e.value.code == pkg.PDDC_ENODEV
    with pytest.raises(pkg.PddcError) as e:
        pkg.Audio(4, 1, 17)
    assert e.value.code == pkg.PDDC_EINVAL
    with pytest.raises(pkg.PddcError):
        pkg.Audio(4, 3, 1, phases=128, taps=32, proto=np.zeros(100, np.float32))
    c = C.c_size_t()
    assert L.pddc_audio_process(None, None, 8, 8, None, 8, None, 8, C.byref(c), None) == pkg.PDDC_EINVAL
    assert L.pddc_audio_next_outputs(None, 8, C.byref(c)) == pkg.PDDC_EINVAL
    assert L.pddc_audio_reset(None) == pkg.PDDC_EINVAL
    assert L.pddc_audio_destroy(None) == 0
