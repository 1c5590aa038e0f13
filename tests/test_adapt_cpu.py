"""The adaptive filter without a GPU: that the reference (tests/adapt_ref.py) does the job -- it removes a carrier and
raises a tone's SNR --, its own properties, the argument checks of the C ABI, and the preconditions the GPU tests' inputs
have to meet."""
import ctypes as C

import numpy as np
import pytest

import adapt_ref as AR

F32 = np.float32
SETTINGS = ((64, 1), (16, 1), (128, 16))          # (T, D) at mu = 0.25, leak = 2^-10, eps = 1e-6
TONE_F = 0.0731


def same(a, b):
    return np.array_equal(AR.bits(a), AR.bits(b))


@pytest.mark.parametrize("T,D", SETTINGS)
def test_the_reference_notches_a_carrier_and_reduces_noise(T, D):
    """A tone 0.5 cos(2 pi 0.0731 m + 0.3) in Gaussian noise of sigma 0.05, n = 3000, over the second half: NOTCH leaves
    the tone's component at least 30 dB down (measured 42 dB at all three settings), NR raises the SNR by at least 3 dB
    (measured 17.1 -> 23.9 dB at T = 64, 21.6 dB at T = 16, 25.0 dB at T = 128 / D = 16)."""
    n, h = 3000, 1500
    tone, noise = AR.tone_noise(n, 1)
    x = (tone + noise).astype(F32)[None, :].repeat(2, axis=0)
    out, w, _ = AR.adapt_ref(x, [(AR.NOTCH, 0.25, 2.0 ** -10), (AR.NR, 0.25, 2.0 ** -10)], T, D)
    a_in, _ = AR.tone_part(x[0], TONE_F, h)
    a_out, _ = AR.tone_part(out[0], TONE_F, h)
    notch_db = 20 * np.log10(a_in / a_out)

    def snr(v):
        a, fit = AR.tone_part(v, TONE_F, h)
        return 10 * np.log10(0.5 * a * a / np.mean((np.asarray(v[h:], np.float64) - fit) ** 2))

    gain = snr(out[1]) - snr(x[1])
    print(f"T {T} D {D}: notch {notch_db:.1f} dB, SNR {snr(x[1]):.1f} -> {snr(out[1]):.1f} dB")
    assert notch_db >= 30.0 and gain >= 3.0
    assert same(w[0], w[1])                       # the weights do not depend on which output is taken


def test_reference_zeros_stay_plus_zero():
    x = np.zeros((3, 400), F32)
    out, w, _ = AR.adapt_ref(x, [(m, 0.5, 2.0 ** -6) for m in AR.MODES], 32, 7)
    assert not AR.bits(out).any() and not AR.bits(w).any()


def test_reference_streaming_equals_one_batch():
    K, n = 12, 1100
    x, rx = AR.audio_series(K, n, 3)[:, :n], AR.interleaved_rx(K)
    for T, D in ((16, 1), (32, 7), (64, 255), (128, 256)):
        out, w, _ = AR.adapt_ref(x, rx, T, D)
        cuts = [0, 1, 2, 0, D, D + T - 1, 97, 1, 0]
        cuts.append(n - sum(cuts))
        assert cuts[-1] > 0
        out2, w2, _ = AR.adapt_ref(x, rx, T, D, cuts=cuts)
        assert same(out, out2) and same(w, w2), (T, D)


def test_reference_off_passes_the_bits_and_holds_the_weights():
    K, n = 4, 600
    x = AR.audio_series(K, n, 4)
    x[2, 300] = -0.0
    rx = [(AR.NR, 0.5, 2.0 ** -10)] * K
    plain = AR.AdaptRef(rx, 32, 3)
    r = AR.AdaptRef(rx, 32, 3)
    a = r.process(x[:, :200])
    plain.process(x[:, :200])
    held = r.weights.copy()
    r.set_rx(2, AR.OFF, 0.5, 2.0 ** -10)
    b = r.process(x[:, 200:400])
    assert same(b[2], x[2, 200:400]) and same(r.weights[2], held[2]) and held[2].any()
    r.set_rx(2, AR.NR, 0.5, 2.0 ** -10)
    c = r.process(x[:, 400:])
    # switched on again it goes on from the held weights over the inputs that went by meanwhile
    again = AR.AdaptRef(rx[:1], 32, 3)
    again.weights = held[2:3].copy()
    again.hist = x[2:3, 400 - 34:400].copy()
    assert same(c[2], again.process(x[2:3, 400:])[0])
    full = np.concatenate([a, b, c], axis=1)
    want = np.concatenate([plain.process(x[:, 200:400]), plain.process(x[:, 400:])], axis=1)
    for j in (0, 1, 3):
        assert same(full[j, 200:], want[j])
    assert not same(full[2, 400:], want[2, 200:])


def test_reference_restart_zeroes_one_receiver_only():
    K, n = 5, 500
    x = AR.audio_series(K, n, 5)
    rx = AR.interleaved_rx(K)
    rx[0] = (AR.NOTCH, 0.25, 0.0)
    r = AR.AdaptRef(rx, 16, 2)
    plain = AR.AdaptRef(rx, 16, 2)
    r.process(x[:, :250])
    plain.process(x[:, :250])
    before = r.weights.copy()
    r.set_rx(1, rx[1][0], rx[1][1], rx[1][2], AR.RESTART)
    r.process(x[:, 250:250])                      # a batch of 0 honours nothing
    assert same(r.weights, before)
    for bad in ((K, 1, 0.5, 0.0, 0), (-1, 1, 0.5, 0.0, 0), (0, 3, 0.5, 0.0, 0), (0, 1, 0.0, 0.0, 0), (0, 1, 2.0, 0.0, 0),
                (0, 1, 0.5, 1.0, 0), (0, 1, 0.5, -0.1, 0), (0, 1, np.nan, 0.0, 0), (0, 1, 0.5, np.inf, 0), (0, 1, 0.5, 0.0, 2)):
        with pytest.raises(ValueError):
            r.set_rx(*bad)
    got = r.process(x[:, 250:])
    want = plain.process(x[:, 250:])
    # receiver 1 is the run of a fresh object whose delay line holds the inputs so far
    fresh = AR.AdaptRef(rx[1:2], 16, 2)
    fresh.hist = x[1:2, 250 - 17:250].copy()
    assert same(got[1], fresh.process(x[1:2, 250:])[0]) and not same(got[1], want[1])
    for j in (0, 2, 3, 4):
        assert same(got[j], want[j]) and same(r.weights[j], plain.weights[j])


def test_argument_errors_without_a_device(pkg):
    L = pkg.ddc_lib()

    def create(rx=((0, 0.5, 0.0, 0), (1, 1.5, 0.5, 0), (2, 0.01, 2.0 ** -10, 1)), nrx=None, params=(64, 1, 1e-6),
               null_rx=False, null_params=False):
        arr = (pkg.AdaptRx * max(len(rx), 1))(*[pkg.AdaptRx(*r) for r in rx])
        par = pkg.AdaptParams(*params)
        s = C.c_void_p()
        rc = L.pddc_adapt_create(C.byref(s), 0, len(rx) if nrx is None else nrx, None if null_params else C.byref(par),
                                 None if null_rx else arr)
        if rc == 0:
            L.pddc_adapt_destroy(s)
        return rc

    nan, inf = float("nan"), float("inf")
    bad = [dict(nrx=0), dict(nrx=-1), dict(rx=[(1, 0.5, 0.0, 0)] * 1025), dict(null_rx=True), dict(null_params=True),
           dict(params=(0, 1, 1e-6)), dict(params=(8, 1, 1e-6)), dict(params=(48, 1, 1e-6)), dict(params=(256, 1, 1e-6)),
           dict(params=(-64, 1, 1e-6)), dict(params=(64, 0, 1e-6)), dict(params=(64, 257, 1e-6)), dict(params=(64, -1, 1e-6)),
           dict(params=(64, 1, 0.0)), dict(params=(64, 1, -1e-6)), dict(params=(64, 1, nan)), dict(params=(64, 1, inf)),
           dict(rx=[(3, 0.5, 0.0, 0)]), dict(rx=[(0xFFFFFFFF, 0.5, 0.0, 0)]),
           dict(rx=[(1, 0.0, 0.0, 0)]), dict(rx=[(1, 2.0, 0.0, 0)]), dict(rx=[(1, -0.5, 0.0, 0)]), dict(rx=[(1, nan, 0.0, 0)]),
           dict(rx=[(1, inf, 0.0, 0)]),
           dict(rx=[(1, 0.5, 1.0, 0)]), dict(rx=[(1, 0.5, -2.0 ** -20, 0)]), dict(rx=[(1, 0.5, nan, 0)]), dict(rx=[(1, 0.5, inf, 0)]),
           dict(rx=[(1, 0.5, 0.0, 2)]), dict(rx=[(1, 0.5, 0.0, 0), (1, 0.5, 0.0, 0x80000000)])]
    for kw in bad:
        assert create(**kw) == pkg.PDDC_EINVAL, kw
    arr = (pkg.AdaptRx * 1)(pkg.AdaptRx(1, 0.5, 0.0, 0))
    par = pkg.AdaptParams(64, 1, 1e-6)
    assert L.pddc_adapt_create(None, 0, 1, C.byref(par), arr) == pkg.PDDC_EINVAL
    import torch
    if not torch.cuda.is_available():
        assert create() == pkg.PDDC_ENODEV
        for T in AR.TAPS:
            assert create(rx=[(2, 1.9999999, 0.99999994, 1)] * 1024, params=(T, 256, 3.0e38)) == pkg.PDDC_ENODEV
        assert create(params=(16, 1, 1e-45)) == pkg.PDDC_ENODEV
        with pytest.raises(pkg.PddcError) as e:
            pkg.Adapt([(pkg.PDDC_ADAPT_NOTCH, 0.25, 0.0)], 64, 1)
        assert e.value.code == pkg.PDDC_ENODEV
    for kw in (dict(rx=[(3, 0.25, 0.0)], taps=64, delay=1), dict(rx=[(1, 0.25, 0.0)], taps=65, delay=1),
               dict(rx=[(1, 0.25, 0.0)], taps=64, delay=1 << 40), dict(rx=[(1, 0.25, 0.0)], taps=64, delay=1, eps=0.0),
               dict(rx=[(-1, 0.25, 0.0)], taps=64, delay=1)):
        with pytest.raises(pkg.PddcError) as e:
            pkg.Adapt(**kw)
        assert e.value.code == pkg.PDDC_EINVAL, kw
    w = (C.c_float * 64)()
    assert L.pddc_adapt_process(None, None, 8, 8, None, 8, None) == pkg.PDDC_EINVAL
    assert L.pddc_adapt_set_rx(None, 0, 1, 0.5, 0.0, 0) == pkg.PDDC_EINVAL
    assert L.pddc_adapt_read_weights(None, w, None) == pkg.PDDC_EINVAL
    assert L.pddc_adapt_reset(None) == pkg.PDDC_EINVAL
    assert L.pddc_adapt_destroy(None) == 0
    assert pkg.adapt_tile_outputs() >= 1 and pkg.adapt_tile_outputs() == L.pddc_adapt_tile_outputs()
    assert (pkg.PDDC_ADAPT_OFF, pkg.PDDC_ADAPT_NR, pkg.PDDC_ADAPT_NOTCH, pkg.PDDC_ADAPT_RESTART) == (AR.OFF, AR.NR, AR.NOTCH, AR.RESTART)
    assert C.sizeof(pkg.AdaptParams) == 12 and C.sizeof(pkg.AdaptRx) == 16


def test_gpu_inputs_meet_their_preconditions():
    """Preconditions of tests/test_gpu_adapt.py, on the reference alone.  Every 16 consecutive receivers -- the smallest
    lane group's share of a wave and more -- hold every mode, and every 4 consecutive ones hold at least two.  Over the
    first 37 rows of the series (the K = 37 cases; a row's bits do not depend on K) at every (T, D) of the GPU tests:
    the outputs are finite, the tiny row's products pass through the denormals and the tinier row's weights are denormal at the end,
    the zero row stays +0, the silent row's outputs return to 0, and every mode's rows differ from their input or not as
    the mode says."""
    rx = AR.interleaved_rx(1024)
    modes = [r[0] for r in rx]
    for j in range(0, 1024 - 16):
        assert set(modes[j:j + 16]) == set(AR.MODES) and len(set(modes[j:j + 4])) >= 2
    assert len({r[1] for r in rx}) == len(AR.MUS) and len({r[2] for r in rx}) == len(AR.LEAKS)
    assert [rx[j][0] for j in (AR.ZERO_ROW, AR.SILENT_ROW, AR.TINY_ROW, AR.TINIER_ROW)] == [AR.NOTCH, AR.NR, AR.NR, AR.NOTCH]
    x = AR.gpu_series()[:37]
    assert not x[AR.ZERO_ROW].any() and x[AR.SILENT_ROW, :AR.SILENT_FROM].any() and not x[AR.SILENT_ROW, AR.SILENT_FROM:].any()
    for j in (AR.TINY_ROW, AR.TINIER_ROW):
        assert np.all(np.abs(x[j][x[j] != 0]) >= AR.TINY)
    for T, D in AR.GPU_SETS:
        out, w, r = AR.adapt_ref(x, rx[:37], T, D, count=True)
        print(f"T {T} D {D}: max |out| {np.abs(out).max():.3g}, denormal products in the tiny row {r.denormals[AR.TINY_ROW]}")
        assert np.isfinite(out).all() and np.isfinite(w).all()
        assert r.denormals[AR.TINY_ROW] >= 1000
        tw = np.abs(w[AR.TINIER_ROW])
        assert np.any((tw > 0) & (tw < AR.TINY))
        assert not AR.bits(out[AR.ZERO_ROW]).any() and not AR.bits(w[AR.ZERO_ROW]).any()
        assert not out[AR.SILENT_ROW, AR.SILENT_FROM + D + T:].any() and w[AR.SILENT_ROW].any()
        for j in range(37):
            if rx[j][0] == AR.OFF:
                assert same(out[j], x[j]) and not w[j].any()
            elif j != AR.ZERO_ROW:
                # (the tinier row's prediction underflows to 0: its NOTCH output is its input, its weights are not 0)
                assert w[j].any() and (j == AR.TINIER_ROW or not same(out[j], x[j]))
