"""The spectral noise reduction without a GPU: the reference (tests/denoise_ref.py) against itself and against closed
forms, the tolerance of the GPU comparison measured on the GPU tests' inputs, and the C ABI's argument checks."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as R


def noise(K, n, seed, sigma=1.0):
    return (sigma * np.random.default_rng(seed).standard_normal((K, n))).astype(np.float32)


@pytest.mark.parametrize("nfft,hop,K", [(256, 128, 37), (512, 128, 9), (1024, 512, 9), (1024, 256, 9)])
def test_streaming_equals_one_shot_under_the_gpu_cuts(pkg, nfft, hop, K):
    w, x, rx = R.window(nfft, hop), R.rows(K), R.receivers(K)
    ref, N = R.oneshot(x, nfft, hop, w, rx)
    for run in R.cut_runs(nfft, hop, pkg.denoise_tile_frames()):
        s, at, out = R.Stream(nfft, hop, w, rx), 0, []
        for b in run:
            out.append(s.process(x[:, at:at + b]))
            at += b
        assert at == R.N_GPU and np.array_equal(np.concatenate(out, axis=1), ref) and np.array_equal(s.noise(), N), run
    ev = R.changes(K)
    ref, N = R.oneshot(x, nfft, hop, w, rx, ev)
    assert np.abs(ref - R.oneshot(x, nfft, hop, w, rx)[0]).max() > 1e-3         # the changes change something
    for cuts in (R.CHANGE_POSITIONS, sorted(set(R.CHANGE_POSITIONS) | {1, 699, 1101, 1500 + hop, 2999})):
        out, Ns = R.stream_with_changes(K, x, nfft, hop, w, rx, ev, cuts)
        assert np.array_equal(out, ref) and np.array_equal(Ns, N)


@pytest.mark.parametrize("nfft,hop", [(256, 128), (256, 64), (512, 256), (1024, 256)])
def test_off_with_the_package_window_is_the_delayed_input(pkg, nfft, hop):
    """out[m + nfft] = x[m] in double, <= 1e-12.  Measured with this reference: 9e-16 .. 1.8e-15 on unit noise (a prototype
    measured 2e-16)."""
    w = pkg.denoise_window(nfft, hop)
    assert w.dtype == np.float64 and np.array_equal(w.astype(np.float32), R.window(nfft, hop))
    assert np.abs(sum(w[r * hop:(r + 1) * hop] ** 2 for r in range(nfft // hop)) - 1).max() < 1e-15
    assert pkg.denoise_delay(nfft) == nfft
    x = noise(3, 4 * nfft + 77, 3)
    out, _ = R.oneshot(x, nfft, hop, w, [(R.OFF, 2.0, 0.1, 0.98)] * 3)
    err = np.abs(out[:, nfft:] - x[:, :-nfft]).max()
    print("OFF identity", err)
    assert np.all(out[:, :nfft] == 0) and err <= 1e-12
    # the device holds the window as float32: its squares sum to 1 within that rounding, and so does the identity
    out, _ = R.oneshot(x, nfft, hop, R.window(nfft, hop), [(R.OFF, 2.0, 0.1, 0.98)] * 3)
    assert np.abs(out[:, nfft:] - x[:, :-nfft]).max() < 5e-7 * np.abs(x).max()


def test_the_zero_row_comes_out_exactly_zero():
    for nfft, hop, _ in R.SIZES:
        x = R.rows(8)
        out, N = R.oneshot(x, nfft, hop, R.window(nfft, hop), R.receivers(8))
        assert np.all(out[R.ZERO_ROW] == 0) and np.all(N[R.ZERO_ROW] == 0) and np.abs(out).max() > 0
        m = R.Stream(nfft, hop, R.window(nfft, hop), R.receivers(8), np.float32)
        assert np.all(m.process(x)[R.ZERO_ROW] == 0)


@pytest.mark.parametrize("nfft,hop", [(256, 128), (1024, 256)])
def test_white_noise_goes_down_to_the_gain_floor(nfft, hop):
    """Stationary white noise at the defaults: the second half's attenuation is within 1.5 dB of 20 log10 gmin = -20 dB.
    Measured with this reference over frames 400 .. 800: -19.9 dB at 256 / 128, -19.5 dB at 1024 / 256 (a prototype
    measured -19.6 .. -19.7); the estimate settles slowly, at 2 % a frame, so frames 100 .. 200 still read -17 .. -18 dB."""
    n = 800 * hop                                   # the estimate of a bin that began low rises 2 % a frame
    x = noise(2, n, 11)
    out, _ = R.oneshot(x, nfft, hop, R.window(nfft, hop), [R.RX_DEFAULT] * 2)
    half = slice(n // 2 + nfft, n)
    db = 10 * np.log10((out[:, half] ** 2).mean(axis=1) / (x[:, n // 2:n - nfft].astype(np.float64) ** 2).mean(axis=1))
    print("attenuation dB", db)
    assert np.all(np.abs(db - 20 * np.log10(0.1)) <= 1.5), db


def test_a_keyed_tone_keeps_its_amplitude():
    """A tone keyed 2560 samples on / 2560 off, 20 dB over the noise, at 256 / 128: >= 0.95 of its amplitude in the
    interior of the on-periods.  Measured with this reference: 0.990 .. 1.006 (a prototype measured 0.99)."""
    nfft, hop, period, n = 256, 128, 2560, 8 * 2560
    m = np.arange(n)
    tone = np.sin(2 * np.pi * 0.1037 * m)
    on = (m // period) % 2 == 1                     # it begins in a gap: a row that begins with the tone takes it for noise
    x = (on * tone + noise(1, n, 5, np.sqrt(0.5 / 100.0))[0]).astype(np.float32)[None, :]
    out, _ = R.oneshot(x, nfft, hop, R.window(nfft, hop), [R.RX_DEFAULT])
    kept = []
    for p in range(1, n // period, 2):
        lo, hi = p * period + 512, (p + 1) * period - 512
        seg = slice(lo + nfft, hi + nfft)           # the output is nfft late
        kept.append(2 * np.mean(out[0, seg] * tone[lo:hi]))
    print("kept amplitude", kept)
    assert min(kept) >= 0.95, kept
    off_rms = np.sqrt(np.mean(out[0, 4 * period + 512 + nfft:5 * period - 512 + nfft] ** 2))
    assert off_rms < 0.3 * np.sqrt(0.5 / 100.0)     # and the gaps between are quieter than they came in


def test_hold_freezes_the_noise_estimate():
    nfft, hop = 256, 128
    x = np.concatenate([noise(2, 2000, 7), noise(2, 2000, 8, 10.0)], axis=1)
    s = R.Stream(nfft, hop, R.window(nfft, hop), [R.RX_DEFAULT] * 2)
    s.process(x[:, :2000])
    before = s.noise()
    s.set_rx(0, *R.RX_DEFAULT, R.HOLD)
    out = s.process(x[:, 2000:3000])
    mid = s.noise()
    assert np.array_equal(mid[0], before[0]) and not np.array_equal(mid[1], before[1]) and mid[1].mean() > before[1].mean() and np.abs(out[0]).max() > 0
    s.set_rx(0, *R.RX_DEFAULT, 0)                   # lasting until a set_rx without it
    s.process(x[:, 3000:])
    assert np.all(s.noise()[0] != before[0])


def test_restart_equals_a_fresh_object_fed_from_that_frame_on():
    for nfft, hop in ((256, 128), (512, 128)):
        x = noise(2, 6000, 9)
        x[:, :2000] *= 30
        w = R.window(nfft, hop)
        at = 2000 + 17                              # the call falls inside a frame
        s = R.Stream(nfft, hop, w, [R.RX_DEFAULT] * 2)
        head = s.process(x[:, :at])
        s.set_rx(1, *R.RX_DEFAULT, R.RESTART)
        out = np.concatenate([head, s.process(x[:, at:])], axis=1)
        q = at // hop                               # the first frame whose last sample arrives after the call
        fresh = R.Stream(nfft, hop, w, [R.RX_DEFAULT])
        fresh.inputs = x[1:2, (q + 1) * hop - nfft:q * hop].astype(np.float64)
        want = fresh.process(x[1:2, q * hop:])
        # once the overlap has drained: out index q hop + nfft on
        assert np.array_equal(out[1, q * hop + nfft:], want[0, nfft:])
        assert np.array_equal(s.noise()[1], fresh.noise()[0])
        plain, _ = R.oneshot(x, nfft, hop, w, [R.RX_DEFAULT] * 2)
        assert np.array_equal(out[0], plain[0]) and np.abs(out[1] - plain[1]).max() > 1e-3


def test_a_bad_sample_in_the_reference_does_what_the_header_says():
    """NaN / inf / 1e25 at p: N is NaN for good once good frames follow, the output is finite again from the first
    good frame's own hop on and is the floor gain's; nfft good samples and RESTART recover."""
    nfft, hop = 256, 64
    w = R.window(nfft, hop)
    for bad in (np.nan, np.inf, 1e25):
        x = noise(1, 4000, 13)
        p = 1000
        x[0, p] = bad
        s = R.Stream(nfft, hop, w, [R.RX_DEFAULT], np.float32)
        out = s.process(x[:, :2000])
        assert np.all(np.isnan(s.noise()))
        lastbad = p // hop + nfft // hop - 1        # the last frame that holds p
        good = slice((lastbad + 2) * hop + nfft - hop, 2000)      # y reached by good frames alone
        assert np.all(np.isfinite(out[0, good])) and not np.all(np.isfinite(out[0, p:p + 2 * nfft]) & (np.abs(out[0, p:p + 2 * nfft]) < 1e6))
        clean = x.copy()
        clean[0, p] = 0
        off = R.Stream(nfft, hop, w, [(R.OFF, 2.0, 0.1, 0.98)], np.float32).process(clean[:, :2000])
        assert np.allclose(out[0, good], np.float32(0.1) * off[0, good], rtol=0, atol=1e-5)
        s.set_rx(0, *R.RX_DEFAULT, R.RESTART)       # more than nfft good samples since p
        tail = s.process(x[:, 2000:])
        c = R.Stream(nfft, hop, w, [R.RX_DEFAULT], np.float32)
        c.process(clean[:, :2000])
        c.set_rx(0, *R.RX_DEFAULT, R.RESTART)
        want = c.process(clean[:, 2000:])
        q = 2000 // hop
        assert np.array_equal(tail[0, q * hop + nfft - 2000:], want[0, q * hop + nfft - 2000:])
        assert np.array_equal(s.noise(), c.noise()) and np.all(np.isfinite(s.noise()))


def test_model_worst(pkg):
    """MODEL_WORST, re-measured: the float32 model against the double reference on the very inputs of the GPU tests,
    outputs and N, plain and with the set_rx calls."""
    worst = 0.0
    for nfft, hop, K in R.SIZES:
        w, x, rx = R.window(nfft, hop), R.rows(K), R.receivers(K)
        ref, N = R.oneshot(x, nfft, hop, w, rx)
        assert np.all(ref[R.ZERO_ROW] == 0) and np.all(x[R.SILENT_ROW, 1000:] == 0) and np.abs(ref[R.SILENT_ROW]).max() > 0
        m = R.Stream(nfft, hop, w, rx, np.float32)
        got = m.process(x)
        assert got.dtype == np.float32 and m.noise().dtype == np.float32
        here = [R.metric(got, ref), R.metric(m.noise(), N)]
        ev = R.changes(K)
        ref, N = R.oneshot(x, nfft, hop, w, rx, ev)
        got, Nm = R.stream_with_changes(K, x, nfft, hop, w, rx, ev, R.CHANGE_POSITIONS, np.float32)
        here += [R.metric(got, ref), R.metric(Nm, N)]
        print(nfft, hop, K, here)
        worst = max(worst, *here)
    print("MODEL_WORST measured", worst)
    assert worst <= R.MODEL_WORST <= 1e-5
    assert R.MODEL_WORST <= 4 * worst               # "that value, rounded up", not a stale wide one
    assert R.TOL_DENOISE == 8 * R.MODEL_WORST


def test_argument_errors_without_a_device(pkg):
    L = pkg.ddc_lib()
    good_rx = ((0, 2.0, 0.1, 0.98, 0), (1, 1.0, 0.0, 0.0, 2), (1, 3.0e38, 1.0, 0.99999994, 3))

    def create(rx=good_rx, nrx=None, params=(256, 128, 0.3, 0.02, 0.3, 1e-4, 1e-20), window=None, null_rx=False,
               null_params=False, null_window=False):
        arr = (pkg.DenoiseRx * max(len(rx), 1))(*[pkg.DenoiseRx(*r) for r in rx])
        par = pkg.DenoiseParams(*params)
        w = np.ones(max(params[0], 1) if params[0] <= 4096 else 1, np.float32) if window is None else np.asarray(window, np.float32)
        s = C.c_void_p()
        rc = L.pddc_denoise_create(C.byref(s), 0, len(rx) if nrx is None else nrx, None if null_params else C.byref(par),
                                   None if null_window else w.ctypes.data, None if null_rx else arr)
        if rc == 0:
            L.pddc_denoise_destroy(s)
        return rc

    def P(**kw):
        d = dict(nfft=256, hop=128, smooth=0.3, up=0.02, down=0.3, nmin=1e-4, eps=1e-20)
        d.update(kw)
        return dict(params=tuple(d[k] for k in ("nfft", "hop", "smooth", "up", "down", "nmin", "eps")))

    nan, inf = float("nan"), float("inf")
    wbad = np.ones(256, np.float32)
    wbad[255] = nan
    winf = np.ones(256, np.float32)
    winf[0] = inf
    bad = [dict(nrx=0), dict(nrx=-1), dict(rx=[(1, 2.0, 0.1, 0.98, 0)] * 1025), dict(null_rx=True), dict(null_params=True),
           dict(null_window=True), dict(window=wbad), dict(window=winf),
           P(nfft=0), P(nfft=128, hop=64), P(nfft=2048, hop=1024), P(nfft=384, hop=192), P(nfft=-256), P(hop=256), P(hop=32),
           P(hop=0), P(hop=-128), P(hop=127), P(nfft=512, hop=64), P(nfft=1024, hop=1024),
           P(smooth=0.0), P(smooth=1.0000001), P(smooth=nan), P(smooth=-0.3), P(up=0.0), P(up=1.5), P(up=nan), P(down=0.0),
           P(down=inf), P(down=nan), P(nmin=-1e-9), P(nmin=1.0000001), P(nmin=nan), P(eps=0.0), P(eps=-1e-20), P(eps=nan),
           P(eps=inf),
           dict(rx=[(2, 2.0, 0.1, 0.98, 0)]), dict(rx=[(0xFFFFFFFF, 2.0, 0.1, 0.98, 0)]),
           dict(rx=[(1, 0.0, 0.1, 0.98, 0)]), dict(rx=[(1, -2.0, 0.1, 0.98, 0)]), dict(rx=[(1, nan, 0.1, 0.98, 0)]),
           dict(rx=[(1, inf, 0.1, 0.98, 0)]),
           dict(rx=[(1, 2.0, -1e-9, 0.98, 0)]), dict(rx=[(1, 2.0, 1.0000001, 0.98, 0)]), dict(rx=[(1, 2.0, nan, 0.98, 0)]),
           dict(rx=[(1, 2.0, 0.1, 1.0, 0)]), dict(rx=[(1, 2.0, 0.1, -1e-9, 0)]), dict(rx=[(1, 2.0, 0.1, nan, 0)]),
           dict(rx=[(1, 2.0, 0.1, inf, 0)]),
           dict(rx=[(1, 2.0, 0.1, 0.98, 4)]), dict(rx=[(1, 2.0, 0.1, 0.98, 0), (1, 2.0, 0.1, 0.98, 0x80000000)])]
    for kw in bad:
        assert create(**kw) == pkg.PDDC_EINVAL, kw
    arr = (pkg.DenoiseRx * 1)(pkg.DenoiseRx(1, 2.0, 0.1, 0.98, 0))
    par = pkg.DenoiseParams(256, 128, 0.3, 0.02, 0.3, 1e-4, 1e-20)
    assert L.pddc_denoise_create(None, 0, 1, C.byref(par), wbad.ctypes.data, arr) == pkg.PDDC_EINVAL
    import torch
    if not torch.cuda.is_available():
        assert create() == pkg.PDDC_ENODEV
        for nfft, hop, _ in R.SIZES:
            assert create(rx=[good_rx[2]] * 1024, **P(nfft=nfft, hop=hop, smooth=1.0, up=1.0, down=1.0, nmin=1.0, eps=3e38)) == pkg.PDDC_ENODEV
        assert create(**P(nmin=0.0, eps=1e-45)) == pkg.PDDC_ENODEV
        with pytest.raises(pkg.PddcError) as e:
            pkg.Denoise(3)
        assert e.value.code == pkg.PDDC_ENODEV
    for kw in (dict(rx=[(2, 2.0, 0.1, 0.98)]), dict(rx=2, nfft=300, hop=150), dict(rx=2, nfft=256, hop=1 << 40),
               dict(rx=2, eps=0.0), dict(rx=[(-1, 2.0, 0.1, 0.98)]), dict(rx=[]), dict(rx=2, window=[nan] * 256)):
        with pytest.raises(pkg.PddcError) as e:
            pkg.Denoise(**kw)
        assert e.value.code == pkg.PDDC_EINVAL, kw
    with pytest.raises(pkg.PddcError):
        pkg.Denoise(2, window=np.ones(255, np.float32))
    nn = (C.c_float * 129)()
    assert L.pddc_denoise_process(None, None, 8, 8, None, 8, None) == pkg.PDDC_EINVAL
    assert L.pddc_denoise_set_rx(None, 0, 1, 2.0, 0.1, 0.98, 0) == pkg.PDDC_EINVAL
    assert L.pddc_denoise_read_noise(None, nn, None) == pkg.PDDC_EINVAL
    assert L.pddc_denoise_reset(None) == pkg.PDDC_EINVAL
    assert L.pddc_denoise_destroy(None) == 0
    assert [pkg.denoise_delay(n) for n in (256, 512, 1024, 128, 2048, 0, -256, 300)] == [256, 512, 1024, 0, 0, 0, 0, 0]
    assert pkg.denoise_tile_frames() >= 1 and pkg.denoise_tile_frames() == L.pddc_denoise_tile_frames()
    assert (pkg.PDDC_DENOISE_OFF, pkg.PDDC_DENOISE_NR, pkg.PDDC_DENOISE_RESTART, pkg.PDDC_DENOISE_HOLD) == (R.OFF, R.NR, R.RESTART, R.HOLD)
    assert C.sizeof(pkg.DenoiseParams) == 28 and C.sizeof(pkg.DenoiseRx) == 20
