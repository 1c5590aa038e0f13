"""The demodulator without a GPU: its reference (tests/demod_ref.py) on known signals, against the cut and against the
set_rx rules; the float32 models that set the GPU tolerances; the argument checks of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import channelizer_ref as CR
import demod_ref as DR
import spectrum_ref as R
import tuner_ref as TR

FS_OUT = DR.OUT_RATE                              # 39 062.5 outputs per second
P = DR.PARAMS


def tone_amplitude(a, f_hz, rate):
    """the amplitude of the component at f_hz of a real series, by projection over whole cycles"""
    n = int(np.floor(a.size * f_hz / rate) * rate / f_hz)
    m = np.arange(n)
    return 2.0 * abs(np.sum(a[:n] * np.exp(-2j * np.pi * f_hz * m / rate))) / n


def test_reference_demodulates_known_signals():
    """AM: carrier 0.8 with a 1 kHz tone at depth 0.5 -> behind the DC block the tone at amplitude depth x carrier (the
    block's gain at 1 kHz, |1 - w| / |1 - rho w|, w = e^{-2 pi i f / fs_out}, taken into account), without it the mean
    is the carrier.  FM: 1 kHz at 3 kHz deviation -> peak = deviation / (fs_out / 2), within the chord's
    sin(x)/x at 1 kHz.  USB: a tone 700 Hz above the carrier with the words of ssb_words -> 700 Hz at the tone's amplitude."""
    n = 1 << 14
    t = np.arange(n) / FS_OUT
    A, depth, f = 0.8, DR.AM_DEPTH, DR.TONE_HZ
    z = (A * (1 + depth * np.cos(2 * np.pi * f * t)) * np.exp(1j * (0.3 + 2 * np.pi * 11.0 * t)))[None, :]
    plain = DR.demod_ref(z, [(DR.AM, 0, 0)], **P)[0]
    assert abs(plain.mean() - A) < 1e-3 and abs(tone_amplitude(plain, f, FS_OUT) - depth * A) < 1e-3
    blocked = DR.demod_ref(z, [(DR.AM, 0, DR.DC)], **P)[0][4000:]
    w = np.exp(-2j * np.pi * f / FS_OUT)
    gain = abs(1 - w) / abs(1 - np.float32(P["rho"]) * w)
    assert abs(blocked.mean()) < 1e-3 and abs(tone_amplitude(blocked, f, FS_OUT) - depth * A * gain) < 1e-3
    assert 0.99 < gain < 1.01
    dev = DR.FM_DEV_HZ
    z = (0.7 * np.exp(1j * (dev / f * np.sin(2 * np.pi * f * t))))[None, :]
    fm = DR.demod_ref(z, [(DR.FM, 0, 0)], **P)[0]
    want = dev / (FS_OUT / 2)
    chord = np.sinc(f / FS_OUT)                   # the phase difference over one output is the deviation's mean over it
    print(f"FM peak {np.max(np.abs(fm)):.5f}, deviation / (fs_out / 2) = {want:.5f}, chord factor {chord:.5f}")
    assert fm[0] == 0 and abs(np.max(np.abs(fm[1:])) - want * chord) < 2e-4 * want
    assert abs(tone_amplitude(fm, f, FS_OUT) - want * chord) < 1e-3 * want
    # USB: the series the tuner would give, tuned to the middle of the sideband
    lo, hi = DR.SSB_BAND
    _, bfo = DR.ssb_words(DR.FS, FS_OUT, DR.CARRIER_HZ, lo, hi, True)
    z = (0.6 * np.exp(2j * np.pi * (DR.SSB_TONE_HZ - (lo + hi) / 2) * t))[None, :]
    usb = DR.demod_ref(z, [(DR.SSB, bfo, 0)], **P)[0]
    fq = (-bfo % (1 << 32)) / 2.0 ** 32 * FS_OUT           # the word's own frequency, (lo + hi) / 2 rounded
    assert abs(fq - (lo + hi) / 2) < FS_OUT / 2.0 ** 32
    assert abs(tone_amplitude(usb, DR.SSB_TONE_HZ, FS_OUT) - 0.6) < 1e-3
    peak = np.argmax(np.abs(np.fft.rfft(usb * np.hanning(n)))) * FS_OUT / n
    assert abs(peak - DR.SSB_TONE_HZ) <= FS_OUT / n


def test_the_other_sideband_is_down_by_the_lowpass(pkg):
    """A tone 700 Hz above a carrier at the row rate 4 x 39 062.5, through the tuner's stage in double (mix to the middle
    of the sideband, tuner_lowpass with the sideband's half width as cutoff, T = 512, R = 4) and demod_ref: with the USB
    words it comes out at the tone's amplitude times the low-pass's response at its offset (-800 Hz); with the LSB words
    it sits 2200 Hz off the middle of that sideband, in the stop band, and comes out down by the response there.  Both
    against the low-pass's own frequency response, and the LSB one below its stop-band figure (the largest response from
    the stop-band edge on, cutoff plus half of Kaiser's transition width for beta = 8)."""
    T, Rd, A = 512, 4, 0.6
    rate = FS_OUT * Rd
    lo, hi = DR.SSB_BAND
    h = pkg.tuner_lowpass(T, Rd, cutoff=(hi - lo) / 2 / rate).astype(np.float64)
    resp = lambda f: abs(np.sum(h * np.exp(-2j * np.pi * f / rate * np.arange(T))))
    att = 8.0 / 0.1102 + 8.7                                # Kaiser: beta = 0.1102 (A - 8.7)
    width = (att - 7.95) / (14.36 * (T - 1)) * rate         # transition width in Hz
    edge = (hi - lo) / 2 + width / 2
    stop = max(resp(f) for f in np.linspace(edge, rate / 2, 4000))
    s = np.arange(1 << 15)
    tone = DR.SSB_TONE_HZ
    got = {}
    for upper in (True, False):
        sign = 1.0 if upper else -1.0
        mid = sign * (lo + hi) / 2                            # where the tuner is tuned, relative to the carrier
        _, bfo = DR.ssb_words(DR.FS, FS_OUT, DR.CARRIER_HZ, lo, hi, upper)
        x = A * np.exp(2j * np.pi * (tone - mid) / rate * s)
        z = TR.fir_decim(x[:, None], h, Rd).T
        a = DR.demod_ref(z, [(DR.SSB, bfo, 0)], **P)[0]
        got[upper] = tone_amplitude(a, tone, FS_OUT)
        want = A * resp(tone - mid)
        print(f"{'USB' if upper else 'LSB'} words: tone at {got[upper]:.3e}, low-pass at {tone - mid:+.0f} Hz gives {want:.3e}")
        assert abs(got[upper] - want) <= 0.02 * want + 1e-9
    down = 20 * np.log10(got[True] / got[False])
    print(f"the other sideband is {down:.1f} dB down; the low-pass's stop band ({edge:.0f} Hz on) is {-20 * np.log10(stop):.1f} dB down")
    assert tone + (lo + hi) / 2 > edge and got[False] <= A * stop and down >= -20 * np.log10(stop / resp(-800.0))


def random_series(K, n, seed=3):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n))).astype(np.complex64)


def test_cut_invariance():
    """demod_ref (and the float32 model) give the same values when the series is cut at 0, 1, 2 and ragged lengths"""
    K, n = 24, 700
    rx = DR.interleaved_rx(K)
    z = random_series(K, n)
    cuts = [0, 1, 2, 0, 255, 256, 1, 100, 0]
    cuts.append(n - sum(cuts))
    for f32 in (False, True):
        one = DR.run_cuts(DR.DemodRef(rx, f32=f32, **P), z)
        cut = DR.run_cuts(DR.DemodRef(rx, f32=f32, **P), z, cuts)
        assert one.shape == (K, n) and np.array_equal(one, cut)
    assert np.all(one[[j for j in range(K) if rx[j][0] == DR.FM], 0] == 0)


def test_set_rx_rules():
    """A BFO change is phase-continuous: a tone at the old word's frequency comes out, after the change to another
    word, as the cosine the accumulator gives (no phase step at m0).  A mode or flag change resets that receiver's
    carried values (its outputs from m0 on equal a fresh object's on the rest of the series, SSB apart: m goes on, psi
    = 0) and leaves the other receivers alone."""
    n, m0 = 600, 217
    b0, b1 = 0x0A000000, 0x0B800000
    m = np.arange(n)
    z = np.exp(-2j * np.pi * (b0 * m % (1 << 32)) / 2.0 ** 32)[None, :] * 0.5          # z e^{-i theta} has frequency -2 b0
    r = DR.DemodRef([(DR.SSB, b0, 0)], **P)
    a0 = r.process(z[:, :m0])
    r.set_rx(0, DR.SSB, b1, 0)
    a1 = r.process(z[:, m0:])
    th = np.where(m < m0, b0 * m, b1 * m + (b0 - b1) * m0) % (1 << 32)
    want = (z[0] * np.exp(-2j * np.pi * th / 2.0 ** 32)).real
    assert int(r.psi[0]) == ((b0 - b1) * m0) % (1 << 32)
    assert np.max(np.abs(np.concatenate([a0, a1], axis=1)[0] - want)) < 1e-14
    # no step: at m0 the phase is what the old word's accumulator had reached, and the new increment counts from there
    assert int(th[m0]) == (b0 * m0) % (1 << 32) and (int(th[m0 + 1]) - int(th[m0])) % (1 << 32) == b1
    K = 6
    rx = [(DR.AM, 0, DR.DC | DR.AGC), (DR.FM, 0, DR.DC), (DR.SSB, 12345678, DR.AGC), (DR.AM, 0, 0), (DR.FM, 0, DR.AGC),
          (DR.SSB, 999, DR.DC)]
    zz = random_series(K, n, seed=8)
    never = DR.demod_ref(zz, rx, **P)
    r = DR.DemodRef(rx, **P)
    a0 = r.process(zz[:, :m0])
    r.set_rx(1, DR.FM, 0, DR.DC | DR.AGC)                   # flags
    r.set_rx(3, DR.FM, 0, 0)                                # mode
    r.set_rx(5, DR.AM, 0, DR.DC)                            # mode
    got = np.concatenate([a0, r.process(zz[:, m0:])], axis=1)
    for j in (0, 2, 4):
        assert np.array_equal(got[j], never[j])
    assert np.array_equal(got[:, :m0], never[:, :m0])
    fresh = DR.demod_ref(zz[[1, 3, 5], m0:], [(DR.FM, 0, DR.DC | DR.AGC), (DR.FM, 0, 0), (DR.AM, 0, DR.DC)], **P)
    assert np.array_equal(got[[1, 3, 5], m0:], fresh) and np.all(fresh[:2, 0] == 0)
    r.set_rx(2, DR.AM, 0, DR.AGC)                           # to SSB and back later: psi starts at 0, m goes on
    r.set_rx(2, DR.SSB, 12345678, DR.AGC)
    assert int(r.psi[2]) == 0 and r.m == n and bool(r.fresh[2])


@pytest.fixture(scope="module")
def tuner_outputs(O):
    """the tuner reference's outputs on the 2^19-sample LCG stream (M = 1024, hop 512, T = 64, R = 4, the 1024 receivers
    of the tuner's parity test), rounded to complex64: [1024, 239]"""
    x = R.to_complex(O, O.lcg_bytes(6 << 19, 12345))
    M, hop, T, Rd = 1024, 512, 64, 4
    y = CR.channelizer_ref(x, M, hop, TR.kaiser_prototype_wide(M, 4))
    return TR.tuner_ref(y, M, hop, TR.receiver_set(M, 1024), TR.kaiser_lowpass(T, Rd), Rd).astype(np.complex64)


def test_float32_model_against_double(tuner_outputs):
    """The measurement that sets TOL_DEMOD: per mode and flag set, the float32 model against the double reference on the
    same complex64 inputs (all 1024 series for every mode and flag set).  The LCG stream is full-scale noise in every
    channel, so the AGC's envelope never sits near 0: min e / max e is asserted above 1e-3 from every series' third
    output on.  The first two are left out because the envelope is a running maximum that starts at 0: FM's first d is 0
    by definition (e = 0), and e's next value is the magnitude of a single random angle or real part -- 8.06e-5 (FM) and
    4.54e-4 (SSB) of the largest e for one of the 1024 series here.  From the third output on it is the largest of several.  TOL = 7 x the worst case per mode; a
    re-measurement may not exceed the written worst cases by more than 0.5 %."""
    z = tuner_outputs
    assert z.shape == (1024, 239)
    rng = np.random.default_rng(5)
    words = rng.integers(0, 1 << 32, z.shape[0], dtype=np.uint64)
    for mode in DR.MODES:
        worst = 0.0
        for flags in DR.FLAG_SETS:
            rx = [(mode, int(w), flags) for w in words]
            ref = DR.DemodRef(rx, **P)
            want = ref.process(z)
            e = DR.err(DR.demod_model_f32(z, rx, **P), want, wrap=(mode == DR.FM))
            first = 2
            cond = float(ref.e[:, first:].min() / ref.e.max())
            print(f"{DR.MODE_NAMES[mode]} flags {flags}: model err {e:.3e}, min e / max e {cond:.2e}, max |ref| {np.max(np.abs(want)):.3f}")
            assert cond > 1e-3, (mode, flags, cond)
            worst = max(worst, e)
        print(f"{DR.MODE_NAMES[mode]}: worst {worst:.3e} (written {DR.MODEL_WORST_DEMOD[mode]:.3e}, TOL {DR.TOL_DEMOD[mode]:.3e})")
        assert worst <= 1.005 * DR.MODEL_WORST_DEMOD[mode]
        assert DR.TOL_DEMOD[mode] == 7 * DR.MODEL_WORST_DEMOD[mode]


def chain_refs(O, mode):
    """chain_signal(mode) packed by the oracle -> (double chain's z [3, n], float32 model chain's z)"""
    c = DR.CHAIN
    packed = O.pack24_f32(DR.chain_signal(mode))
    x = R.to_complex(O, packed)
    w = TR.kaiser_prototype_wide(c["nchan"], c["proto_taps"])
    h = TR.kaiser_lowpass(c["ntaps"], c["decim"])
    words, rx = DR.chain_receivers(mode)
    kr = [TR.channel_of(c["nchan"], f) for f in words]
    cols, res = np.array([k for k, _ in kr]), [r for _, r in kr]
    y = CR.channelizer_ref(x, c["nchan"], c["hop"], w)
    z = TR.tuner_ref(y, c["nchan"], c["hop"], words, h, c["decim"])
    y32 = CR.channelizer_model_f32(x, c["nchan"], c["hop"], w)[:, cols]
    z32 = TR.tuner_model_f32(y32, res, [0] * len(words), c["hop"], h, c["decim"])
    return z, z32, rx


@pytest.mark.parametrize("mode", DR.MODES)
def test_float32_chain_model_against_double(O, mode):
    """The measurement that sets TOL_DEMOD_CHAIN: channelizer_model_f32 -> tuner_model_f32 -> demod_model_f32 against the
    three double references on chain_signal(mode), the very input of the GPU's end-to-end test.  The strong carrier keeps
    the detectors well conditioned: min |z| / max |z| >= 0.1 on the reference."""
    z, z32, rx = chain_refs(O, mode)
    cond = float(np.min(np.abs(z)) / np.max(np.abs(z)))
    want = DR.demod_ref(z, rx, **P)
    got = DR.demod_model_f32(z32, rx, **P)
    worst = 0.0
    for j, r in enumerate(rx):
        e = DR.err(got[j:j + 1], want[j:j + 1], wrap=(mode == DR.FM))
        print(f"{DR.MODE_NAMES[mode]} flags {r[2]}: chain model err {e:.3e}, max |ref| {np.max(np.abs(want[j])):.4f}")
        worst = max(worst, e)
    print(f"{DR.MODE_NAMES[mode]}: worst {worst:.3e} (written {DR.MODEL_WORST_DEMOD_CHAIN[mode]:.3e}), min |z| / max |z| {cond:.3f}, "
          f"|z| {np.max(np.abs(z)):.4f}, outputs {z.shape[1]}")
    assert cond >= 0.1
    assert worst <= 1.005 * DR.MODEL_WORST_DEMOD_CHAIN[mode]
    assert DR.TOL_DEMOD_CHAIN[mode] == 7 * DR.MODEL_WORST_DEMOD_CHAIN[mode]


def test_ssb_words_helper(pkg):
    for upper in (True, False):
        for lo, hi in ((300.0, 2700.0), (0.0, 3000.0), (650.0, 750.0)):
            assert pkg.demod_ssb_words(DR.FS, FS_OUT, DR.CARRIER_HZ, lo, hi, upper) == \
                DR.ssb_words(DR.FS, FS_OUT, DR.CARRIER_HZ, lo, hi, upper)
    word, bfo = pkg.demod_ssb_words(80e6, 39062.5, 7.1e6, 300, 2700, True)
    assert abs(word * 80e6 / 2.0 ** 32 - 7.1015e6) < 0.02 and abs((-bfo % (1 << 32)) * 39062.5 / 2.0 ** 32 - 1500) < 1e-4
    word, bfo = pkg.demod_ssb_words(80e6, 39062.5, 7.1e6, 300, 2700, False)
    assert abs(word * 80e6 / 2.0 ** 32 - 7.0985e6) < 0.02 and abs(bfo * 39062.5 / 2.0 ** 32 - 1500) < 1e-4
    assert (pkg.PDDC_DEMOD_AM, pkg.PDDC_DEMOD_FM, pkg.PDDC_DEMOD_SSB) == (DR.AM, DR.FM, DR.SSB)
    assert (pkg.PDDC_DEMOD_DCBLOCK, pkg.PDDC_DEMOD_AGC) == (DR.DC, DR.AGC)


def test_argument_errors_without_a_device(pkg):
    L = pkg.ddc_lib()
    assert pkg.demod_tile_outputs() >= 1

    def create(rx=((0, 0, 0), (1, 0, 3), (2, 5, 1)), nrx=None, params=(0.995, 0.999, 0.25, 100.0), null_rx=False,
               null_params=False):
        arr = (pkg.DemodRx * max(len(rx), 1))(*[pkg.DemodRx(*r) for r in rx])
        par = pkg.DemodParams(*params)
        d = C.c_void_p()
        rc = L.pddc_demod_create(C.byref(d), 0, len(rx) if nrx is None else nrx, None if null_rx else arr,
                                 None if null_params else C.byref(par))
        if rc == 0:
            L.pddc_demod_destroy(d)
        return rc

    nan, inf = float("nan"), float("inf")
    bad = [dict(nrx=0), dict(nrx=-1), dict(rx=[(0, 0, 0)] * 1025), dict(null_rx=True), dict(null_params=True),
           dict(rx=[(3, 0, 0)]), dict(rx=[(-1, 0, 0)]), dict(rx=[(0, 0, 4)]), dict(rx=[(0, 0, 0), (1, 0, 0x80000000)]),
           dict(params=(1.0, 0.999, 0.25, 100.0)), dict(params=(-0.1, 0.999, 0.25, 100.0)),
           dict(params=(0.995, 1.0, 0.25, 100.0)), dict(params=(0.995, -1e-3, 0.25, 100.0)),
           dict(params=(0.995, 0.999, 0.0, 100.0)), dict(params=(0.995, 0.999, 0.25, 0.0)),
           dict(params=(0.995, 0.999, -1.0, 100.0)), dict(params=(0.995, 0.999, 0.25, -5.0)),
           dict(params=(nan, 0.999, 0.25, 100.0)), dict(params=(0.995, nan, 0.25, 100.0)),
           dict(params=(0.995, 0.999, nan, 100.0)), dict(params=(0.995, 0.999, 0.25, inf))]
    for kw in bad:
        assert create(**kw) == pkg.PDDC_EINVAL, kw
    arr = (pkg.DemodRx * 1)(pkg.DemodRx(0, 0, 0))
    par = pkg.DemodParams(0.995, 0.999, 0.25, 100.0)
    assert L.pddc_demod_create(None, 0, 1, arr, C.byref(par)) == pkg.PDDC_EINVAL
    import torch
    if not torch.cuda.is_available():
        assert create() == pkg.PDDC_ENODEV
        assert create(rx=[(2, 0xFFFFFFFF, 3)] * 1024, params=(0.0, 0.0, 1e-30, 1e30)) == pkg.PDDC_ENODEV
        with pytest.raises(pkg.PddcError) as e:
            pkg.Demod([(pkg.PDDC_DEMOD_AM, 0, 0)])
        assert e.value.code == pkg.PDDC_ENODEV
    with pytest.raises(pkg.PddcError) as e:
        pkg.Demod([(7, 0, 0)])
    assert e.value.code == pkg.PDDC_EINVAL
    assert L.pddc_demod_process(None, None, 8, 8, None, 8, None) == pkg.PDDC_EINVAL
    assert L.pddc_demod_set_rx(None, 0, 0, 0, 0) == pkg.PDDC_EINVAL
    assert L.pddc_demod_reset(None) == pkg.PDDC_EINVAL
    assert L.pddc_demod_destroy(None) == 0
