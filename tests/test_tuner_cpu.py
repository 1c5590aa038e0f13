"""The tuner without a GPU: its reference (tests/tuner_ref.py) against the project's oracle DDC, the direct sum with the
shifted prototype and a closed form; the retune rule; the output and channel arithmetic and the argument checks of the C
ABI; the two design helpers; and the float32 models that set the GPU tolerances."""
import ctypes as C

import numpy as np
import pytest

import channelizer_ref as CR
import spectrum_ref as R
import tuner_ref as TR


@pytest.fixture(scope="module")
def lcg19(O):
    packed = O.lcg_bytes(6 << 19, 12345)
    return packed, R.to_complex(O, packed)


def tone_packed(O, n, f_cycles, amp):
    """amp exp(2 pi i f n), f in cycles per sample given as an exact fraction of 2^32 (int) plus a float remainder"""
    word, delta = f_cycles
    t = np.arange(n, dtype=np.int64)
    ph = ((word * t) & TR.MASK).astype(np.float64) / 2.0 ** 32 + delta * t
    x = amp * np.exp(2j * np.pi * ph)
    i = np.clip(np.rint(x.real * 8388607.0), -8388608, 8388607).astype(np.int64)
    q = np.clip(np.rint(x.imag * 8388607.0), -8388608, 8388607).astype(np.int64)
    return O.pack24(i, q).reshape(-1)


@pytest.mark.parametrize("decim", [4, 8])
def test_reference_is_the_oracles_two_stage_chain(O, decim):
    """Words on channel centres, hop M/2: out_j[m] is output (m R + T - 1 + L/D) / R of the oracle's two-stage chain
    [(D, [0, w reversed]), (R, h)] behind the NCO word F_j, to 1e-6 of the largest value (the oracle returns float32).
    M = 1024, P = 4, D = 512: L/D = 8, T = 65, so T - 1 + L/D = 72 is a multiple of R = 4 and 8."""
    M, P, T = 1024, 4, 65
    D, L = M // 2, P * M
    packed = O.lcg_bytes(6 << 18, 12345)
    x = R.to_complex(O, packed)
    w = TR.kaiser_prototype_wide(M, P)
    h = TR.kaiser_lowpass(T, decim)
    y = CR.channelizer_ref(x, M, D, w)
    h1 = np.concatenate([[0.0], w[::-1]]).astype(np.float32)
    words = [k << 22 for k in (0, 1, 37, M // 2, M - 1)]
    ref = TR.tuner_ref(y, M, D, words, h, decim)
    first = (T - 1 + L // D) // decim
    for j, f in enumerate(words):
        c = O.ddc_chain(packed, [(D, h1), (decim, h)], freg=f, mix=True).astype(np.float64)
        c = (c[0::2] + 1j * c[1::2])[first:]
        n = min(c.size, ref.shape[1])
        assert n >= ref.shape[1] - 1 and n > 50
        e = float(np.max(np.abs(c[:n] - ref[j, :n])) / np.max(np.abs(ref[j, :n])))
        print(f"R {decim} word {f:#010x}: {e:.2e} over {n} outputs")
        assert e <= 1e-6, (decim, f, e)


def test_z_is_the_receiver_with_the_shifted_prototype(O):
    """Words off centre (r = -2^(31-b), r = 2^(31-b) - 1, a word that wraps to channel 0 among them):
    z_j[s] = sum_n w[n] e^{+2 pi i r n / 2^32} x[sD + n] e^{-2 pi i F (sD + n) / 2^32}, in double, to 1e-12 of the largest."""
    M, P = 1024, 8
    D, L = M // 2, P * M
    x = R.to_complex(O, O.lcg_bytes(6 << 16, 12345))
    w = TR.kaiser_prototype_wide(M, P).astype(np.float64)
    y = CR.channelizer_ref(x, M, D, w)
    half = 1 << 21
    words = [(5 << 22) - half, (5 << 22) + half - 1, (700 << 22) + 12345, TR.MASK - 5, (1 << 22) - half, 0x12345678]
    assert TR.channel_of(M, words[0]) == (5, -half) and TR.channel_of(M, words[1]) == (5, half - 1)
    assert TR.channel_of(M, words[3]) == (0, -6) and TR.channel_of(M, words[4]) == (1, -half)
    kr = [TR.channel_of(M, f) for f in words]
    z = TR.mix(y[:, [k for k, _ in kr]], [r for _, r in kr], [0] * len(words), D)
    n = np.arange(L, dtype=np.int64)
    for j, f in enumerate(words):
        r = kr[j][1]
        ws = w * np.exp(2j * np.pi * ((r * n) & TR.MASK).astype(np.float64) / 2.0 ** 32)
        direct = np.empty(y.shape[0], complex)
        for s in range(y.shape[0]):
            lo = np.exp(-2j * np.pi * ((f * (s * D + n)) & TR.MASK).astype(np.float64) / 2.0 ** 32)
            direct[s] = np.sum(ws * x[s * D:s * D + L] * lo)
        e = float(np.max(np.abs(direct - z[:, j])) / np.max(np.abs(direct)))
        print(f"word {f:#010x} (k {kr[j][0]}, r {r}): {e:.2e}")
        assert e <= 1e-12, (f, e)


@pytest.mark.parametrize("word", [(300 << 22) - (1 << 21), (17 << 22) + 999, 0xFFFFFFF0])
def test_tone_closed_form(O, word):
    """A 24-bit tone A e^{2 pi i (F / 2^32 + delta) n}:
    out[m] = A sum_n w[n] e^{2 pi i (delta + r / 2^32) n} sum_t h[t] e^{-2 pi i delta D t} e^{2 pi i delta D (m R + T - 1)},
    within the tone's quantisation summed over |w| and |h|."""
    M, P, T, Rd, A = 1024, 8, 64, 4, 0.5
    D = M // 2
    delta = 0.11 / M
    w = TR.kaiser_prototype_wide(M, P)
    h = TR.kaiser_lowpass(T, Rd)
    x = R.to_complex(O, tone_packed(O, 1 << 16, (word, delta), A))
    out = TR.tuner_ref(CR.channelizer_ref(x, M, D, w), M, D, [word], h, Rd)[0]
    r = TR.channel_of(M, word)[1]
    n = np.arange(w.size)
    W = np.sum(w * np.exp(2j * np.pi * (delta + r / 2.0 ** 32) * n))
    H = np.sum(h * np.exp(-2j * np.pi * delta * D * np.arange(T)))
    m = np.arange(out.size)
    want = A * W * H * np.exp(2j * np.pi * delta * D * (m * Rd + T - 1))
    bound = 2.0 ** -23 * np.sum(np.abs(w)) * np.sum(np.abs(h)) * 2
    print(f"word {word:#010x}: max deviation {np.max(np.abs(out - want)):.2e}, bound {bound:.2e}, |out| {abs(want[0]):.4f}")
    assert out.size > 10 and np.max(np.abs(out - want)) <= bound


def test_retune_keeps_the_accumulator(O):
    """A tone at F0 + delta; the receiver starts on F0, is retuned to F1 at row s0 and back to F0 at row s1.  After each
    transient the output is what the accumulator F n + phi says: on F1 the closed form with phi = (F0 - F1) s0 D (the
    phase did not step), and the streaming reference in batches equals the one-shot reference with the rule applied by
    hand, on F1 and back on F0."""
    M, P, T, Rd, A = 1024, 4, 32, 2, 0.5
    D = M // 2
    F0, F1 = (200 << 22) + 77777, (200 << 22) - 300001
    delta = 0.03 / M
    w = TR.kaiser_prototype_wide(M, P)
    h = TR.kaiser_lowpass(T, Rd)
    x = R.to_complex(O, tone_packed(O, 1 << 17, (F0, delta), A))
    y = CR.channelizer_ref(x, M, D, w)
    s0, s1 = 81, 161
    t = TR.TunerRef(M, D, [F0], h, Rd)
    outs = [t.process(y[:s0])]
    t.set_freq(0, F1)
    outs.append(t.process(y[s0:s0 + 1]))
    outs.append(t.process(y[s0 + 1:s1]))
    t.set_freq(0, F0)
    outs.append(t.process(y[s1:]))
    got = np.concatenate(outs, axis=1)[0]
    never = TR.tuner_ref(y, M, D, [F0], h, Rd)[0]
    # back on F0 the offset is what the time on F1 left behind: (F0 - F1) s0 D + (F1 - F0) s1 D
    phi2 = ((F0 - F1) * ((s0 * D) & TR.MASK) + (F1 - F0) * ((s1 * D) & TR.MASK)) & TR.MASK
    assert t.phi[0] == phi2
    back = TR.tuner_ref(y, M, D, [F0], h, Rd, phi=[phi2])[0]
    assert got.size == never.size
    m = np.arange(got.size)
    before = m * Rd + T - 1 < s0
    after = m * Rd >= s1
    assert before.sum() > 10 and after.sum() > 10
    assert np.array_equal(got[before], never[before]) and np.max(np.abs(got[after] - back[after])) <= 1e-15
    # on F1: by hand, z = y[k1] e^{-i theta}, theta = r1 s D + (F0 - F1) s0 D
    phi = ((F0 - F1) * ((s0 * D) & TR.MASK)) & TR.MASK
    hand = TR.tuner_ref(y, M, D, [F1], h, Rd, phi=[phi])[0]
    on1 = (m * Rd >= s0) & (m * Rd + T - 1 < s1)
    assert on1.sum() > 10 and np.max(np.abs(got[on1] - hand[on1])) <= 1e-15
    # and what the accumulator says: the tone sits (F0 - F1) / 2^32 + delta above F1
    r1 = TR.channel_of(M, F1)[1]
    d1 = (F0 - F1) / 2.0 ** 32 + delta
    n = np.arange(w.size)
    W = np.sum(w * np.exp(2j * np.pi * (d1 + r1 / 2.0 ** 32) * n))
    H = np.sum(h * np.exp(-2j * np.pi * d1 * D * np.arange(T)))
    want = A * W * H * np.exp(2j * np.pi * (d1 * D * (m * Rd + T - 1) - phi / 2.0 ** 32))
    bound = 2.0 ** -23 * np.sum(np.abs(w)) * np.sum(np.abs(h)) * 2
    print(f"retuned: max deviation from the closed form {np.max(np.abs(got[on1] - want[on1])):.2e} (bound {bound:.2e})")
    assert np.max(np.abs(got[on1] - want[on1])) <= bound


def test_outputs_and_channel_arithmetic(pkg):
    rng = np.random.default_rng(11)
    for T, Rd in ((1, 1), (64, 4), (512, 64), (3, 64), (65, 8), (512, 1)):
        before = 0
        for _ in range(80):
            n = int(rng.choice([0, 0, 1, Rd - 1, T, int(rng.integers(0, 3000))]))
            want = TR.noutputs_of(before + n, T, Rd) - TR.noutputs_of(before, T, Rd)
            assert pkg.tuner_outputs(T, Rd, before, n) == want, (T, Rd, before, n)
            before += n
    assert pkg.tuner_outputs(64, 4, 0, 131072) == (131072 - 64) // 4 + 1
    for bad in ((0, 1), (513, 1), (8, 0), (8, 65)):
        assert pkg.tuner_outputs(bad[0], bad[1], 0, 1 << 20) == 0
    for M in CR.SIZES:
        b = M.bit_length() - 1
        sh, half = 32 - b, 1 << (31 - b)
        for k in range(M):
            c = k << sh
            assert pkg.tuner_channel(M, c) == (k, 0) == TR.channel_of(M, c)
            assert pkg.tuner_channel(M, (c + 1) & TR.MASK) == (k, 1)
            assert pkg.tuner_channel(M, (c - 1) & TR.MASK) == (k, -1) == TR.channel_of(M, c - 1)
            assert pkg.tuner_channel(M, (c - half) & TR.MASK) == (k, -half)
            assert pkg.tuner_channel(M, (c + half - 1) & TR.MASK) == (k, half - 1)
            assert pkg.tuner_channel(M, (c + half) & TR.MASK) == ((k + 1) % M, -half)
        assert pkg.tuner_channel(M, TR.MASK) == (0, -1)
    with pytest.raises(pkg.PddcError) as e:
        pkg.tuner_channel(512, 0)
    assert e.value.code == pkg.PDDC_EINVAL


def test_argument_errors_without_a_device(pkg):
    L = pkg.ddc_lib()
    h = np.ones(512, np.float32)
    ph = h.ctypes.data_as(C.POINTER(C.c_float))
    f = np.array([5 << 22, 6 << 22, (900 << 22) + 5], np.uint32)
    pf = f.ctypes.data_as(C.POINTER(C.c_uint32))

    def create(nchan=1024, hop=512, first=0, count=1024, freg=pf, nrx=3, taps=ph, ntaps=64, decim=4, flags=0):
        t = C.c_void_p()
        rc = L.pddc_tuner_create(C.byref(t), 0, nchan, hop, first, count, freg, nrx, taps, ntaps, decim, flags)
        if rc == 0:
            L.pddc_tuner_destroy(t)
        return rc

    bad = [dict(nchan=512, hop=512, count=512), dict(nchan=3000, hop=3000), dict(nchan=8192, hop=8192), dict(hop=256),
           dict(hop=0), dict(hop=2048), dict(first=-1), dict(first=1024), dict(count=0), dict(count=1025), dict(freg=None),
           dict(nrx=0), dict(nrx=1025), dict(taps=None), dict(ntaps=0), dict(ntaps=513), dict(decim=0), dict(decim=65),
           dict(flags=1), dict(first=0, count=900), dict(first=6, count=1000), dict(first=901, count=100)]
    for kw in bad:
        assert create(**kw) == pkg.PDDC_EINVAL, kw
    assert L.pddc_tuner_create(None, 0, 1024, 512, 0, 1024, pf, 3, ph, 64, 4, 0) == pkg.PDDC_EINVAL
    import torch
    if not torch.cuda.is_available():
        assert create() == pkg.PDDC_ENODEV
        assert create(first=900, count=1024 - 900 + 7, ntaps=512, decim=64) == pkg.PDDC_ENODEV      # a wrapping range
        with pytest.raises(pkg.PddcError) as e:
            class Ch:
                nchan, hop, device, first, count = 1024, 512, 0, 0, 1024
            pkg.Tuner(Ch, [1 << 22], pkg.tuner_lowpass(64, 4), 4)
        assert e.value.code == pkg.PDDC_ENODEV
    assert L.pddc_tuner_process(None, None, 8, None, 0, None, None) == pkg.PDDC_EINVAL
    assert L.pddc_tuner_set_freq(None, 0, 0) == pkg.PDDC_EINVAL
    assert L.pddc_tuner_set_range(None, 0, 1) == pkg.PDDC_EINVAL
    assert L.pddc_tuner_reset(None) == pkg.PDDC_EINVAL
    assert L.pddc_tuner_next_outputs(None, 1 << 20) == 0
    assert L.pddc_tuner_destroy(None) == 0
    assert L.pddc_tuner_channel(512, 0, None, None) == pkg.PDDC_EINVAL
    assert L.pddc_tuner_channel(1024, 0, None, None) == 0


def passband_and_stopband(w, M, half_width):
    """the worst-placed receiver (half a spacing off its centre): pass-band variation in dB over +-half_width spacings,
    and the largest response, in dB below DC, at anything that folds into that band at hop M/2 (>= 1.5 - half_width)"""
    w = np.asarray(w, np.float64)
    n = np.arange(w.size)
    resp = lambda f: np.abs(np.exp(-2j * np.pi * np.outer(f, n) / M) @ w)
    p = resp(0.5 + np.linspace(-half_width, half_width, 41))
    s = resp(np.linspace(1.5 - half_width, M / 2, 4001))
    return 20 * np.log10(p.max() / p.min()), -20 * np.log10(s.max() / np.sum(w))


def test_design_helpers(pkg):
    """tuner_prototype and tuner_lowpass: symmetric, sum 1, float32, equal to the restatements in tuner_ref; and the
    worst-placed receiver sees less pass-band variation with tuner_prototype than with channelizer_prototype."""
    for M, P in ((1024, 4), (1024, 8), (4096, 4)):
        w = pkg.tuner_prototype(M, P)
        assert w.dtype == np.float32 and w.size == M * P and np.array_equal(w, w[::-1])
        assert abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-6
        assert np.array_equal(w, TR.kaiser_prototype_wide(M, P))
        var_t, stop_t = passband_and_stopband(w, M, 0.1)
        var_c, stop_c = passband_and_stopband(pkg.channelizer_prototype(M, P), M, 0.1)
        print(f"M {M} P {P}: pass-band variation of the worst-placed receiver (half width 0.1 spacings) "
              f"{var_t:.4f} dB with tuner_prototype, {var_c:.2f} dB with channelizer_prototype; "
              f"what folds into it is {stop_t:.1f} dB down ({stop_c:.1f} dB)")
        assert var_t < var_c
    for T, Rd in ((64, 4), (512, 64), (65, 8)):
        h = pkg.tuner_lowpass(T, Rd)
        assert h.dtype == np.float32 and h.size == T and np.array_equal(h, h[::-1])
        assert abs(float(h.astype(np.float64).sum()) - 1.0) < 1e-6 and np.array_equal(h, TR.kaiser_lowpass(T, Rd))


def test_float32_models_against_double(lcg19):
    """The measurement that sets the GPU tolerances (metric: max |out - ref| / max |ref| over all receivers and
    outputs; 2^19 LCG samples, the 1024 receivers of the GPU parity test).  Tuner alone: the float32 model against the
    double reference on the same complex64-rounded rows.  Chain: channelizer_model_f32 -> tuner model against double on
    double.  TOL = 7 x the worst case of each; a re-measurement may not exceed the written worst cases by more than 0.5 %."""
    _, x = lcg19
    worst_t = worst_c = 0.0
    for M in (1024, 4096):
        words = TR.receiver_set(M, 1024)
        kr = [TR.channel_of(M, f) for f in words]
        cols, res = np.array([k for k, _ in kr]), [r for _, r in kr]
        phi = [0] * len(words)
        w = TR.kaiser_prototype_wide(M, 4)
        for D in (M, M // 2):
            y = CR.channelizer_ref(x, M, D, w)[:, cols]
            y32 = CR.channelizer_model_f32(x, M, D, w)[:, cols]
            y64r = y.astype(np.complex64)
            z, zr = TR.mix(y, res, phi, D), TR.mix(y64r.astype(np.complex128), res, phi, D)
            for T, Rd in TR.CASES_TR:
                for name, h in (("kaiser", TR.kaiser_lowpass(T, Rd)), ("random", TR.random_lowpass(T))):
                    if TR.noutputs_of(y.shape[0], T, Rd) == 0:
                        continue
                    et = TR.err(TR.tuner_model_f32(y64r, res, phi, D, h, Rd), TR.fir_decim(zr, h, Rd).T)
                    ec = TR.err(TR.tuner_model_f32(y32, res, phi, D, h, Rd), TR.fir_decim(z, h, Rd).T)
                    print(f"M {M} D {D} T {T} R {Rd} {name}: tuner {et:.3e} chain {ec:.3e}")
                    worst_t, worst_c = max(worst_t, et), max(worst_c, ec)
    print(f"worst: tuner {worst_t:.3e} (TOL_TUNER {TR.TOL_TUNER:.3e}), chain {worst_c:.3e} (TOL_CHAIN {TR.TOL_CHAIN:.3e})")
    assert worst_t <= 1.005 * TR.MODEL_WORST_TUNER and worst_c <= 1.005 * TR.MODEL_WORST_CHAIN
    assert TR.TOL_TUNER == 7 * TR.MODEL_WORST_TUNER and TR.TOL_CHAIN == 7 * TR.MODEL_WORST_CHAIN


def test_receiver_set_in_a_wrapped_range():
    """receiver_set_in: every word's channel lies in the range, wrapped or not; the boundary residues sit on the range's
    first and last channel and on channel 0 where the range holds it; two words are identical; about nrx / count
    receivers share a column."""
    for M, first, count, nrx in ((1024, 1024 - 20, 64, 1024), (4096, 4094, 4, 16), (1024, 100, 50, 300), (1024, 0, 1024, 64)):
        words = TR.receiver_set_in(M, first, count, nrx)
        assert len(words) == nrx and words == TR.receiver_set_in(M, first, count, nrx)
        cols = TR.columns_of(M, first, words)
        assert cols.min() >= 0 and cols.max() < count
        half = 1 << (31 - (M.bit_length() - 1))
        kr = [TR.channel_of(M, f) for f in words]
        ends = [first, (first + count - 1) % M] + ([0] if (0 - first) % M < count and first and (first + count - 1) % M else [])
        for k in ends:
            for r in (-half, -1, 0, 1, half - 1):
                assert (k, r) in kr, (M, first, k, r)
        if nrx > 5 * len(ends) + 1:
            assert len(set(words)) < nrx
    cols = TR.columns_of(1024, 1024 - 20, TR.receiver_set_in(1024, 1024 - 20, 64, 1024))
    per = np.bincount(cols, minlength=64)
    print(f"receivers per column, K 1024 on 64: {per.min()} .. {per.max()}")
    assert per.min() >= 4 and per.max() >= 16 and (cols == 20).sum() >= 5          # channel 0 is column 20


def test_fir_decim_mm_is_fir_decim():
    """The sliding-window matrix product gives fir_decim's sums (another order, in double): <= 1e-13 of the largest value,
    at sizes on both sides of its block and with a ragged last block."""
    rng = np.random.default_rng(3)
    for T, Rd, S in ((1, 1, 50), (2, 1, 300), (5, 4, 333), (64, 64, 1000), (130, 7, 1500), (512, 1, 1500), (512, 63, 1500),
                     (64, 4, 63), (64, 4, 64)):
        z = rng.standard_normal((S, 7)) + 1j * rng.standard_normal((S, 7))
        for h in (TR.random_lowpass(T), TR.kaiser_lowpass(T, Rd)):
            a, b = TR.fir_decim(z, h, Rd), TR.fir_decim_mm(z, h, Rd)
            assert a.shape == b.shape == (TR.noutputs_of(S, T, Rd), 7)
            if a.size:
                assert TR.err(b, a) <= 1e-13, (T, Rd, TR.err(b, a))
                assert TR.err(TR.fir_decim_mm(z, h, Rd, block=3), a) <= 1e-13


def test_tunerref_from_a_row_offset():
    """A TunerRef started at row0 = 1000 with the words and the phi a full run had there, handed the rows from 1000 on
    with the same later retune, gives the full run's outputs from output 1000 / R on: <= 1e-12 of the largest value.  The
    phi there is also what the rule gives in exact integers."""
    M, D, T, Rd, S, row0 = 1024, 512, 64, 4, 3000, 1000
    first, count = 1024 - 20, 64
    y = TR.gaussian_rows(S, count, seed=5).astype(np.complex128)
    words = TR.receiver_set_in(M, first, count, 12)
    h = TR.kaiser_lowpass(T, Rd)
    f1, f2, f3 = (3 << 22) + 4321, (1023 << 22) - 77, (0 << 22) + (1 << 21) - 1
    full = TR.TunerRef(M, D, words, h, Rd)
    outs = [full.process(y[:400], first)]
    full.set_freq(2, f1)
    full.set_freq(5, f2)
    outs.append(full.process(y[400:row0], first))
    there_words, there_phi = list(full.words), list(full.phi)
    assert there_phi[2] == ((words[2] - f1) * ((400 * D) & TR.MASK)) & TR.MASK and there_phi[0] == 0
    outs.append(full.process(y[row0:1200], first))
    full.set_freq(2, f3)
    outs.append(full.process(y[1200:], first))
    want = np.concatenate(outs, axis=1)
    part = TR.TunerRef(M, D, there_words, h, Rd, row0=row0, phi=there_phi)
    got = [part.process(y[row0:1200], first)]
    part.set_freq(2, f3)
    got.append(part.process(y[1200:], first))
    got = np.concatenate(got, axis=1)
    assert part.phi == full.phi
    assert got.shape[1] == TR.noutputs_of(S - row0, T, Rd) and want.shape[1] == TR.noutputs_of(S, T, Rd)
    e = TR.err(got, want[:, row0 // Rd:])
    print(f"TunerRef from row {row0}: {e:.2e}")
    assert e <= 1e-12
    one = TR.tuner_ref_range(y[row0:], M, D, first, there_words, h, Rd, phi=there_phi, row0=row0)
    before = np.arange(one.shape[1]) * Rd + T - 1 < 1200 - row0
    assert before.sum() > 10 and TR.err(one[:, before], got[:, before]) <= 1e-12


def test_schedule_refuses_a_null_handle(pkg):
    o = (C.c_int * 5)()
    assert pkg.ddc_lib().pddc_tuner_schedule(None, 100, o) == pkg.PDDC_EINVAL
    assert pkg.ddc_lib().pddc_tuner_schedule(None, 100, None) == pkg.PDDC_EINVAL


def test_float32_model_on_the_shape_cases():
    """The measurement that sets TOL_TUNER_SHAPES, on the inputs of tests/test_gpu_tuner_shapes.py: the float32 model
    against the double reference on the same complex64 rows (seeded Gaussian, seed 99).  (a) 8300 rows of the wrapped
    64-channel range of M = 1024, hop 512, the 1024 receivers of receiver_set_in, every (T, R) of CASES_TR_SHAPES, Kaiser
    and random h; (b) the deep windows: M = 4096, hop 4096 and 2048, 16 receivers on the wrapped 4-channel range, 4096
    rows from row0 = v - 2048 and w - 2048 (s D passes 2^31 at v, 2^32 at w), (T, R) of CASES_DEEP.  A re-measurement may
    not exceed the written worst case by more than 0.5 %."""
    worst = 0.0
    M, D, first, count, S = TR.SHAPES_GRID
    y64 = TR.gaussian_rows(S, count)
    words = TR.receiver_set_in(M, first, count, 1024)
    res = [TR.channel_of(M, f)[1] for f in words]
    phi = [0] * len(words)
    ycols = y64[:, TR.columns_of(M, first, words)]
    z = TR.mix(ycols.astype(np.complex128), res, phi, D)
    for T, Rd in TR.CASES_TR_SHAPES:
        for name, h in (("kaiser", TR.kaiser_lowpass(T, Rd)), ("random", TR.random_lowpass(T))):
            e = TR.err(TR.tuner_model_f32(ycols, res, phi, D, h, Rd), TR.fir_decim_mm(z, h, Rd).T)
            print(f"T {T} R {Rd} {name}: {e:.3e}")
            worst = max(worst, e)
    M, first, count = TR.DEEP_GRID
    words = TR.receiver_set_in(M, first, count, 16)
    res = [TR.channel_of(M, f)[1] for f in words]
    phi = [0] * len(words)
    for D in (4096, 2048):
        w = (1 << 32) // D
        rows = TR.gaussian_rows(w + 4096, count)
        for row0 in (w // 2 - 2048, w - 2048):
            ycols = rows[row0:row0 + 4096][:, TR.columns_of(M, first, words)]
            z = TR.mix(ycols.astype(np.complex128), res, phi, D, row0)
            for T, Rd in TR.CASES_DEEP:
                for name, h in (("kaiser", TR.kaiser_lowpass(T, Rd)), ("random", TR.random_lowpass(T))):
                    e = TR.err(TR.tuner_model_f32(ycols, res, phi, D, h, Rd, row0), TR.fir_decim_mm(z, h, Rd).T)
                    print(f"deep D {D} row0 {row0} T {T} R {Rd} {name}: {e:.3e}")
                    worst = max(worst, e)
    print(f"worst: {worst:.3e} (MODEL_WORST_TUNER_SHAPES {TR.MODEL_WORST_TUNER_SHAPES:.3e}, TOL {TR.TOL_TUNER_SHAPES:.3e})")
    assert worst <= 1.005 * TR.MODEL_WORST_TUNER_SHAPES
    assert TR.TOL_TUNER_SHAPES == 7 * TR.MODEL_WORST_TUNER_SHAPES
