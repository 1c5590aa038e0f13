"""The MFSK decoder without a GPU: the numpy reference (tests/mfsk_ref.py) against its float32 model and against itself at
every cut, the capacity bound, the clock's behaviour on the reference, the host side of 2G ALE (Golay, interleaving, the
vote) in round trips, and the C ABI's argument errors that need no device."""
import ctypes as C
import itertools

import numpy as np
import pytest

import mfsk_ref as R


def test_the_helpers_are_the_reference_s(pkg):
    """mfsk_modem's taps, inc, q and step are mfsk_ref's, for boxcar and Hann windows, orthogonal and ALE spacing;
    mfsk_encode is mfsk_ref.encode without its noise and carrier phase; the dtypes; ALE's Gray map."""
    for rate, baud, f0, df, M, W, win in ((8000.0, 1000.0, -3500.0, 1000.0, 8, 8, "rect"), (8000.0, 500.0, -750.0, 500.0, 4, 40, "rect"),
                                          (R.ALE_RATE, 125.0, 750.0, 250.0, 8, 80, "hann"), (48000.0, 15.625, 300.0, 15.625, 16, 256, "rect")):
        a = pkg.mfsk_modem(rate, baud, f0, df, M, W, window=win)
        freqs = (f0 + df * np.arange(M)) / rate
        b = R.modem(freqs, W, rate / baud, window=win)
        assert a[0].shape == (M, W) and a[0].tobytes() == b[0].tobytes() and a[1:4] == b[1:], (rate, baud)
        h, inc, q, step = a[:4]
        assert 1 <= inc <= 1 << 29 and 1 <= q <= 64 and 4 * q * inc <= 1 << 32 and step == inc // 64 and a[4:] == (f0, df)
        assert np.abs(np.abs(h.astype(np.complex128)).sum(axis=1) - 1.0).max() < 1e-6
        tones = np.random.default_rng(5).integers(0, M, 12)
        z = pkg.mfsk_encode(tones, a, rate, lead=3.5, ppm=150.0)
        want = R.encode(tones, freqs, (1 << 32) / inc, len(z), lead=3.5, ppm=150.0, seed=0)
        ph = np.exp(2j * np.pi * np.random.default_rng(0).uniform())
        assert np.abs(z * ph - want).max() < 2e-6
    assert pkg.ale_modem(R.ALE_RATE, 80)[1:4] == (54975581, 19, 54975581 // 2) and pkg.ale_modem(R.ALE_RATE, 80)[0].shape == (8, 80)
    assert pkg.mfsk_sym_dtype() == R.SYM and pkg.mfsk_sym_dtype().itemsize == 16 and pkg.mfsk_status_dtype() == R.STATUS
    assert (pkg.PDDC_MFSK_ON, pkg.PDDC_MFSK_REVERSE, pkg.PDDC_MFSK_RESTART, pkg.PDDC_MFSK_MAX_TONES) == (R.ON, R.REVERSE, R.RESTART, R.MAX_TONES)
    assert pkg.ale_tribits(range(8)) == [0, 0, 0, 0, 0, 1, 0, 1, 1, 0, 1, 0, 1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 0, 0]
    with pytest.raises(pkg.PddcError):
        pkg.mfsk_modem(8000.0, 1000.0, 0.0, 1000.0, 33, 8)
    with pytest.raises(pkg.PddcError):
        pkg.mfsk_modem(8000.0, 1001.0, 0.0, 1000.0, 8, 8)             # fewer than 8 samples a symbol


def test_float32_model_against_double():
    """The float32 model against the double reference on the GPU parity test's own inputs (mfsk_ref's header): the worst
    |quality_model - quality_ref| and |best_model - best_ref| per window is the figure written into MODEL_WORST, TOL_MFSK
    is 7 x the largest, MARGIN 4 x that.  The same runs show what the GPU tests rely on: every receiver of the small sets
    and of the slow case keeps a margin of at least MARGIN, of the 1024 at most a quarter fall below it, and the model's
    strobes, records and integer status are the reference's wherever the margin holds."""
    worst = {}
    sets = [(W, 9, R.case(W, 9)) for W in R.WINDOWS] + [("slow", 5, R.slow_case())] + [(W, 1024, R.case(W, 1024)) for W in R.BIG_WINDOWS]
    for key, nrx, (bank, sel, z) in sets:
        W = 256 if key == "slow" else key
        syms, best, margin, st, strobes = R.run_cuts(R.MfskRef(bank, sel, W), z)
        m32 = R.run_cuts(R.MfskRef(bank, sel, W, f32=True), z)
        below = int((margin < R.MARGIN).sum())
        print(f"nrx {nrx} W {key}: least margin {margin.min():.3e} (MARGIN {R.MARGIN:.3e}), {below} below")
        assert below == 0 if nrx < 1024 else below <= nrx // 4, (nrx, key, below)
        w = float(np.abs(m32[1] - best).max())
        for j in range(nrx):
            if margin[j] >= R.MARGIN:
                assert m32[4][j] == strobes[j], (nrx, key, j)
                for k in ("start", "tone", "second", "flags"):
                    assert np.array_equal(m32[0][j][k], syms[j][k]), (nrx, key, j, k)
                assert all(m32[3][k][j] == st[k][j] for k in ("symbols", "acc", "skip", "tone_last"))
            if m32[4][j] == strobes[j] and syms[j].size:
                w = max(w, float(np.abs(m32[0][j]["quality"].astype(np.float64) - syms[j]["quality"]).max()))
        worst[key] = max(worst.get(key, 0.0), w)
        want = R.SLOW_SYMS if key == "slow" else R.PARITY_SYMS
        assert all(want <= s.size <= want + 6 for s in syms), [s.size for s in syms][:9]
    for k, v in worst.items():
        print(f"W = {k}: worst |model32 - ref| of quality and best {v:.3e} (written {R.MODEL_WORST[k]:.3e})")
        assert abs(v - R.MODEL_WORST[k]) <= 0.0005 * R.MODEL_WORST[k] + 1e-12, k
    assert R.TOL_MFSK == 7 * max(R.MODEL_WORST.values()) and R.MARGIN == 4 * R.TOL_MFSK


def same(a, b, exact=True):
    """two results of run_cuts: records, best, status and strobes by their bytes (the margin is a minimum over the
    batches).  Not exact (the double reference, whose filter sums are the matrix library's: their order, and so their
    last bits, go with the batch's length): the integers equal, the floats within 1e-12."""
    if a[4] != b[4] or len(a[0]) != len(b[0]):
        return False
    if exact:
        return (all(x.tobytes() == y.tobytes() for x, y in zip(a[0], b[0])) and a[1].tobytes() == b[1].tobytes()
                and a[3].tobytes() == b[3].tobytes() and np.array_equal(a[2], b[2]))
    ints = all(np.array_equal(x[k], y[k]) for x, y in zip(a[0], b[0]) for k in ("start", "tone", "second", "flags"))
    ints = ints and all(np.array_equal(a[3][k], b[3][k]) for k in ("symbols", "acc", "skip", "tone_last"))
    floats = max([float(np.abs(x["quality"].astype(np.float64) - y["quality"]).max()) for x, y in zip(a[0], b[0]) if x.size]
                 + [float(np.abs(a[1] - b[1]).max()), float(np.abs(a[3]["q_last"].astype(np.float64) - b[3]["q_last"]).max())])
    return ints and floats <= 1e-12


@pytest.mark.parametrize("f32", [False, True])
def test_reference_against_itself_at_every_cut(f32):
    """9 receivers, W = 2, 16 and 256: one batch against every list of cut_lists (batches of 0 and 1, cuts on and beside
    256-sample seams, forty batches of one sample, cuts just before, on and behind a strobe and its late sample) gives the
    same records, best, status and strobes, bit for bit in the float32 model and to the last bits of the matrix library's
    sums in double; and with receiver changes between batches
    at two cuts that share the change points."""
    for W in (2, 16, 256):
        bank, sel, z = R.case(W, 9)
        n = z.shape[1]
        one = R.run_cuts(R.MfskRef(bank, sel, W, f32), z)
        lists = R.cut_lists(n, 256, strobe=one[4][0][20], q=bank[sel[0][0]][2])
        assert len(lists) == 4
        for cuts in lists:
            assert same(R.run_cuts(R.MfskRef(bank, sel, W, f32), z, cuts), one, f32), (W, cuts)

        def changes(at):
            def before(i, r):
                if i == at:
                    r.set_rx(1, sel[1][0], R.ON | R.RESTART)
                    r.set_rx(2, (sel[2][0] + 1) % len(bank), R.ON | R.REVERSE)
                    r.set_rx(3, sel[3][0], 0)
            return before
        a = R.run_cuts(R.MfskRef(bank, sel, W, f32), z, [200, n - 200], changes(1))
        b = R.run_cuts(R.MfskRef(bank, sel, W, f32), z, [1, 199, 0, 63, n - 263], changes(3))
        assert same(a, b, f32) and not same(a, one, False), W
        assert a[3]["symbols"][1] == one[3]["symbols"][1] or abs(int(a[3]["symbols"][1]) - int(one[3]["symbols"][1])) <= 2
        assert a[3]["symbols"][3] < one[3]["symbols"][3]


def test_max_syms_is_never_exceeded():
    """Adversarial inc and step: a receiver whose early sample always wins (the amplitude falls towards every strobe) is
    advanced at every strobe and has its strobes D = floor((2^32 - step) / inc) apart, the least the definition lets
    them be; one whose late sample always wins is delayed every time.  For every batch length from 0 to 2 D + 1 and 255,
    256, 257, at every alignment of the batch to the strobes, the count is at most max_syms(n) -- and equal to it somewhere
    where step = inc and inc is a power of two."""
    for inc, q, step in ((1 << 29, 1, 1 << 29), (1 << 29, 2, 1 << 26), (1 << 28, 4, 1 << 28), (300000000, 1, 300000000), (268425483, 3, 12345),
                         (54975581, 19, 54975581 // 2)):
        bank = [(np.array([[1.0], [0.5]], np.complex64), inc, q, step)]
        D = R.distance(bank)
        assert D == ((1 << 32) - step) // inc >= 7
        n = 1500
        for falling in (True, False):
            # |z| falls (rises) along the series, and so does b: the early (late) sample is the greater at every strobe
            ramp = np.linspace(2.0, 1.0, n) if falling else np.linspace(1.0, 2.0, n)
            z = ramp[None].astype(np.complex64)
            ref = R.run_cuts(R.MfskRef(bank, [(0, R.ON)], 1), z)
            m = np.array(ref[4][0])
            gaps = np.diff(m)
            assert gaps.min() >= D, (inc, step, falling, gaps.min())
            if falling:
                assert (gaps == D).all() or step != inc or inc & (inc - 1), (inc, step)
            hit = np.zeros(n + 600, np.int64)
            hit[m] = 1
            csum = np.concatenate([[0], np.cumsum(hit)])
            for b in list(range(0, 2 * D + 2)) + [255, 256, 257]:
                most = int((csum[b:n + 1] - csum[:n + 1 - b]).max()) if b else 0
                assert most <= R.max_syms(bank, b), (inc, step, b, most)
                if falling and step == inc and not inc & (inc - 1):
                    assert most == R.max_syms(bank, b), (inc, step, b, most)
    assert R.max_syms([(None, 1 << 29, 1, 1 << 29)], 15) == 3 and R.max_syms([(None, 1 << 29, 1, 0)], 16) == 2 and R.max_syms([(None, 1, 1, 0)], 0) == 0


@pytest.mark.parametrize("sps", R.CLOCK_SPS)
def test_the_clock_settles_in_the_middle(sps):
    """mfsk_ref.clock_case on the double reference: CLOCK_SYMS random tones of 8, a baud apart, at 8, 16 and 78.125 samples
    per symbol, the sender's clock 200 ppm off either way, eight starting phases, 20 seeds; complex white noise CLOCK_SNR =
    15 dB below the carrier (at 8 samples a symbol the matched filter leaves 24 dB between a tone and the noise in its
    bin).  step is clock_step: a 64th of a symbol per strobe, at most a sample.  From CLOCK_SETTLE symbols on, every
    symbol has exactly one record, its on-time sample lies within a quarter symbol of the sample at which the filter
    covers the symbol, and its tone is the one sent: 320 of 320 receivers."""
    bank, sel, z, tones, leads, Ts = R.clock_case(sps)
    assert len(sel) == 8 * 2 * R.CLOCK_SEEDS
    L = int(round(sps))
    ref = R.run_cuts(R.MfskRef(bank, sel, L), z)
    bad, worst = [], 0.0
    for j in range(len(sel)):
        rec = ref[0][j]
        x = (rec["start"].astype(np.float64) - leads[j] - (L - 1)) / Ts[j]          # in symbols: whole numbers are the middles
        i = np.round(x).astype(np.int64)
        keep = (i >= R.CLOCK_SETTLE) & (i < R.CLOCK_SYMS)
        off = np.abs(x - i)[keep]
        ok = (np.array_equal(i[keep], np.arange(R.CLOCK_SETTLE, R.CLOCK_SYMS)) and off.max() <= 0.25
              and np.array_equal(rec["tone"][keep], tones[j][R.CLOCK_SETTLE:]))
        worst = max(worst, float(off.max()) if off.size else 1.0)
        if not ok:
            bad.append(j)
    print(f"{sps} samples per symbol: {len(sel) - len(bad)} of {len(sel)} settle, the worst offset behind symbol {R.CLOCK_SETTLE} is {worst:.3f} symbols")
    assert not bad, (sps, bad[:10])


# ---- 2G ALE on the host ------------------------------------------------------------------------------------------------

def test_golay_corrects_three_errors(pkg):
    """The (24, 12) code: 4096 codewords of weight 0, 8, 12, 16 or 24 (distance 8); every pattern of up to 3 errors on one
    codeword is corrected, exhaustively (2325 patterns), and on 200 seeded others, 60 sampled patterns each; 4 errors are
    never miscorrected into another word's data with fewer than 4 (they are refused or -- never -- accepted: the
    distance forbids it)."""
    check = pkg.ale_golay_check
    weights = {bin(d << 12 | check(d)).count("1") for d in range(4096)}
    assert weights == {0, 8, 12, 16, 24}
    assert all(check(a ^ b) == check(a) ^ check(b) for a, b in ((0x123, 0xABC), (0xFFF, 0x001), (0x800, 0x7FF)))
    d0 = 0xA5C
    cw = d0 << 12 | check(d0)
    n = 0
    for w in range(4):
        for bits in itertools.combinations(range(24), w):
            e = sum(1 << b for b in bits)
            assert pkg.ale_golay_decode(cw ^ e) == (d0, w), (bits,)
            n += 1
    assert n == 2325
    rng = np.random.default_rng(24)
    for d in rng.integers(0, 4096, 200):
        cw = int(d) << 12 | check(int(d))
        for _ in range(60):
            w = int(rng.integers(0, 4))
            e = sum(1 << int(b) for b in rng.choice(24, w, replace=False))
            assert pkg.ale_golay_decode(cw ^ e) == (int(d), w)
    for bits in itertools.islice(itertools.combinations(range(24), 4), 0, None, 37):
        assert pkg.ale_golay_decode(cw ^ sum(1 << b for b in bits)) is None


def test_ale_words_round_trip_and_wrong_offsets(pkg):
    """ale_encode -> ale_words on the tones themselves: 49 tones a word; the call comes back at the offsets 0, 49 and 98
    with no bit corrected and no split vote, and no other offset gives a word (ALE_CALL was chosen for that: ale_words'
    docstring says how often a wrong offset decodes).  With 3 wrong tones a word (up to 9 bits, spread over the three
    copies) the vote and the code still give the call.  ale_text joins it.  Words ale_encode refuses."""
    tones = pkg.ale_encode(R.ALE_CALL)
    assert len(tones) == 49 * 3 == pkg.ALE_WORD_SYMBOLS * 3 and set(tones) <= set(range(8))
    words = pkg.ale_words(tones)
    assert [(w["start"], w["preamble"], w["chars"], w["errors"], w["split"]) for w in words] == \
        [(49 * i, p, c, 0, 0) for i, (p, c) in enumerate(R.ALE_CALL)]
    assert pkg.ale_text(words) == "TO KK6 TIS OAM89"
    for off in range(1, 49):                                          # a wrong symbol offset, within a word and across two
        assert not pkg.ale_words(tones[off:off + 49]), off
    assert pkg.ale_words(tones[49:98])[0]["chars"] == "OAM" and not pkg.ale_words(tones[:48])
    rng = np.random.default_rng(141)
    hurt = np.array(tones)
    for w in range(3):
        for k in rng.choice(49, 3, replace=False):
            hurt[49 * w + k] = (hurt[49 * w + k] + 1 + rng.integers(0, 7)) % 8
    got = [w for w in pkg.ale_words(hurt) if w["start"] % 49 == 0]
    assert [(w["preamble"], w["chars"]) for w in got] == R.ALE_CALL
    rec = np.zeros(len(tones), R.SYM)
    rec["tone"], rec["start"] = tones, 1000 + 78 * np.arange(len(tones))
    assert [w["start"] for w in pkg.ale_words(rec)] == [1000, 1000 + 78 * 49, 1000 + 78 * 98]
    for bad in (("XX", "ABC"), ("TO", "AB"), ("TO", "ab1"), (8, "ABC")):
        with pytest.raises((pkg.PddcError, ValueError)):
            pkg.ale_encode([bad])


def test_ale_round_trip_through_the_reference(pkg):
    """ale_encode -> mfsk_encode -> the double reference -> ale_words: ALE_LEAD_SYMS seeded tones for the clock to settle
    on, then the call, at 78.125 samples per symbol (9765.625 Hz), the sender 150 ppm fast and slow and at four starting
    phases, noise 15 dB below: every receiver gives back TO / TIS / DATA with no split vote."""
    m = pkg.ale_modem(R.ALE_RATE, 80)
    lead_tones = list(np.random.default_rng(188).integers(0, 8, R.ALE_LEAD_SYMS))
    tones = lead_tones + pkg.ale_encode(R.ALE_CALL)
    rows = []
    for j in range(8):
        z = pkg.mfsk_encode(tones, m, R.ALE_RATE, lead=20.0 + 78.125 * (j % 4) / 4.0, ppm=150.0 if j < 4 else -150.0,
                            n=int(78.125 * (len(tones) + 3)))
        rng = np.random.default_rng(500 + j)
        rows.append(z + (10.0 ** (-15.0 / 20.0) / np.sqrt(2.0)) * (rng.standard_normal(z.size) + 1j * rng.standard_normal(z.size)))
    ref = R.run_cuts(R.MfskRef([m[:4]], [(0, R.ON)] * 8, 80), np.stack(rows).astype(np.complex64))
    for j in range(8):
        words = [w for w in pkg.ale_words(ref[0][j]) if w["split"] == 0]
        assert [(w["preamble"], w["chars"]) for w in words] == R.ALE_CALL, (j, words)
        assert pkg.ale_text(words) == "TO KK6 TIS OAM89"
        assert np.diff([w["start"] for w in words]).tolist() == pytest.approx([49 * 78.125] * 2, abs=39)         # the clock may still be moving: half a symbol


# ---- the C ABI without a device ----------------------------------------------------------------------------------------

def test_argument_errors_without_a_device(pkg):
    """Create refuses non-finite taps (in any of the 32 tone rows), modems out of range, a bad modem index, unknown flag
    bits, sizes out of range and NULLs with PDDC_EINVAL before it asks for a device; good arguments without a device are
    PDDC_ENODEV.  set_rx, process, max_syms, read, reset on a NULL handle are PDDC_EINVAL."""
    L = pkg.ddc_lib()
    W, B, nrx = 16, 2, 3

    def create(nrx=nrx, W=W, B=B, taps=None, modems=((8, 1 << 28, 4, 1 << 22), (3, 1 << 29, 1, 0)), rx=((0, 1), (1, 3), (1, 0)), null=None):
        t = np.full((B, 32, W, 2), 0.25, np.float32) if taps is None else taps
        k = (pkg.MfskModem * len(modems))(*[pkg.MfskModem(*v) for v in modems])
        arr = (pkg.MfskRx * len(rx))(*[pkg.MfskRx(m, f) for m, f in rx])
        args = [t.ctypes.data_as(C.POINTER(C.c_float)), k, arr]
        if null is not None:
            args[null] = None
        h = C.c_void_p()
        rc = L.pddc_mfsk_create(C.byref(h), 0, nrx, W, B, *args)
        if rc == pkg.PDDC_OK:
            L.pddc_mfsk_destroy(h)
        return rc

    good = pkg.PDDC_OK if L.pddc_device_count() > 0 else pkg.PDDC_ENODEV
    assert create() == good
    for bad in (np.nan, np.inf, -np.inf):
        for where in ((1, 2, W - 1, 1), (0, 31, 0, 0)):
            t = np.full((B, 32, W, 2), 0.25, np.float32)
            t[where] = bad
            assert create(taps=t) == pkg.PDDC_EINVAL
    ok = (8, 1 << 28, 4, 1 << 22)
    for kw in (dict(modems=(ok, (1, 1 << 28, 4, 0))), dict(modems=(ok, (33, 1 << 28, 4, 0))), dict(modems=(ok, (8, 0, 4, 0))),
               dict(modems=(ok, (8, (1 << 29) + 1, 1, 0))), dict(modems=(ok, (8, 1 << 28, 0, 0))), dict(modems=(ok, (8, 1 << 28, 5, 0))),
               dict(modems=(ok, (8, 1 << 24, 65, 0))), dict(modems=(ok, (8, 1 << 28, 4, (1 << 28) + 1))),
               dict(rx=((0, 1), (2, 1), (0, 1))), dict(rx=((0, 1), (-1, 1), (0, 1))), dict(rx=((0, 1), (1, 8), (0, 1))),
               dict(rx=((0, 1), (1, 0x100), (0, 1))), dict(nrx=0), dict(nrx=1025), dict(W=0), dict(W=257), dict(B=0), dict(B=17),
               dict(null=0), dict(null=1), dict(null=2)):
        assert create(**kw) == pkg.PDDC_EINVAL, kw
    # the bounds themselves, REVERSE and RESTART at create
    assert create(modems=((2, 1, 64, 1), (32, 1 << 29, 2, 1 << 29)), rx=((0, 1), (1, 7), (1, 6))) == good
    assert create(modems=((2, 1 << 24, 64, 0), (32, 1 << 29, 1, 0))) == good
    assert L.pddc_mfsk_create(None, 0, nrx, W, B, None, None, None) == pkg.PDDC_EINVAL
    c = C.c_size_t()
    assert L.pddc_mfsk_set_rx(None, 0, 0, 1) == pkg.PDDC_EINVAL
    assert L.pddc_mfsk_process(None, None, 0, 0, None, 0, None, None, 0, None) == pkg.PDDC_EINVAL
    assert L.pddc_mfsk_max_syms(None, 10, C.byref(c)) == pkg.PDDC_EINVAL
    assert L.pddc_mfsk_read(None, None, None) == pkg.PDDC_EINVAL
    assert L.pddc_mfsk_reset(None) == pkg.PDDC_EINVAL
    assert L.pddc_mfsk_destroy(None) == pkg.PDDC_OK
    assert L.pddc_mfsk_tile_outputs() == pkg.mfsk_tile_outputs() == 256
    with pytest.raises(pkg.PddcError) as e:
        pkg.Mfsk([R.modem(R.tone_freqs(8, 16), 16, 16)], [(0, 1)], 8)      # taps of another length than W
    assert e.value.code == pkg.PDDC_EINVAL
