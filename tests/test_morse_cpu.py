"""The Morse decoder without a GPU: the numpy reference (tests/morse_ref.py) decodes its own signal from any starting
speed, is independent of the cut, its float32 model gives the GPU tolerance, every receiver of the GPU cases keeps its
margin, the capacity bound holds and is reached, the helpers match their restatements, and argument errors are reported
as such with or without a device."""
import ctypes as C

import numpy as np
import pytest

import morse_ref as M


@pytest.mark.parametrize("spd", [16, 40])
def test_reference_decodes_the_quick_brown_fox(pkg, spd):
    """"VVV THE QUICK BROWN FOX 73" keyed at `spd` samples per dot (dot 1, dash 3, gaps 1 / 3 / 7), a carrier with noise
    20 dB below it, seeds 0 .. 19, through MorseRef with Morse's default parameters and morse_keyer's Hann window of half
    a dot, the tracker starting from 0.4, 1 and 2.5 times the true speed (60 receivers side by side): morse_text reads
    everything from "THE" onwards for every seed and start, and the restated decoder agrees.  What comes before "THE" is
    the tracker's to spoil: the first block of a transmission is lost, and a wrong starting speed takes a few pairs of
    marks to leave.
    The dot estimate ends near the truth, a little below it: behind the Hann window of L = spd / 2 samples the power
    passes a_on = 0.5 of the peak where the window's running sum is 0.707, 0.62 L behind a rising edge, and a_off = 0.3
    where it is 1 - 0.548, 0.47 L behind a falling one, so every mark reads 0.15 L = 0.075 dots short and a dot beside a
    dash, 4 dots, gives two dots 3.75 % short; the two marks' four edges are each read to a sample, half a sample in the
    mean of two, 2 / (4 spd); and 3 % are left for what noise 20 dB down does to the edges of the last pairs (shift 2
    weighs the last pair with a quarter).  The bound is the sum, 9.9 % at 16 and 8.0 % at 40 samples per dot."""
    rate, wpm, W = spd * 20.0 / 1.2, 20.0, spd // 2
    h, two0, two_min, two_max, shift = pkg.morse_keyer(rate, wpm, W)
    assert two0 == M.two_of(spd) and two_min == two0 // 3 + (two0 % 3 > 1) and two_max == 4 * two0 and shift == 2
    assert abs(float(h.sum()) - 1.0) < 1e-6 and (h > 0).all()
    speeds = (0.4, 1.0, 2.5)
    bank = [(h, int(s * two0), two_min, two_max, shift) for s in speeds]
    line = M.keying(M.TEXT, spd, 3 * spd, 8 * spd)
    z = np.stack([M.keyed_carrier(line, 20.0, seed) for seed in range(20) for _ in speeds])
    sel = [(b, M.ON) for _ in range(20) for b in range(3)]
    chars, p, margin, st, peak = M.run_cuts(M.MorseRef(bank, sel, W, **M.PARAMS), z)
    for j, c in enumerate(chars):
        text = pkg.morse_text(c)
        assert text == M.decode(c) and text.endswith("THE QUICK BROWN FOX 73"), (j, text)
        assert abs(int(st["two"][j]) - two0) <= (0.0375 + 2.0 / (4 * spd) + 0.03) * two0, (j, st["two"][j], two0)
        assert st["chars"][j] == c.size and st["nel"][j] == 0 and st["key"][j] == 0
    # FIXED at the true speed decodes as well, and never moves two
    fixed = M.run_cuts(M.MorseRef(bank, [(1, M.ON | M.FIXED)] * 4, W, **M.PARAMS), z[1:12:3])
    assert all(M.decode(c).endswith("THE QUICK BROWN FOX 73") and (c["two"] == two0).all() for c in fixed[0])


@pytest.mark.parametrize("W", [2, 16, 256])
def test_reference_is_cut_independent(W):
    """5 receivers of the parity case, one batch against every cut list (batches of 0 and 1, cuts at 63, 64, 65 and on the
    seams of 256): the float32 model's p, characters and status by their bits; the double reference's characters and
    integer status equal, its p within 1e-14 of the peak (its filter is a matrix product, whose summation order numpy
    does not pin)."""
    bank, sel, z = M.case(W, 5)
    for f32 in (True, False):
        one = M.run_cuts(M.MorseRef(bank, sel, W, f32=f32, **M.CASE_PARAMS), z)
        for cuts in M.cut_lists(z.shape[1], 256):
            assert sum(cuts) == z.shape[1] and 1 in cuts
            got = M.run_cuts(M.MorseRef(bank, sel, W, f32=f32, **M.CASE_PARAMS), z, cuts)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got[0], one[0]))
            if f32:
                assert got[1].tobytes() == one[1].tobytes() and got[3].tobytes() == one[3].tobytes()
            else:
                assert np.abs(got[1] - one[1]).max() <= 1e-14 * one[4].max()
                assert all(np.array_equal(got[3][k], one[3][k]) for k in ("chars", "marks", "two", "nel", "key"))


def test_float32_model_against_double():
    """The float32 model against the double reference on the GPU parity test's own inputs, every receiver of every case
    (morse_ref's header): the worst |p_model - p_ref| / peak per window is the figure written into MODEL_WORST,
    TOL_MORSE is 7 x the largest.  The same runs show what the GPU tests rely on: every receiver of the small sets keeps
    a margin of at least MARGIN, of the 1024 at most 10 % fall below it, every receiver that has a text reads it, and
    the model's characters and integer status are the reference's wherever the margin holds."""
    worst = {}
    for nrx in (9, 1024):
        for W in M.WINDOWS:
            bank, sel, z = M.case(W, nrx)
            chars, p, margin, st, peak = M.run_cuts(M.MorseRef(bank, sel, W, **M.CASE_PARAMS), z)
            m32 = M.run_cuts(M.MorseRef(bank, sel, W, f32=True, **M.CASE_PARAMS), z)
            worst[W] = max(worst.get(W, 0.0), float((np.abs(m32[1].astype(np.float64) - p) / peak[:, None]).max()))
            below = int((margin < M.MARGIN).sum())
            print(f"nrx {nrx} W {W}: least margin {margin.min():.3e} (MARGIN {M.MARGIN:.3e}), {below} below")
            assert below == 0 if nrx == 9 else below <= nrx // 10, (nrx, W, below)
            for j, c in enumerate(chars):
                want = M.case_text(W, j)
                if want is not None:
                    assert M.decode(c).endswith(want), (nrx, W, j, M.decode(c))
                if margin[j] >= M.MARGIN:
                    assert m32[0][j].tobytes() == c.tobytes(), (nrx, W, j)
                    assert all(m32[3][k][j] == st[k][j] for k in ("chars", "marks", "two", "nel", "key"))
            if W > 16:                                                # FIXED receivers keep the speed they start from
                fixed = [j for j in range(nrx) if j % 4 == 3]
                assert all(st["two"][j] == bank[(7 * j + 3) % 16][1] for j in fixed)
                assert len({int(st["two"][j]) for j in range(nrx)}) > 3
    for k, v in worst.items():
        print(f"W = {k}: worst |p_model32 - p_ref| / peak {v:.3e} (written {M.MODEL_WORST[k]:.3e})")
        assert abs(v - M.MODEL_WORST[k]) <= 0.0005 * M.MODEL_WORST[k] + 1e-12, k
    assert M.MODEL_WORST_MORSE == max(M.MODEL_WORST.values())
    assert M.TOL_MORSE == 7 * M.MODEL_WORST_MORSE and M.MARGIN == 100 * M.TOL_MORSE


def test_margins_of_the_other_gpu_cases():
    """The cases of tests/test_gpu_morse.py that compare every receiver exactly, run on the reference alone: the series
    of TT - 1 .. 2 TT + 1 samples and the receiver control case under its changes keep every margin."""
    bank, sel, z = M.case(16, 5)
    for n in (255, 256, 257, 513):
        assert (M.run_cuts(M.MorseRef(bank, sel, 16, **M.CASE_PARAMS), z[:, :n])[2] >= M.MARGIN).all(), n
    bank = [M.tailed_keyer(16, 0), M.tailed_keyer(16, 0, speed=2.5, shift=0)]
    sel = [(0, M.ON), (0, 0), (0, 0), (0, M.ON), (0, M.ON), (0, M.ON), (1, M.ON | M.FIXED)]

    def before(i, r):
        if i == 1:
            r.set_rx(2, 0, M.ON)
            r.set_rx(3, 0, M.ON | M.RESTART)
        if i == 2:
            r.set_rx(4, 1, M.ON)
            r.set_rx(5, 0, 0)
            r.set_rx(0, 0, M.ON | M.FIXED)
    chars, p, margin, st, peak = M.run_cuts(M.MorseRef(bank, sel, 16, **M.CASE_PARAMS), M.parity_inputs(9)[:7], [460, 200, 640], before)
    assert (margin >= M.MARGIN).all(), margin
    assert not p[1].any() and chars[1].size == 0 and st["two"][1] == bank[0][1] and st["two"][6] == bank[1][1]
    assert st["chars"][3] == chars[3].size and chars[2]["start"].min() >= 460 and chars[5]["start"].max() < 660


def test_capacity_bound_is_never_exceeded_and_is_reached():
    """W = 1, h = 1, a clean line.  Random keying with marks and gaps of 1 .. 12 samples under keyers with two_min = 512
    and 1300, cut into random batches: no batch holds more characters than max_chars(n).  Marks of one sample with gaps
    of gc samples, the closest the definition allows (the next mark on the emission's own sample): behind the first
    block every batch that begins on a mark holds exactly max_chars(n) characters, so the bound is reached."""
    rng = np.random.default_rng(11)
    one = np.ones(1, np.float32)
    for two in (512, 1300):
        bank = [(one, two, two, 4 * two, 1)]
        D = M.distance(bank)
        assert D == 1 + ((two + 255) >> 8) and M.max_chars(bank, 0) == 0 and M.max_chars(bank, 1) == 1 == M.max_chars(bank, D)
        assert M.max_chars(bank, D + 1) == 2
        lines = []
        for _ in range(8):
            runs = rng.integers(1, 13, 400)
            lines.append(np.repeat(np.arange(400) % 2 == 0, runs)[:1500])
        z = np.stack(lines).astype(np.complex64)
        r, off, total = M.MorseRef(bank, [(0, M.ON)] * 8, 1, **M.PARAMS), 0, 0
        while off < 1500:
            b = int(min(rng.integers(0, 90), 1500 - off))
            _, counts, _, _ = r.process(z[:, off:off + b])
            assert (counts <= M.max_chars(bank, b)).all(), (two, off, b, counts)
            off, total = off + b, total + int(counts.sum())
        assert total > 200
        # back to back
        n = 64 * D + 256 + D
        z = np.zeros((1, n), np.complex64)
        z[0, ::D] = 1.0
        for b in list(range(0, 3 * D + 2)) + [64, 255]:
            r = M.MorseRef(bank, [(0, M.ON | M.FIXED)], 1, **M.PARAMS)
            first = r.process(z[:, :64 * D])[0][0]
            assert (np.diff(first["start"].astype(np.int64)) == D).all() and first.size >= 40
            counts = r.process(z[:, 64 * D:64 * D + b])[1]
            assert counts[0] == M.max_chars(bank, b), (two, b, counts)


def test_helpers_against_restatements(pkg):
    """morse_keyer against morse_ref.keyer (taps by their bits), morse_text against decode on every code of the table, on
    unknown codes and with the WORD and LONG flags, the two dtypes and the flag values against the reference's."""
    for rate, wpm, W, kw in ((266.667, 20.0, 8, {}), (8000.0, 25.0, 256, dict(wpm_min=10, wpm_max=40, shift=3)),
                             (1000.0, 12.0, 40, {}), (48.0, 30.0, 1, dict(shift=0)), (100.0, 60.0, 4, dict(wpm_min=60, wpm_max=60))):
        got, want = pkg.morse_keyer(rate, wpm, W, **kw), M.keyer(rate, wpm, W, **kw)
        assert got[0].dtype == np.float32 and got[0].shape == (W,)
        assert got[0].tobytes() == want[0].tobytes() and tuple(got[1:]) == tuple(want[1:])
        assert 512 <= got[2] <= got[1] <= got[3] <= 1 << 28 and abs(float(got[0].sum()) - 1.0) < 1e-6
        L = min(W, max(1, int(round(0.6 * rate / wpm))))
        assert (got[0][:L] > 0).all() and not got[0][L:].any()
    assert pkg.morse_keyer(16 * 20 / 1.2, 20, 8)[1] == 2 * 16 * 256
    for bad in (dict(rate_hz=0.0, wpm=20, W=8), dict(rate_hz=100.0, wpm=0, W=8), dict(rate_hz=100.0, wpm=20, W=0),
                dict(rate_hz=100.0, wpm=20, W=8, wpm_min=30, wpm_max=20)):
        with pytest.raises(pkg.PddcError):
            pkg.morse_keyer(**bad)
    rec = np.zeros(len(M.ITU) + 4, M.CHAR)
    rec["code"][:len(M.ITU)] = [M.code_of(ch) for ch in M.ITU]
    rec["code"][len(M.ITU):] = [1, 0b1000000, 0xFFFF, M.code_of("K")]
    rec["flags"][::5] = M.WORD
    rec["flags"][-1] = M.LONG | M.WORD
    text = pkg.morse_text(rec)
    assert text == M.decode(rec) and text.replace(" ", "").startswith("".join(M.ITU)) and text.endswith("??? ?")
    assert text.count(" ") == len(range(5, rec.size, 5)) + (0 if (rec.size - 1) % 5 == 0 else 1)
    assert pkg.morse_text(rec[:0]) == ""
    paris = np.zeros(5, M.CHAR)
    paris["code"], paris["flags"][0] = [M.code_of(c) for c in "PARIS"], M.WORD
    assert pkg.morse_text(paris) == "PARIS" and M.code_of("A") == 0b101 and M.code_of("E") == 0b10
    assert pkg.morse_char_dtype() == M.CHAR and M.CHAR.itemsize == 16 and pkg.morse_status_dtype() == M.STATUS
    assert (pkg.PDDC_MORSE_ON, pkg.PDDC_MORSE_FIXED, pkg.PDDC_MORSE_RESTART) == (M.ON, M.FIXED, M.RESTART)
    assert (pkg.PDDC_MORSE_WORD, pkg.PDDC_MORSE_LONG) == (M.WORD, M.LONG)


def test_argument_errors_without_a_device(pkg):
    """Create refuses non-finite taps, keyers and parameters out of range, a bad keyer index, unknown flag bits, sizes out
    of range and NULLs with PDDC_EINVAL before it asks for a device; good arguments without a device are PDDC_ENODEV.
    set_rx, process, max_chars, read, reset on a NULL handle are PDDC_EINVAL."""
    L = pkg.ddc_lib()
    W, B, nrx = 16, 2, 3

    def create(nrx=nrx, W=W, B=B, taps=None, keyers=((8192, 2048, 32768, 2), (512, 512, 1 << 28, 8)),
               par=(0.5, 0.3, 1 / 16, 1 / 64, 4.0), rx=((0, 1), (1, 3), (1, 0)), null=None):
        t = np.full((B, W), 0.25, np.float32) if taps is None else taps
        k = (pkg.MorseKeyer * len(keyers))(*[pkg.MorseKeyer(*v) for v in keyers])
        p = pkg.MorseParams(*par)
        arr = (pkg.MorseRx * len(rx))(*[pkg.MorseRx(m, f) for m, f in rx])
        args = [t.ctypes.data_as(C.POINTER(C.c_float)), k, C.pointer(p), arr]
        if null is not None:
            args[null] = None
        h = C.c_void_p()
        rc = L.pddc_morse_create(C.byref(h), 0, nrx, W, B, *args)
        if rc == pkg.PDDC_OK:
            L.pddc_morse_destroy(h)
        return rc

    good = pkg.PDDC_OK if L.pddc_device_count() > 0 else pkg.PDDC_ENODEV
    assert create() == good
    for bad in (np.nan, np.inf, -np.inf):
        t = np.full((B, W), 0.25, np.float32)
        t[1, W - 1] = bad
        assert create(taps=t) == pkg.PDDC_EINVAL
    ok = (8192, 2048, 32768, 2)
    for kw in (dict(keyers=(ok, (511, 511, 600, 0))), dict(keyers=(ok, (600, 601, 700, 0))), dict(keyers=(ok, (701, 600, 700, 0))),
               dict(keyers=(ok, (600, 600, (1 << 28) + 1, 0))), dict(keyers=(ok, (600, 600, 700, 9))),
               dict(par=(0.5, 0.0, 0.1, 0.1, 4.0)), dict(par=(0.3, 0.5, 0.1, 0.1, 4.0)), dict(par=(1.0, 0.3, 0.1, 0.1, 4.0)),
               dict(par=(0.5, 0.3, -0.1, 0.1, 4.0)), dict(par=(0.5, 0.3, 0.1, 1.5, 4.0)), dict(par=(0.5, 0.3, 0.1, 0.1, 0.5)),
               dict(par=(np.nan, 0.3, 0.1, 0.1, 4.0)), dict(par=(0.5, 0.3, np.nan, 0.1, 4.0)), dict(par=(0.5, 0.3, 0.1, 0.1, np.nan)),
               dict(rx=((0, 1), (2, 1), (0, 1))), dict(rx=((0, 1), (-1, 1), (0, 1))), dict(rx=((0, 1), (1, 8), (0, 1))),
               dict(rx=((0, 1), (1, 0x100), (0, 1))), dict(nrx=0), dict(nrx=1025), dict(W=0), dict(W=257), dict(B=0), dict(B=17),
               dict(null=0), dict(null=1), dict(null=2), dict(null=3)):
        assert create(**kw) == pkg.PDDC_EINVAL, kw
    # the bounds themselves, RESTART at create
    assert create(par=(0.5, 0.5, 0.0, 1.0, 1.0), keyers=((512, 512, 512, 0), (1 << 28, 1 << 28, 1 << 28, 8)),
                  rx=((0, 1), (1, 7), (1, 4))) == good
    assert L.pddc_morse_create(None, 0, nrx, W, B, None, None, None, None) == pkg.PDDC_EINVAL
    c = C.c_size_t()
    assert L.pddc_morse_set_rx(None, 0, 0, 1) == pkg.PDDC_EINVAL
    assert L.pddc_morse_process(None, None, 0, 0, None, 0, None, None, 0, None) == pkg.PDDC_EINVAL
    assert L.pddc_morse_max_chars(None, 10, C.byref(c)) == pkg.PDDC_EINVAL
    assert L.pddc_morse_read(None, None, None) == pkg.PDDC_EINVAL
    assert L.pddc_morse_reset(None) == pkg.PDDC_EINVAL
    assert L.pddc_morse_destroy(None) == pkg.PDDC_OK
    assert L.pddc_morse_tile_outputs() == pkg.morse_tile_outputs() == 256
    with pytest.raises(pkg.PddcError) as e:
        pkg.Morse([M.keyer(100.0, 20.0, 16)], [(0, 1)], 8)            # taps of another length than W
    assert e.value.code == pkg.PDDC_EINVAL
