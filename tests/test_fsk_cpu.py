"""The FSK decoder without a GPU: the numpy reference (tests/fsk_ref.py) decodes its own signal, is independent of the cut,
its float32 model gives the GPU tolerance, the capacity bound holds on back-to-back characters, the helpers match their
restatements, and argument errors are reported as such with or without a device."""
import ctypes as C

import numpy as np
import pytest

import fsk_ref as F


def test_reference_decodes_the_quick_brown_fox(pkg):
    """TEXT -> ITA2 codes with their shifts -> a continuous-phase two-tone series at 16 samples per bit with noise 10 dB
    below the tone -> FskRef with the boxcar pair of fsk_modem -> fsk_ita2: the same text, no framing error, no false
    start; the restated decoder agrees."""
    codes = F.ita2_encode(F.TEXT)
    z = F.two_tone(F.keying(codes), F.MARK, F.SPACE, 10.0, 2024)[None]
    hm, hs, inc, nbits = pkg.fsk_modem(16 * 45.45, 45.45, F.MARK * 16 * 45.45, F.SPACE * 16 * 45.45, 16)
    assert inc == 1 << 28 and nbits == 5
    chars, d, margin, st = F.run_cuts(F.FskRef([(hm, hs, inc, nbits)], [(0, F.ON)], 16), z)
    c = chars[0]
    assert list(c["code"]) == codes and not c["flags"].any()
    assert pkg.fsk_ita2(c["code"], c["flags"]) == F.TEXT == F.ita2_decode(c["code"], c["flags"])
    assert (st["chars"], st["framing"], st["false_starts"], st["state"]) == (len(codes), 0, 0, F.IDLE)
    # a character is 7.5 bits of 16 samples; the noise moves an edge by a sample at the most
    assert c["quality"].min() > 0.1 and np.all(np.abs(c["start"].astype(np.int64) - (39 + 120 * np.arange(c.size))) <= 1)
    # the inverted signal reads the same through REVERSE
    zi = F.two_tone(F.keying(codes), F.SPACE, F.MARK, 10.0, 2024)[None]
    ci = F.run_cuts(F.FskRef([(hm, hs, inc, nbits)], [(0, F.ON | F.REVERSE)], 16), zi)[0][0]
    assert list(ci["code"]) == codes and not ci["flags"].any()


@pytest.mark.parametrize("W", [2, 16, 256])
def test_reference_is_cut_independent(W):
    """5 receivers of the parity case, one batch against every cut list (batches of 0 and 1, seams of 256): the float32
    model's d, characters and status by their bits; the double reference's characters and status equal, its d within
    1e-14 (its filter is a matrix product, whose summation order numpy does not pin)."""
    bank, sel, z = F.case(W, 5)
    for f32 in (True, False):
        one = F.run_cuts(F.FskRef(bank, sel, W, f32=f32), z)
        for cuts in F.cut_lists(z.shape[1], 256):
            assert sum(cuts) == z.shape[1] and 1 in cuts
            got = F.run_cuts(F.FskRef(bank, sel, W, f32=f32), z, cuts)
            for a, b in zip(got[0], one[0]):
                if f32:
                    assert a.tobytes() == b.tobytes()
                else:
                    assert all(np.array_equal(a[k], b[k]) for k in ("start", "code", "flags"))
                    assert np.allclose(a["quality"], b["quality"], rtol=0, atol=1e-6)
            if f32:
                assert got[1].tobytes() == one[1].tobytes() and got[3].tobytes() == one[3].tobytes()
            else:
                assert np.abs(got[1] - one[1]).max() <= 1e-14
                assert all(np.array_equal(got[3][k], one[3][k]) for k in ("chars", "framing", "false_starts", "state"))


def test_float32_model_against_double():
    """The float32 model against the double reference on the GPU parity test's own inputs, every receiver of every case
    (fsk_ref's header): the worst
    |d_model - d_ref| per window is the figure written into MODEL_WORST, TOL_FSK is 7 x the largest.  The same runs show
    what the GPU test relies on: every receiver of the small sets decodes its text with a margin of at least MARGIN;
    of the 1024 at most 10 % fall below it, and all of them decode."""
    worst = {}
    for nrx in (9, 1024):
        for W in (F.WINDOWS if nrx == 9 else F.BIG_WINDOWS):
            bank, sel, z = F.case(W, nrx)
            chars, d, margin, st = F.run_cuts(F.FskRef(bank, sel, W), z)
            d32 = F.run_cuts(F.FskRef(bank, sel, W, f32=True), z)[1]
            worst[W] = max(worst.get(W, 0.0), float(np.abs(d32.astype(np.float64) - d).max()))
            below = int((margin < F.MARGIN).sum())
            print(f"nrx {nrx} W {W}: least margin {margin.min():.3e} (MARGIN {F.MARGIN:.3e}), {below} below")
            assert below == 0 if nrx == 9 else below <= nrx // 10, (nrx, W, below)
            for j, c in enumerate(chars):
                want = F.case_codes(W, j)
                if want is not None:
                    assert list(c["code"]) == want and not c["flags"].any(), (nrx, W, j)
            if W == 1:                                                # the odd receivers read a break
                assert all(c.size == (j & 1) and (not c.size or c["flags"][0] == F.FRAMING) for j, c in enumerate(chars))
            if W > 16:                                                # inc = 1: the edge, and no strobe in this life
                slow = [j for j in range(nrx) if (7 * j + 3) % 16 >= 12]
                assert all(chars[j].size == 0 and st["state"][j] == F.START for j in slow)
    # the reversed series of test_gpu_fsk.py::test_reverse: every margin holds, every receiver reads its text
    chars, _, margin, _ = F.run_cuts(F.FskRef([F.tailed_modem(16, 0)], [(0, F.ON | F.REVERSE)] * 5, 16), F.reverse_inputs(5))
    assert (margin >= F.MARGIN).all(), margin
    assert all(list(c["code"]) == F.parity_text(j) and not c["flags"].any() for j, c in enumerate(chars))
    for k, v in worst.items():
        print(f"W = {k}: worst |d_model32 - d_ref| {v:.3e} (written {F.MODEL_WORST[k]:.3e})")
        assert abs(v - F.MODEL_WORST[k]) <= 0.0005 * F.MODEL_WORST[k] + 1e-12, k
    assert F.MODEL_WORST_FSK == max(F.MODEL_WORST.values())
    assert F.TOL_FSK == 7 * F.MODEL_WORST_FSK and F.MARGIN == 100 * F.TOL_FSK


@pytest.mark.parametrize("nbits", [5, 8])
@pytest.mark.parametrize("inc", [1 << 30, 1 << 24])
def test_max_chars_on_back_to_back_characters(inc, nbits):
    """The closest the definition lets characters follow each other: P samples of space from the edge on (the start
    element and nbits zeros), one sample of mark under the STOP strobe, the next edge on the sample behind it, P =
    stop_distance.  The reference's start-stop receiver, given these decisions, ends a character every P + 1 samples; for
    every length n no batch of n samples of that series holds more STOP strobes than max_chars(n), and the batch that
    begins on one reaches it within 1.  inc = 2^30 is the largest there is;
    2^24 (256 samples per bit) is the smallest a sample-by-sample reference runs in a test's time: for inc = 1, the
    least there is, the next test checks the bound's arithmetic in exact integers."""
    P = F.stop_distance(inc, nbits)
    assert P == -(-(2 * nbits + 3) * (1 << 31) // inc)
    reps = 12
    space = np.tile(np.r_[np.ones(P, bool), np.zeros(1, bool)], reps)[None]
    bank = [(np.ones(1, np.complex64), np.ones(1, np.complex64), inc, nbits)]
    r = F.FskRef(bank, [(0, F.ON)], 1)
    chars = r.receive(space, np.where(space, -1.0, 1.0))[0]
    assert chars.size == reps and not chars["code"].any() and not chars["flags"].any()
    ends = chars["start"].astype(np.int64) + P                        # the samples of the STOP strobes
    assert np.array_equal(ends, P + (P + 1) * np.arange(reps))
    # a batch is any n samples of the series: it holds the most STOP strobes when it begins on one
    for n in range(0, space.shape[1] - P, 1 if P < 100 else 97):
        bound = F.max_chars(bank, n)
        for a in (0, 1, P // 2, P - 1, P, P + 1):
            got = int(((ends >= a) & (ends < a + n)).sum())
            assert got <= bound, (n, a, got, bound)
        assert int(((ends >= P) & (ends < P + n)).sum()) >= bound - 1, (n, bound)


def test_max_chars_arithmetic_at_the_bounds():
    """stop_distance against the accumulator of the definition run carry by carry, at inc = 1, 2^30 and values between
    that divide nothing; max_chars takes the bank's most."""
    for inc in (1, 3, 12345, (1 << 28) + 1, (1 << 30) - 1, 1 << 30):
        for nbits in (5, 8):
            acc, s = 1 << 31, 0
            for _ in range(nbits + 2):
                step = -(-((1 << 32) - acc) // inc)                   # samples to the next carry
                s, acc = s + step, (acc + step * inc) - (1 << 32)
                assert 0 <= acc < inc
            assert s == F.stop_distance(inc, nbits), (inc, nbits)
    assert F.stop_distance(1, 5) == 13 << 31 and F.stop_distance(1 << 30, 8) == 38
    one = np.ones(1, np.complex64)
    assert F.max_chars([(one, one, 1, 5), (one, one, 1 << 30, 8), (one, one, 1 << 30, 5)], 1264) == 1264 // 26 + 1
    assert F.max_chars([(one, one, 1, 5)], 1 << 40) == (1 << 40) // (13 << 31) + 1 == 40


def test_helpers_against_restatements(pkg):
    """fsk_modem against fsk_ref.modem (taps by their bits), fsk_ita2 against ita2_decode on every code in both tables
    with and without framing flags, the two dtypes against the reference's."""
    for rate, baud, mark, space, W, nbits in ((727.2, 45.45, 85.0, -85.0, 16, 5), (8000.0, 50.0, 1275.0, 1445.0, 256, 5),
                                              (1200.0, 75.0, 425.0, -425.0, 9, 7), (4.0, 1.0, 1.0, -1.0, 2, 8)):
        got, want = pkg.fsk_modem(rate, baud, mark, space, W, nbits), F.modem(rate, baud, mark, space, W, nbits)
        assert got[0].dtype == np.complex64 and got[0].shape == (W,)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2:] == want[2:]
        L = min(W, int(round(rate / baud)))
        assert abs(np.abs(got[0]).sum() - 1.0) < 1e-6 and not got[0][L:].any()
    assert pkg.fsk_modem(727.2, 45.45, 85.0, -85.0, 16)[2] == 1 << 28
    with pytest.raises(pkg.PddcError):
        pkg.fsk_modem(0.0, 45.45, 85.0, -85.0, 16)
    rng = np.random.default_rng(5)
    codes = np.r_[np.arange(32), 27, np.arange(32), 31, rng.integers(0, 32, 200), 32, 255]
    flags = (rng.uniform(size=codes.size) < 0.1).astype(np.uint16)
    assert pkg.fsk_ita2(codes) == F.ita2_decode(codes)
    assert pkg.fsk_ita2(codes, flags) == F.ita2_decode(codes, flags)
    assert pkg.fsk_ita2(F.ita2_encode("RYRY 73, DE K1ABC")) == "RYRY 73, DE K1ABC"
    assert pkg.fsk_ita2([20, 1, 40], [0, pkg.PDDC_FSK_FRAMING, 0]) == "H\ufffd\ufffd"
    assert pkg.fsk_char_dtype() == F.CHAR and F.CHAR.itemsize == 16 and pkg.fsk_status_dtype() == F.STATUS
    assert (pkg.PDDC_FSK_ON, pkg.PDDC_FSK_REVERSE, pkg.PDDC_FSK_RESTART, pkg.PDDC_FSK_FRAMING) == (F.ON, F.REVERSE, F.RESTART, F.FRAMING)
    assert (pkg.PDDC_FSK_IDLE, pkg.PDDC_FSK_START, pkg.PDDC_FSK_DATA, pkg.PDDC_FSK_STOP) == (F.IDLE, F.START, F.DATA, F.STOP)


def test_argument_errors_without_a_device(pkg):
    """Create refuses non-finite taps, inc and nbits out of range, a bad modem index, unknown flag bits, sizes out of range
    and NULLs with PDDC_EINVAL before it asks for a device; good arguments without a device are PDDC_ENODEV.  set_rx,
    process, max_chars, read, reset on a NULL handle are PDDC_EINVAL."""
    L = pkg.ddc_lib()
    W, B, nrx = 16, 2, 3

    def create(nrx=nrx, W=W, B=B, taps=None, inc=(1 << 28, 1 << 30), nbits=(5, 8), rx=((0, 1), (1, 3), (1, 0)), null=None):
        t = np.full((B, 2, W, 2), 0.25, np.float32) if taps is None else taps
        i, b = np.array(inc, np.uint32), np.array(nbits, np.int32)
        arr = (pkg.FskRx * len(rx))(*[pkg.FskRx(m, f) for m, f in rx])
        args = [t.ctypes.data_as(C.POINTER(C.c_float)), i.ctypes.data_as(C.POINTER(C.c_uint32)),
                b.ctypes.data_as(C.POINTER(C.c_int)), arr]
        if null is not None:
            args[null] = None
        h = C.c_void_p()
        rc = L.pddc_fsk_create(C.byref(h), 0, nrx, W, B, *args)
        if rc == pkg.PDDC_OK:
            L.pddc_fsk_destroy(h)
        return rc

    good = pkg.PDDC_OK if L.pddc_device_count() > 0 else pkg.PDDC_ENODEV
    assert create() == good
    for bad in (np.nan, np.inf, -np.inf):
        t = np.full((B, 2, W, 2), 0.25, np.float32)
        t[1, 1, W - 1, 1] = bad
        assert create(taps=t) == pkg.PDDC_EINVAL
    for kw in (dict(inc=(0, 1 << 30)), dict(inc=(1 << 28, (1 << 30) + 1)), dict(nbits=(4, 8)), dict(nbits=(5, 9)),
               dict(rx=((0, 1), (2, 1), (0, 1))), dict(rx=((0, 1), (-1, 1), (0, 1))), dict(rx=((0, 1), (1, 8), (0, 1))),
               dict(rx=((0, 1), (1, 0x100), (0, 1))), dict(nrx=0), dict(nrx=1025), dict(W=0), dict(W=257), dict(B=0), dict(B=17),
               dict(null=0), dict(null=1), dict(null=2), dict(null=3)):
        assert create(**kw) == pkg.PDDC_EINVAL, kw
    assert create(inc=(1, 1 << 30), rx=((0, 1), (1, 7), (1, 4))) == good   # the bounds themselves, RESTART at create
    assert L.pddc_fsk_create(None, 0, nrx, W, B, None, None, None, None) == pkg.PDDC_EINVAL
    c = C.c_size_t()
    assert L.pddc_fsk_set_rx(None, 0, 0, 1) == pkg.PDDC_EINVAL
    assert L.pddc_fsk_process(None, None, 0, 0, None, 0, None, None, 0, None) == pkg.PDDC_EINVAL
    assert L.pddc_fsk_max_chars(None, 10, C.byref(c)) == pkg.PDDC_EINVAL
    assert L.pddc_fsk_read(None, None, None) == pkg.PDDC_EINVAL
    assert L.pddc_fsk_reset(None) == pkg.PDDC_EINVAL
    assert L.pddc_fsk_destroy(None) == pkg.PDDC_OK
    assert L.pddc_fsk_tile_outputs() == pkg.fsk_tile_outputs() == 256
    with pytest.raises(pkg.PddcError) as e:
        pkg.Fsk([F.modem(16.0, 1.0, 1.0, -1.0, 16)], [(0, 1)], 8)      # taps of another length than W
    assert e.value.code == pkg.PDDC_EINVAL
