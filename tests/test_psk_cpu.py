"""The PSK decoder without a GPU: the numpy reference (tests/psk_ref.py) against itself and against the facts of the
radio it is for.  TOL_PSK and MARGIN are measured and asserted here, on the GPU tests' own inputs; the seeds of the small
sets and the noise level of the radio facts are checked on the reference alone.  Nothing here runs k_psk."""
import numpy as np

import psk_ref as P


def test_varicode_and_the_modem_helper(pkg):
    """The table: 128 codes, each beginning and ending with 1, none holding 00, no two alike; the issue's four; the
    package's table, its bit maker and its modem are the reference's; an unknown code gives U+FFFD."""
    assert len(P.VARICODE) == 128 and len(set(P.VARICODE)) == 128
    for b in P.VARICODE:
        assert b[0] == "1" and b[-1] == "1" and "00" not in b and len(b) <= 10
    for ch, b in ((" ", "1"), ("e", "11"), ("t", "101"), ("o", "111"), ("a", "1011"), ("\n", "11101"), ("E", "1110111")):
        assert P.VARICODE[ord(ch)] == b
    codes = [int(b, 2) for b in P.VARICODE]
    assert pkg.psk_varicode(codes) == "".join(chr(i) for i in range(128)) == P.decode(codes)
    assert pkg.psk_varicode([1, 3, 5, 7, 0b100, 0xFFFF]) == " eto\ufffd\ufffd"
    assert pkg.psk_varicode_bits(P.TEXT) == P.bits_of(P.TEXT)
    for W, sps in ((16, 16), (64, 16), (80, 40), (256, 256), (33, 8), (256, 1000.5)):
        a, b = pkg.psk_modem(W, sps), P.modem(W, sps)
        assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:], (W, sps)
        h, inc, q, step = a
        assert 1 <= inc <= 1 << 29 and 1 <= q <= 64 and 4 * q * inc <= 1 << 32 and step == inc // 4
        assert abs(float(h.astype(np.float64).sum()) - 1.0) < 1e-6 and (h >= 0).all()
    assert pkg.psk_modem(64, 16)[1:3] == (1 << 28, 4) and pkg.psk_modem(256, 256)[1:3] == (1 << 24, 64)
    assert pkg.psk_char_dtype() == P.CHAR and pkg.psk_status_dtype() == P.STATUS and pkg.psk_char_dtype().itemsize == 16


def test_float32_model_against_double():
    """The float32 model against the double reference on the GPU parity test's own inputs (psk_ref's header): the worst
    |d_model - d_ref| and |x_model - x_ref| per window is the figure written into MODEL_WORST, TOL_PSK is 7 x the
    largest, MARGIN 4 x that.  The same runs show what the GPU tests rely on: every receiver of the small sets keeps a
    margin of at least MARGIN, of the 1024 at most 10 % fall below it, and the model's strobes, characters and integer
    status are the reference's wherever the margin holds."""
    worst = {}
    for nrx in (9, 1024):
        for W in (P.WINDOWS if nrx == 9 else P.BIG_WINDOWS):
            bank, sel, z = P.case(W, nrx)
            assert 80 <= P.PARITY_SYMS <= 160
            chars, sym, margin, st, strobes = P.run_cuts(P.PskRef(bank, sel, W), z)
            m32 = P.run_cuts(P.PskRef(bank, sel, W, f32=True), z)
            below = int((margin < P.MARGIN).sum())
            print(f"nrx {nrx} W {W}: least margin {margin.min():.3e} (MARGIN {P.MARGIN:.3e}), {below} below")
            assert below == 0 if nrx == 9 else below <= nrx // 10, (nrx, W, below)
            for j in range(nrx):
                if margin[j] >= P.MARGIN:
                    assert m32[4][j] == strobes[j], (nrx, W, j)
                    for k in ("start", "code", "nbits", "flags"):
                        assert np.array_equal(m32[0][j][k], chars[j][k]), (nrx, W, j, k)
                    assert all(m32[3][k][j] == st[k][j] for k in ("chars", "symbols", "acc", "reg"))
                if m32[4][j] == strobes[j] and sym[j].size:
                    worst[W] = max(worst.get(W, 0.0), float(np.abs(m32[1][j] - sym[j]).max()))
            assert sum(s.shape[0] > 70 for s in sym) == nrx
    for k, v in worst.items():
        print(f"W = {k}: worst |(d, x)_model32 - (d, x)_ref| {v:.3e} (written {P.MODEL_WORST[k]:.3e})")
        assert abs(v - P.MODEL_WORST[k]) <= 0.0005 * P.MODEL_WORST[k] + 1e-12, k
    assert P.MODEL_WORST_PSK == max(P.MODEL_WORST.values())
    assert P.TOL_PSK == 7 * P.MODEL_WORST_PSK and P.MARGIN >= 4 * P.TOL_PSK


def test_margins_of_the_other_gpu_cases():
    """The cases of tests/test_gpu_psk.py that compare every receiver, run on the reference alone: the slowest modem, the
    tile seam lengths, the control case with its changes.  Every receiver keeps MARGIN, and the control case does what its
    text says: RESTART and the modem change fall into a character and lose it."""
    import test_gpu_psk as G
    bank, sel, z = P.slow_case()
    c, s, margin, st, sb = P.run_cuts(P.PskRef(bank, sel, 256), z)
    assert (margin >= P.MARGIN).all() and (st["symbols"] == P.SLOW_SYMS + 2).all(), margin
    bank, sel, z = P.case(16, 5)
    for n in (255, 256, 257, 513):
        assert (P.run_cuts(P.PskRef(bank, sel, 16), z[:, :n])[2] >= P.MARGIN).all(), n
    bank, sel, z, changes = G.control_case()
    a, b, _ = G.CONTROL_CUTS
    chars, sym, margin, st, sb = P.run_cuts(P.PskRef(bank, sel, 16), z, G.CONTROL_CUTS, before=changes(1, 2))
    print("control margins", margin)
    assert (margin >= P.MARGIN).all(), margin
    full = P.run_cuts(P.PskRef([bank[0]], [(0, P.ON)] * 7, 16), np.nan_to_num(z))[0]
    for j, cut in ((3, a), (4, a + b)):
        inside = [(int(r["start"]), int(sb_end)) for r, sb_end in zip(full[j], full[j]["start"] + 16 * (full[j]["nbits"].astype(np.int64) + 2))]
        assert any(s0 < cut < s1 for s0, s1 in inside), (j, cut, inside)       # the change falls into a character
        assert P.decode(chars[j]) != P.decode(full[j]) and len(chars[j]) == st["chars"][j] and st["symbols"][j] >= st["symbols"][0] - 1
    assert P.decode(chars[0]).endswith(P.PARITY_TEXTS[0]) and chars[1].size == 0 and st["symbols"][1] == 0


def test_capacity_bounds_on_the_reference():
    """Strobes and characters never exceed pddc_psk_max_syms and pddc_psk_max_chars, over every window of the parity
    series and the radio series; with step = inc and an input that advances the clock at every reversal
    (psk_ref.advancing_case) they reach them within 1: strobes D = 7 samples apart for 1200 samples, and with the bits
    1 0 0 over and over a character every 7 + 7 + 8 samples, within 1 of (max_syms - 1) div 3 + 1 for 100 samples (a 1
    is not a reversal and corrects nothing, so the three strobes of a character span 22 samples, not 21: the bound,
    which is host arithmetic over D alone, moves ahead by one every 21 characters)."""
    # the derived distance against the issue's: never below, above where inc divides 2^32
    for inc, step in ((1 << 29, 1 << 29), (1 << 28, 1 << 26), (268425483, 268425483), (1 << 24, 0), (300000000, 5)):
        issue = -(-(1 << 32) // inc) - 2
        assert P.distance([(None, inc, 1, step)]) >= issue, (inc, step)
    assert P.distance([(None, 1 << 29, 1, 1 << 29)]) == 7 and P.distance([(None, 1 << 29, 1, 0)]) == 8
    for W in (2, 256):
        bank, sel, z = P.case(W, 9)
        chars, sym, margin, st, strobes = P.run_cuts(P.PskRef(bank, sel, W), z)
        D = P.distance(bank)
        for j in range(9):
            m = np.array(strobes[j])
            assert (np.diff(m) >= D).all()
            for n in (1, D, D + 1, 100, 977):
                most = max(np.searchsorted(m, m + n, "left") - np.arange(m.size))
                assert most <= P.max_syms(bank, n), (W, j, n)
    bank, sel, z, D, first = P.advancing_case()
    n = z.shape[1]
    chars, sym, margin, st, strobes = P.run_cuts(P.PskRef(bank, sel, 1), z)
    assert (np.diff(strobes[0]) == D).all() and strobes[0][0] == first and margin[0] > 0.1
    assert P.max_syms(bank, n) - 1 <= len(strobes[0]) <= P.max_syms(bank, n)
    tail = [m for m in strobes[0] if m >= first]
    assert len(tail) == P.max_syms(bank, n - first)                   # a batch that begins on a strobe holds the bound
    bank, sel, z, D, first = P.advancing_case(bits=[1, 0, 0], n=100)
    chars, sym, margin, st, strobes = P.run_cuts(P.PskRef(bank, sel, 1), z)
    assert (chars[0]["code"] == 1).all() and (chars[0]["nbits"] == 1).all() and (np.diff(chars[0]["start"].astype(np.int64)) == 22).all()
    assert P.max_chars(bank, 100) - 1 <= len(chars[0]) <= P.max_chars(bank, 100), (len(chars[0]), P.max_chars(bank, 100))


def test_radio_facts():
    """"CQ CQ DE TEST TEST pse k" behind 64 idle reversals, raised-cosine keying, at 16 and 40 samples per symbol, the
    clock 200 ppm off either way, each of 8 starting phases, 20 seeds: at NOISE_DB = 18 dB (noise power in the sample
    rate's bandwidth below the carrier, that is 30 dB and 34 dB below it in a bandwidth of one baud) every one of the 640
    receivers reads the text from the second word on; at 17 dB one does not -- 18 dB is the highest noise level, in whole
    dB, at which the bar holds.  With step = 0 a receiver half a symbol off reads nothing of it.  A carrier 2 Hz off at
    31.25 baud still reads at that noise level (20 seeds over the 8 phases), and the angle of the mean of (d + j x)^2 gives twice the offset's phase per symbol: every
    seed's estimate lies within six standard deviations of the 20 estimates from the truth."""
    bank, sel, z = P.radio_case(P.NOISE_DB)
    assert len(sel) == 640 and P.NOISE_DB == 18.0
    chars = P.run_cuts(P.PskRef(bank, sel, P.RADIO_W), z)[0]
    assert P.radio_read(chars) == 640, [j for j, c in enumerate(chars) if P.RADIO_WANT not in P.decode(c)]
    bank, sel, z = P.radio_case(P.NOISE_DB - 1.0)
    assert P.radio_read(P.run_cuts(P.PskRef(bank, sel, P.RADIO_W), z)[0]) < 640
    # a fixed clock: the strobe's on-time sample lies 4.5 + 16 phase samples from the symbol's middle (mod 16)
    bits = [0] * 64 + P.bits_of(P.TEXT) + [0] * 4
    h, inc, q, _ = P.modem(P.RADIO_W, 16)
    zz = np.stack([P.bpsk(bits, 16, lead=16, snr_db=40.0, seed=s, phase=3.5 / 16) for s in range(4)])
    off = P.run_cuts(P.PskRef([(h, inc, q, 0)], [(0, P.ON)] * 4, P.RADIO_W), zz)[0]
    on = P.run_cuts(P.PskRef([(h, inc, q, inc // 4)], [(0, P.ON)] * 4, P.RADIO_W), zz)[0]
    assert all("TEST" not in P.decode(c) for c in off) and all(P.RADIO_WANT in P.decode(c) for c in on)
    # 2 Hz at 31.25 baud
    theta = 2.0 * np.pi * 2.0 / 31.25
    zz = np.stack([P.bpsk(bits, 16, lead=16, snr_db=P.NOISE_DB, seed=500 + s, freq=2.0 / (31.25 * 16), phase=(s % 8) / 8.0) for s in range(20)])
    chars, sym = P.run_cuts(P.PskRef([P.modem(P.RADIO_W, 16)], [(0, P.ON)] * 20, P.RADIO_W), zz)[:2]
    assert all(P.RADIO_WANT in P.decode(c) for c in chars)
    est = np.array([0.5 * np.angle(np.mean((s[70:, 0] + 1j * s[70:, 1]) ** 2)) for s in sym])
    print("offset estimates", est, "truth", theta, "std", est.std())
    assert np.abs(est - theta).max() <= 6.0 * est.std() and est.std() < 0.05 * theta
