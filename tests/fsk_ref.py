"""The FSK decoder's reference: numpy, DESIGN.md 8 / include/perseus_ddc.h "fsk" restated.  `FskRef` evaluates the
streaming definition in double, with f32=True the same operation order in float32 (fmaf as one rounding of the exact
double product plus the addend, double rounding aside, as in rxfilter_ref.py; the float32 division is numpy's, correctly
rounded).  The start-stop receiver goes sample by sample, all receivers side by side.  Never the code under test.

The GPU tolerance.  tests/test_fsk_cpu.py::test_float32_model_against_double measures the float32 model's d against the
double reference's on the GPU parity test's own inputs: case(W, 9) for every window of WINDOWS and case(W, 1024) for
those of BIG_WINDOWS (noisy two-tone text, 1264 samples at 16 samples per bit; W = 2: 400 samples at 4 per bit, nine
receivers at the most), every receiver of every case.  Worst |d_model - d_ref| per W over both inputs:
    1: 8.345e-08   2: 1.413e-07   16: 5.223e-07   255: 3.275e-06   256: 2.815e-06
TOL_FSK = 7 x the worst of them, the margin the tuner's, the demodulator's, the audio and the receiver filter tests use.
Never taken from k_fsk.

Decisions.  A receiver's characters, counts and status are compared exactly where the reference's margin holds: the
least |d| of the double reference over the samples with s > 0, the first behind zero history (m = 0, and the first after
RESTART or OFF -> ON) left out, is at least MARGIN = 100 TOL_FSK, so that an error
of TOL_FSK cannot turn a decision.  (Sample 0 of a boxcar pair sees one tap of equal magnitude in both filters: pm = ps in
any arithmetic, and the strict > reads mark.)  A two-tone signal passes d = 0 at every change of tone, where the window
holds as much of the one as of the other; what the sample next to that point reads is the noise's doing, so at a given
margin some receivers of a large set fall below it (test_gpu_fsk.py caps them at 10 % of 1024 and at none of the small
sets)."""
import numpy as np

ON, REVERSE, RESTART = 0x1, 0x2, 0x4
FRAMING = 0x1
IDLE, START, DATA, STOP = 0, 1, 2, 3
CHAR = np.dtype([("start", np.uint64), ("code", np.uint16), ("flags", np.uint16), ("quality", np.float32)])
STATUS = np.dtype([("chars", np.uint32), ("framing", np.uint32), ("false_starts", np.uint32), ("state", np.uint32),
                   ("d_last", np.float32)])

WINDOWS = (1, 2, 16, 255, 256)
BIG_WINDOWS = (1, 16, 255, 256)               # the windows of the 1024-receiver case (the series of W = 2 has nine rows)
MODEL_WORST = {1: 8.345e-08, 2: 1.413e-07, 16: 5.223e-07, 255: 3.275e-06, 256: 2.815e-06}
MODEL_WORST_FSK = max(MODEL_WORST.values())
TOL_FSK = 7 * MODEL_WORST_FSK
MARGIN = 100 * TOL_FSK
CUTS = [0, 1, 2, 30, 0, 31, 255, 256, 257, 1]                         # then the rest; the kernel's tile is 256


def cut_lists(n, TT):
    """the batch sizes every series of n samples is cut by, beside one batch: CUTS as far as it fits and the rest; batches
    that end on and beside the kernel's tile seams, with batches of 0 and 1 (TT - 1 | 1 | 1 | 0 | TT - 1 | TT | 2 | the
    rest, as far as it fits); forty batches of one sample and the rest"""
    def fit(sizes):
        out = []
        for b in sizes:
            if sum(out) + b >= n:
                break
            out.append(b)
        return out + [n - sum(out)]
    return [fit(CUTS), fit([TT - 1, 1, 1, 0, TT - 1, TT, 2]), fit([1] * 40)]


# ---- ITA2, restated ---------------------------------------------------------------------------------------------------

LTRS = ["\0", "E", "\n", "A", " ", "S", "I", "U", "\r", "D", "R", "J", "N", "F", "C", "K", "T", "Z", "L", "W", "H", "Y", "P",
        "Q", "O", "B", "G", None, "M", "X", "V", None]
FIGS = ["\0", "3", "\n", "-", " ", "'", "8", "7", "\r", "\x05", "4", "\a", ",", "!", ":", "(", "5", "+", ")", "2", "#", "6",
        "0", "1", "9", "?", "&", None, ".", "/", "=", None]
TO_FIGS, TO_LTRS = 27, 31
TEXT = "THE QUICK BROWN FOX JUMPS OVER THE LAZY DOG 0123456789"


def ita2_encode(text):
    """text -> 5-bit codes, starting in letters, a shift code wherever the table changes; characters of both tables
    (space, CR, LF, NUL) keep the table"""
    codes, figs = [], False
    for ch in text:
        if ch in (LTRS if not figs else FIGS):
            pass
        elif ch in (FIGS if not figs else LTRS):
            figs = not figs
            codes.append(TO_FIGS if figs else TO_LTRS)
        else:
            raise ValueError(ch)
        codes.append((FIGS if figs else LTRS).index(ch))
    return codes


def ita2_decode(codes, flags=None):
    """fsk_ita2 restated"""
    out, figs = [], False
    for i, c in enumerate(codes):
        if (flags is not None and int(flags[i]) & FRAMING) or int(c) > 31:
            out.append("\ufffd")
        elif c == TO_FIGS:
            figs = True
        elif c == TO_LTRS:
            figs = False
        else:
            out.append((FIGS if figs else LTRS)[int(c)])
    return "".join(out)


# ---- modems and signals -----------------------------------------------------------------------------------------------

def modem(rate, baud, mark, space, W, nbits=5):
    """fsk_modem restated: boxcars of min(W, round(rate / baud)) samples with sum 1 under exp(+2 pi i f t / rate), double,
    rounded once; inc = round(2^32 baud / rate)"""
    L = min(W, int(round(rate / baud)))
    t = np.arange(W, dtype=np.float64)
    w = (t < L) / float(L)
    return ((w * np.exp(2j * np.pi * mark * t / rate)).astype(np.complex64),
            (w * np.exp(2j * np.pi * space * t / rate)).astype(np.complex64), int(round(2.0 ** 32 * baud / rate)), nbits)


def keying(codes, nbits=5, sps=16, stop=1.5, lead=2.0, tail=2.0):
    """the line of start-stop characters, a value per sample, True = space: `lead` bits of mark, then per character a
    start element (space), nbits data elements, the first bit first (1 = mark), a stop element (mark) of `stop` bits;
    `tail` bits of mark behind the last"""
    line = [False] * int(round(lead * sps))
    for c in codes:
        line += [True] * sps
        for k in range(nbits):
            line += [not (c >> k) & 1] * sps
        line += [False] * int(round(stop * sps))
    return np.array(line + [False] * int(round(tail * sps)), bool)


def two_tone(line, mark, space, snr_db, seed, n=None):
    """a continuous-phase two-tone series of unit amplitude for the keying `line` (frequencies in cycles per sample; the
    phase moves by the frequency of the sample it arrives at), padded with mark to n samples, plus complex white noise
    snr_db below the tone (None: none), seeded -> complex64 [n]"""
    line = np.asarray(line, bool)
    if n is not None:
        assert n >= line.size
        line = np.concatenate([line, np.zeros(n - line.size, bool)])
    rng = np.random.default_rng(seed)
    ph = 2.0 * np.pi * (rng.uniform() + np.cumsum(np.where(line, space, mark)))
    z = np.exp(1j * ph)
    if snr_db is not None:
        sigma = 10.0 ** (-snr_db / 20.0) / np.sqrt(2.0)
        z = z + sigma * (rng.standard_normal(line.size) + 1j * rng.standard_normal(line.size))
    return z.astype(np.complex64)


SPS = 16
MARK, SPACE = 3.0 / 32.0, -3.0 / 32.0         # cycles per sample: a shift of 3 baud, 136 Hz at 45.45 baud
PARITY_N = 1264
PARITY_CHARS = 9                              # 2 + 9 x 7.5 + 2 bits = 1144 samples, mark behind them
FAST_N = 400                                  # the 4-samples-per-bit series: 2 + 9 x 10.5 + 2 bits = 394 samples
SMALL_SEEDS = (9000, 9100, 9201, 9301, 9400, 9502, 9612, 9705, 9802)
FAST_SEEDS = (400, 500, 600, 700, 800, 900, 1000, 1100, 1200)
REVERSE_SEEDS = (9900, 10000, 10100, 10200, 10300)


def parity_text(j):
    """receiver j's nine characters: a stretch of TEXT's codes, from another place for every receiver"""
    codes = ita2_encode(TEXT)
    return [codes[(5 * j + i) % len(codes)] for i in range(PARITY_CHARS)]


def fast_text(j):
    """receiver j's nine 8-bit characters"""
    return [(37 * j + 11 * i + 5) % 256 for i in range(PARITY_CHARS)]


_INPUTS = {}


def parity_inputs(nrx):
    """the GPU parity test's series at 16 samples per bit: receiver j keys parity_text(j), 1264 samples, tones at
    +-3/32 cycles per sample, noise 10 dB (nrx = 1024: 16 dB) below the tone; 1, 5 and 9 receivers are the first rows of
    one array, whose seeds are chosen so that every case leaves those receivers' margins above MARGIN
    (test_fsk_cpu.py asserts it)"""
    key = 1024 if nrx == 1024 else 9
    if key not in _INPUTS:
        snr, seeds = (16.0, range(50000, 51024)) if key == 1024 else (10.0, SMALL_SEEDS)
        _INPUTS[key] = np.stack([two_tone(keying(parity_text(j)), MARK, SPACE, snr, seeds[j], PARITY_N) for j in range(key)])
    return _INPUTS[key][:nrx]


def reverse_inputs(nrx):
    """the parity series with its tones exchanged (mark at -3/32, space at +3/32), for REVERSE receivers: up to five rows,
    noise 10 dB below the tone, seeds chosen like SMALL_SEEDS so that every margin holds (test_fsk_cpu.py asserts it)"""
    assert nrx <= len(REVERSE_SEEDS)
    return np.stack([two_tone(keying(parity_text(j)), SPACE, MARK, 10.0, REVERSE_SEEDS[j], PARITY_N) for j in range(nrx)])


def fast_inputs(nrx):
    """the series at 4 samples per bit, for inc = 2^30: receiver j keys the 8-bit characters fast_text(j), 400 samples,
    tones at +-1/4 cycles per sample, noise 20 dB below the tone"""
    assert nrx <= 9
    if "fast" not in _INPUTS:
        _INPUTS["fast"] = np.stack([two_tone(keying(fast_text(j), nbits=8, sps=4), 0.25, -0.25, 20.0, FAST_SEEDS[j], FAST_N)
                                    for j in range(9)])
    return _INPUTS["fast"][:nrx]


def tailed_modem(W, seed, inc=1 << 28, nbits=5):
    """the 16-sample boxcar pair of the parity tones in a window of W: behind the 16th tap every tap is a seeded
    complex value of modulus below 3e-3, so that every tap of a long window takes part in every output"""
    hm, hs, _, _ = modem(float(SPS), 1.0, MARK * SPS, SPACE * SPS, W)
    if W > SPS:
        t = np.random.default_rng(seed).uniform(-2e-3, 2e-3, (2, W - SPS, 2))
        hm[SPS:] = (t[0, :, 0] + 1j * t[0, :, 1]).astype(np.complex64)
        hs[SPS:] = (t[1, :, 0] + 1j * t[1, :, 1]).astype(np.complex64)
    return hm, hs, inc, nbits


def case(W, nrx):
    """The parity case of window W for nrx receivers -> (bank, sel, z):
      1    one tap, hm = [1], hs = [0.5]: d = 0.6 for every sample; the odd receivers are REVERSE, read space from sample
           0 on and report a break: one framing character, then nothing
      2    inc = 2^30 (4 samples per bit), nbits = 8: fast_inputs, the boxcar pair of two samples at +-1/4
      16   inc = 2^28, nbits = 5, one modem: parity_inputs, the boxcar pair of 16 samples
      255, 256   a bank of 16 tailed modems, receiver j on modem (7 j + 3) mod 16; the modems 12 .. 15 have inc = 1,
           the least there is: their receivers see the first edge and wait for a strobe that is 2^31 samples away"""
    if W == 1:
        one = np.ones(1, np.complex64)
        return [(one, 0.5 * one, 1 << 28, 5)], [(0, ON | (REVERSE if j & 1 else 0)) for j in range(nrx)], parity_inputs(nrx)
    if W == 2:
        return [modem(4.0, 1.0, 1.0, -1.0, 2, 8)], [(0, ON)] * nrx, fast_inputs(nrx)
    if W == 16:
        return [tailed_modem(16, 0)], [(0, ON)] * nrx, parity_inputs(nrx)
    bank = [tailed_modem(W, 100 * W + b, 1 if b >= 12 else 1 << 28) for b in range(16)]
    return bank, [((7 * j + 3) % 16, ON) for j in range(nrx)], parity_inputs(nrx)


def case_codes(W, j):
    """what receiver j of case(W, .) decodes where nothing goes wrong; None: no characters are expected to compare"""
    if W == 2:
        return fast_text(j)
    if W == 1 or (W > 16 and (7 * j + 3) % 16 >= 12):
        return None
    return parity_text(j)


# ---- the definition ---------------------------------------------------------------------------------------------------

def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


class FskRef:
    """The streaming definition: batches of [nrx, n] complex values.  bank: (hm, hs, inc, nbits) per modem, sel: (modem,
    flags) per receiver.  f32 False: double.  f32 True: the float32 model."""

    def __init__(self, bank, sel, W, f32=False):
        self.W, self.f32 = int(W), f32
        self.hm = np.stack([np.asarray(b[0], np.complex64).astype(np.complex128) for b in bank])
        self.hs = np.stack([np.asarray(b[1], np.complex64).astype(np.complex128) for b in bank])
        assert self.hm.shape == self.hs.shape == (len(bank), self.W)
        self.inc = np.array([int(b[2]) for b in bank], np.uint64)
        self.nbits = np.array([int(b[3]) for b in bank], np.int64)
        assert all(1 <= i <= 1 << 30 for i in self.inc) and all(5 <= b <= 8 for b in self.nbits)
        self.nrx = len(sel)
        self.modem = np.array([int(s[0]) for s in sel], np.int64)
        fl = np.array([int(s[1]) for s in sel], np.int64)
        assert ((0 <= self.modem) & (self.modem < len(bank))).all() and not (fl & ~(ON | REVERSE | RESTART)).any()
        self.on, self.rev = (fl & ON) != 0, (fl & REVERSE) != 0
        self.reset()

    def reset(self):
        K = self.nrx
        self.m = 0
        self.hist = np.zeros((K, self.W - 1), np.complex128)           # float32 values
        self.state = np.zeros(K, np.int64)
        self.prev = np.zeros(K, bool)
        self.acc = np.zeros(K, np.uint64)
        self.k = np.zeros(K, np.int64)
        self.shift = np.zeros(K, np.int64)
        self.qmin = np.zeros(K, np.float64)
        self.start = np.zeros(K, np.uint64)
        self.chars = np.zeros(K, np.int64)
        self.framing = np.zeros(K, np.int64)
        self.false_starts = np.zeros(K, np.int64)
        self.d_last = np.zeros(K, np.float64)
        self.first = np.ones(K, bool)                                  # the next sample is the first behind zero history

    def set_rx(self, rx, modem, flags):
        assert 0 <= rx < self.nrx and 0 <= modem < self.inc.size and not flags & ~(ON | REVERSE | RESTART)
        on = bool(flags & ON)
        if flags & RESTART or (on and not self.on[rx]):
            self.hist[rx] = 0.0
            self.state[rx], self.prev[rx], self.first[rx] = IDLE, False, True
        if modem != self.modem[rx]:
            self.state[rx] = IDLE
        self.modem[rx], self.on[rx], self.rev[rx] = modem, on, bool(flags & REVERSE)

    # -- discriminator: the rows of the ON receivers
    def _filter(self, h, zz, n):
        W = self.W
        if not self.f32:
            # out[r, m] = sum over i of h[r, W - 1 - i] zz[r, m + i]: one product of [n, W] by [W] per receiver
            if not n:
                return np.zeros((zz.shape[0], 0)), np.zeros((zz.shape[0], 0))
            win = np.lib.stride_tricks.sliding_window_view(zz, W, axis=1)
            out = np.matmul(win, h[:, ::-1, None])[..., 0]
            return out.real, out.imag
        # the float32 model: the accumulators hold float32 values in double; a block of rows at a time stays in the cache
        R = zz.shape[0]
        re, im = np.zeros((R, n), np.float32), np.zeros((R, n), np.float32)
        for r0 in range(0, R, 32):
            zr, zi = np.ascontiguousarray(zz[r0:r0 + 32].real), np.ascontiguousarray(zz[r0:r0 + 32].imag)
            hh = h[r0:r0 + 32]
            acc = [np.zeros((zr.shape[0], n)), np.zeros((zr.shape[0], n))]
            tmp, t32 = np.empty_like(acc[0]), np.empty((zr.shape[0], n), np.float32)

            def fma(c, x, k):                                         # acc[k] = float32(c x + acc[k]), rounded once
                np.multiply(c, x, out=tmp)
                np.add(tmp, acc[k], out=tmp)
                np.copyto(t32, tmp, casting="same_kind")
                np.copyto(acc[k], t32)

            for t in range(W):
                a, b = W - 1 - t, W - 1 - t + n
                hr, hi = hh[:, t:t + 1].real.copy(), hh[:, t:t + 1].imag.copy()
                fma(hr, zr[:, a:b], 0)
                fma(-hi, zi[:, a:b], 0)
                fma(hr, zi[:, a:b], 1)
                fma(hi, zr[:, a:b], 1)
            re[r0:r0 + 32], im[r0:r0 + 32] = acc[0], acc[1]
        return re, im

    def discriminate(self, z):
        """-> (space bool [nrx, n], d [nrx, n], s [nrx, n]); OFF rows: False, +0, 0, and nothing carried moves"""
        z = np.asarray(z).reshape(self.nrx, -1).astype(np.complex64).astype(np.complex128)
        n = z.shape[1]
        rows = np.flatnonzero(self.on)
        space = np.zeros((self.nrx, n), bool)
        d = np.zeros((self.nrx, n), np.float32 if self.f32 else np.float64)
        ssum = np.zeros((self.nrx, n), np.float64)
        if rows.size:
            zz = np.concatenate([self.hist[rows], z[rows]], axis=1)
            with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
                mr, mi = self._filter(self.hm[self.modem[rows]], zz, n)
                sr, si = self._filter(self.hs[self.modem[rows]], zz, n)
                if self.f32:
                    pm = _f32(mi.astype(np.float64) * mi + (mr * mr).astype(np.float64))
                    ps = _f32(si.astype(np.float64) * si + (sr * sr).astype(np.float64))
                else:
                    pm, ps = mi * mi + mr * mr, si * si + sr * sr
                rev = self.rev[rows][:, None]
                pm, ps = np.where(rev, ps, pm), np.where(rev, pm, ps)
                s = pm + ps
                pos = s > 0
                dd = np.where(pos, (pm - ps) / np.where(pos, s, 1), 0).astype(d.dtype)
            space[rows], d[rows], ssum[rows] = ps > pm, dd, s
            self.hist[rows] = zz[:, zz.shape[1] - (self.W - 1):]
        return space, d, ssum

    # -- the start-stop receiver, sample by sample
    def receive(self, space, d):
        """-> one CHAR array per receiver: the characters whose STOP strobe lies in these samples"""
        K, n = space.shape
        out = [[] for _ in range(K)]
        on = self.on.copy()
        inc, nbits = self.inc[self.modem], self.nbits[self.modem]
        q = np.abs(d.astype(np.float64))
        two32 = np.uint64(1 << 32)
        for i in range(n):
            sp, qi = space[:, i], q[:, i]
            idle = on & (self.state == IDLE)
            edge = idle & sp & ~self.prev
            run = on & ~idle
            a2 = (self.acc + inc) % two32
            strobe = run & (a2 < self.acc)
            self.acc = np.where(run, a2, self.acc)
            st = self.state
            s_start, s_data, s_stop = strobe & (st == START), strobe & (st == DATA), strobe & (st == STOP)
            go = s_start & sp
            bad = s_start & ~sp
            self.k = np.where(go, 0, self.k)
            self.shift = np.where(go, 0, self.shift)
            self.qmin = np.where(go, qi, self.qmin)
            self.false_starts += bad
            self.shift = np.where(s_data, self.shift | (np.where(sp, 0, 1) << self.k), self.shift)
            both = s_data | s_stop
            self.qmin = np.where(both, np.fmin(self.qmin, qi), self.qmin)
            self.k = self.k + s_data
            for j in np.flatnonzero(s_stop):
                out[j].append((self.start[j], self.shift[j], FRAMING if sp[j] else 0, self.qmin[j]))
            self.chars += s_stop
            self.framing += s_stop & sp
            new = np.where(go, DATA, st)
            new = np.where(bad | s_stop, IDLE, new)
            new = np.where(s_data & (self.k == nbits), STOP, new)
            new = np.where(edge, START, new)
            self.state = new
            self.acc = np.where(edge, np.uint64(1 << 31), self.acc)
            self.start = np.where(edge, np.uint64(self.m + i), self.start)
            self.prev = np.where(on, sp, self.prev)
        if n:
            self.d_last = np.where(on, d[:, n - 1].astype(np.float64), self.d_last)
        self.m += n
        return [np.array(c, CHAR) for c in out]

    def process(self, z):
        """-> (chars: a CHAR array per receiver, counts int64 [nrx], d [nrx, n], margin [nrx]: the least |d| over this
        batch's samples with s > 0, a receiver's first sample behind zero history left out (the tie of the header); inf
        where there is none)"""
        space, d, s = self.discriminate(z)
        look = s > 0
        if look.shape[1]:
            look[:, 0] &= ~self.first
            self.first &= ~self.on
        with np.errstate(invalid="ignore"):
            margin = np.where(look, np.abs(d.astype(np.float64)), np.inf).min(axis=1, initial=np.inf)
        chars = self.receive(space, d)
        return chars, np.array([c.size for c in chars], np.int64), d, margin

    def read(self):
        st = np.zeros(self.nrx, STATUS)
        st["chars"], st["framing"], st["false_starts"], st["state"] = self.chars, self.framing, self.false_starts, self.state
        st["d_last"] = self.d_last
        return st


def run_cuts(r, z, cuts=None, before=None):
    """all of z through r in the given batches (default: one); before(i, r) is called ahead of batch i -> (chars: a CHAR
    array per receiver, d [nrx, n], margin [nrx], status)"""
    z = np.asarray(z)
    parts, ds, margin, off = [[] for _ in range(r.nrx)], [], np.full(r.nrx, np.inf), 0
    for i, b in enumerate(cuts or [z.shape[1]]):
        if before:
            before(i, r)
        chars, _, d, mg = r.process(z[:, off:off + b])
        for j, c in enumerate(chars):
            parts[j].append(c)
        ds.append(d)
        margin = np.minimum(margin, mg)
        off += b
    assert off == z.shape[1]
    return [np.concatenate(p) for p in parts], np.concatenate(ds, axis=1), margin, r.read()


def stop_distance(inc, nbits):
    """samples from the edge to the STOP strobe, carry by carry from the definition: the accumulator starts at 2^31 on
    the edge's sample and the c-th carry comes with the first sample s behind it at which 2^31 + s inc >= c 2^32; the
    STOP strobe is carry nbits + 2.  Exact integers"""
    c = nbits + 2
    need = c * (1 << 32) - (1 << 31)
    return -(-need // inc)


def max_chars(bank, n):
    """pddc_fsk_max_chars restated: the most over the bank of n div P + 1"""
    return max(n // stop_distance(int(b[2]), int(b[3])) + 1 for b in bank)
