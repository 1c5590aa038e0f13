"""The Morse decoder's reference: numpy, DESIGN.md 8 / include/perseus_ddc.h "morse" restated.  `MorseRef` evaluates the
streaming definition in double, with f32=True the same operation order in float32 (fmaf as one rounding of the exact
double product plus the addend, double rounding aside, as in fsk_ref.py and rxfilter_ref.py).  The meter, the key and the
element timing go sample by sample, all receivers side by side; the timing is in exact integers.  Never the code under
test.

The GPU tolerance.  tests/test_morse_cpu.py::test_float32_model_against_double measures the float32 model's p against
the double reference's on the GPU parity test's own inputs: case(W, 9) and case(W, 1024) for
every window of WINDOWS, every receiver of every case.  The figure is |p_model - p_ref| / peak, peak the largest p of the
receiver's row in the double reference (what the meter's pk holds while the key is down).  Worst per W over both inputs:
    1: 1.055e-07   2: 2.212e-07   16: 8.842e-07   255: 4.051e-06   256: 4.014e-06
TOL_MORSE = 7 x the worst of them, the margin the fsk, tuner, demodulator, audio and receiver filter tests use.  Never
taken from k_morse.

Decisions.  A receiver's characters, counts and integer status are compared exactly where the reference's margin holds:
the least distance, over the receiver's peak, of any p from the threshold it was compared with (`on` while the key is
up, `off` while it is down; samples whose thresholds are +inf compare with nothing) and of pk from ratio fl at a block's
end is at least MARGIN = 100 TOL_MORSE, so that an error of TOL_MORSE in p, pk, fl and the thresholds cannot turn a
decision.  An envelope passes its thresholds at every edge, and how near the sample next to the crossing comes is the
noise's doing, so at a given margin some receivers of a large set fall below it (test_gpu_morse.py caps them at 10 % of
1024 and at none of the small sets, whose seeds were chosen on the reference alone)."""
import numpy as np

ON, FIXED, RESTART = 0x1, 0x2, 0x4
WORD, LONG = 0x1, 0x2
CHAR = np.dtype([("start", np.uint64), ("code", np.uint16), ("nel", np.uint8), ("flags", np.uint8), ("two", np.uint32)])
STATUS = np.dtype([("chars", np.uint32), ("marks", np.uint32), ("two", np.uint32), ("nel", np.uint32), ("key", np.uint32),
                   ("pk", np.float32), ("fl", np.float32)])
PARAMS = dict(a_on=0.5, a_off=0.3, rel=1.0 / 16, relf=1.0 / 64, ratio=4.0)      # the defaults of Morse
# The parameters of every case(): the parity series key on whole samples, so behind the Hann window of 8 samples an edge
# passes the same places every time -- the squares of the window's running sum, 0.0007, 0.014, 0.081, 0.25, 0.51, 0.78,
# 0.95, 1 of the peak.  a_on = 0.5 would sit on 0.51 and leave every receiver's margin to the noise; 0.375 lies midway
# between 0.25 and 0.51, a_off = 0.16 midway between 0.081 and 0.25.
CASE_PARAMS = dict(a_on=0.375, a_off=0.16, rel=1.0 / 8, relf=1.0 / 32, ratio=3.0)

WINDOWS = (1, 2, 16, 255, 256)
MODEL_WORST = {1: 1.055e-07, 2: 2.212e-07, 16: 8.842e-07, 255: 4.051e-06, 256: 4.014e-06}
MODEL_WORST_MORSE = max(MODEL_WORST.values())
TOL_MORSE = 7 * MODEL_WORST_MORSE
MARGIN = 100 * TOL_MORSE
CUTS = [0, 1, 2, 30, 0, 31, 63, 64, 65, 1]                            # then the rest; the meter's block is 64


def cut_lists(n, TT):
    """the batch sizes every series of n samples is cut by, beside one batch: CUTS as far as it fits and the rest (batches
    of 0 and 1, cuts at 63, 64 and 65 from where they begin); batches that end on and beside the kernel's tile seams
    (TT - 1 | 1 | 1 | 0 | TT - 1 | TT | 2 | the rest: ends at TT - 1, TT, TT + 1 = 255, 256, 257); forty batches of one
    sample and the rest; and 63 | 1 | 1 | the rest, whose batches end at m = 63, 64 and 65, on and beside the end of the
    meter's first block (blocks are absolute in m, so it is where a batch ends that counts, not how long it is)"""
    def fit(sizes):
        out = []
        for b in sizes:
            if sum(out) + b >= n:
                break
            out.append(b)
        return out + [n - sum(out)]
    return [fit(CUTS), fit([TT - 1, 1, 1, 0, TT - 1, TT, 2]), fit([1] * 40), fit([63, 1, 1])]


# ---- the ITU table, restated ------------------------------------------------------------------------------------------

ITU = {"A": ".-", "B": "-...", "C": "-.-.", "D": "-..", "E": ".", "F": "..-.", "G": "--.", "H": "....", "I": "..", "J": ".---",
       "K": "-.-", "L": ".-..", "M": "--", "N": "-.", "O": "---", "P": ".--.", "Q": "--.-", "R": ".-.", "S": "...", "T": "-",
       "U": "..-", "V": "...-", "W": ".--", "X": "-..-", "Y": "-.--", "Z": "--..", "0": "-----", "1": ".----", "2": "..---",
       "3": "...--", "4": "....-", "5": ".....", "6": "-....", "7": "--...", "8": "---..", "9": "----.", ".": ".-.-.-",
       ",": "--..--", ":": "---...", "?": "..--..", "'": ".----.", "-": "-....-", "/": "-..-.", "(": "-.--.", ")": "-.--.-",
       '"': ".-..-.", "=": "-...-", "+": ".-.-.", "@": ".--.-.", "É": "..-.."}
TEXT = "VVV THE QUICK BROWN FOX 73"


def code_of(ch):
    """the record's code of a character: 1, then an element per bit, dash = 1"""
    return int("1" + ITU[ch].replace(".", "0").replace("-", "1"), 2)


def decode(records):
    """morse_text restated"""
    back = {code_of(ch): ch for ch in ITU}
    out = []
    for i, c in enumerate(records):
        if int(c["flags"]) & WORD and i:
            out.append(" ")
        out.append("?" if int(c["flags"]) & LONG else back.get(int(c["code"]), "?"))
    return "".join(out)


def keyer(rate, wpm, W, wpm_min=5, wpm_max=60, shift=2):
    """morse_keyer restated"""
    L = min(W, max(1, int(round(0.6 * rate / wpm))))
    t = np.arange(W, dtype=np.float64)
    w = np.where(t < L, 1.0 - np.cos(2.0 * np.pi * (t + 1.0) / (L + 1.0)), 0.0)
    two = [min(max(int(round(256.0 * 2.4 * rate / float(v))), 512), 1 << 28) for v in (wpm, wpm_max, wpm_min)]
    return (w / w.sum()).astype(np.float32), min(max(two[0], two[1]), two[2]), two[1], two[2], int(shift)


# ---- signals ----------------------------------------------------------------------------------------------------------

def keying(text, spd, lead=0, tail=0):
    """the key line of `text`, a value per sample, True = key down: a dot is spd samples, a dash 3 spd, the gap between
    elements spd, between characters 3 spd, between words 7 spd; `lead` and `tail` samples of key up around it"""
    line = [False] * lead
    words = text.split(" ")
    for wi, word in enumerate(words):
        for ci, ch in enumerate(word):
            for ei, el in enumerate(ITU[ch]):
                line += [True] * (spd if el == "." else 3 * spd)
                if ei + 1 < len(ITU[ch]):
                    line += [False] * spd
            if ci + 1 < len(word):
                line += [False] * 3 * spd
        if wi + 1 < len(words):
            line += [False] * 7 * spd
    return np.array(line + [False] * tail, bool)


def keyed_carrier(line, snr_db, seed, n=None, freq=0.0):
    """a carrier of unit amplitude, `freq` cycles per sample off the receiver's centre and of a seeded phase, keyed by
    `line` and padded with key up to n samples, plus complex white noise snr_db below the carrier (None: none) ->
    complex64 [n]"""
    line = np.asarray(line, bool)
    if n is not None:
        assert n >= line.size, (n, line.size)
        line = np.concatenate([line, np.zeros(n - line.size, bool)])
    rng = np.random.default_rng(seed)
    z = line * np.exp(2j * np.pi * (rng.uniform() + freq * np.arange(line.size)))
    if snr_db is not None:
        sigma = 10.0 ** (-snr_db / 20.0) / np.sqrt(2.0)
        z = z + sigma * (rng.standard_normal(line.size) + 1j * rng.standard_normal(line.size))
    return z.astype(np.complex64)


SPD, FAST_SPD = 16, 4                         # samples per dot of the parity series, and of those of W = 1 and 2
LEAD = 40
PARITY_N = 1300
FAST_N = 420
PARITY_TEXTS = ("THE", "QUI", "CK ", "BRO", "WN ", "FOX", " 73", "PAR", "IS ")
SMALL_SEEDS = (7000, 7100, 7200, 7300, 7400, 7500, 7600, 7700, 7800)
FAST_SEEDS = (300, 400, 500, 600, 700, 800, 900, 1000, 1100)
SMALL_SNR, BIG_SNR, FAST_SNR = 30.0, 30.0, 30.0


def parity_text(j):
    """what receiver j keys: "VV " and three characters of its own"""
    return "VV " + PARITY_TEXTS[j % len(PARITY_TEXTS)].strip() + ("" if j % 3 else " E")


_INPUTS = {}


def parity_inputs(nrx):
    """the GPU parity test's series at 16 samples per dot: receiver j keys parity_text(j) behind LEAD samples of noise,
    1300 samples, the carrier (j mod 5 - 2) / 2048 cycles per sample off centre, noise 30 dB below it; 1, 5 and 9
    receivers are the first rows of one array, whose seeds are chosen so that every case leaves those receivers' margins
    above MARGIN (test_morse_cpu.py asserts it)"""
    key = 1024 if nrx == 1024 else 9
    if key not in _INPUTS:
        snr, seeds = (BIG_SNR, range(60000, 61024)) if key == 1024 else (SMALL_SNR, SMALL_SEEDS)
        _INPUTS[key] = np.stack([keyed_carrier(keying(parity_text(j), SPD, LEAD), snr, seeds[j], PARITY_N, (j % 5 - 2) / 2048.0)
                                 for j in range(key)])
    return _INPUTS[key][:nrx]


def fast_inputs(nrx):
    """the series at 4 samples per dot, for W = 1 and 2, up to 1024 rows: receiver j keys parity_text(j mod 9), 420
    samples, noise 30 dB below; the first nine rows have FAST_SEEDS, the others seeds of their own"""
    if "fast" not in _INPUTS:
        _INPUTS["fast"] = np.stack([keyed_carrier(keying(parity_text(j % 9), FAST_SPD, LEAD // 4), FAST_SNR,
                                                  FAST_SEEDS[j] if j < 9 else 20000 + j, FAST_N) for j in range(1024)])
    return _INPUTS["fast"][:nrx]


def two_of(spd):
    return 2 * spd * 256


def tailed_keyer(W, seed, spd=SPD, speed=1.0, shift=2):
    """the Hann window of half a dot of `spd` samples in a window of W, two0 = `speed` x the truth (two_min and two_max
    a factor of 4 below and above the truth): behind the Hann window every tap is a seeded value of modulus below 2e-4,
    so that every tap of a long window takes part in every output"""
    L = min(W, max(1, spd // 2))
    t = np.arange(W, dtype=np.float64)
    w = np.where(t < L, 1.0 - np.cos(2.0 * np.pi * (t + 1.0) / (L + 1.0)), 0.0)
    h = (w / w.sum()).astype(np.float32)
    if W > L:
        h[L:] = np.random.default_rng(seed).uniform(-2e-4, 2e-4, W - L).astype(np.float32)
    two = two_of(spd)
    return h, int(round(speed * two)), two // 4, 4 * two, shift


SPEEDS = (1.0, 0.4, 2.5, 1.0)


def case(W, nrx):
    """The parity case of window W for nrx receivers -> (bank, sel, z), to be run with CASE_PARAMS:
      1    one tap, h = [1], at 4 samples per dot: p = |z|^2 and nothing smooths it; the odd receivers are FIXED
      2    two taps (0.5, 0.5) at 4 samples per dot, shift 0: the tracker follows every pair at once
      16   one keyer, the Hann window of 8 samples with a tail, 16 samples per dot: parity_inputs
      255, 256   a bank of 16 tailed keyers, receiver j on keyer (7 j + 3) mod 16; keyer b starts at SPEEDS[b mod 4] x
           the true speed with shift b mod 5, and the receivers with j mod 4 = 3 are FIXED"""
    if W == 1:
        return ([(np.ones(1, np.float32), two_of(FAST_SPD), 512, 4 * two_of(FAST_SPD), 2)],
                [(0, ON | (FIXED if j & 1 else 0)) for j in range(nrx)], fast_inputs(nrx))
    if W == 2:
        return [(np.full(2, 0.5, np.float32), two_of(FAST_SPD), 512, 4 * two_of(FAST_SPD), 0)], [(0, ON)] * nrx, fast_inputs(nrx)
    if W == 16:
        return [tailed_keyer(16, 0)], [(0, ON)] * nrx, parity_inputs(nrx)
    bank = [tailed_keyer(W, 100 * W + b, speed=SPEEDS[b % 4], shift=b % 5) for b in range(16)]
    return bank, [((7 * j + 3) % 16, ON | (FIXED if j % 4 == 3 else 0)) for j in range(nrx)], parity_inputs(nrx)


def case_text(W, j):
    """what receiver j of case(W, .) decodes behind its "VV " where nothing goes wrong (the speed it starts from is the
    true one); None: no text is expected to compare"""
    if W > 16 and SPEEDS[((7 * j + 3) % 16) % 4] != 1.0:
        return None
    return parity_text(j % 9 if W < 16 else j)[3:]


# ---- the definition ---------------------------------------------------------------------------------------------------

def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


F32_MAX = float(np.finfo(np.float32).max)


class MorseRef:
    """The streaming definition: batches of [nrx, n] complex values.  bank: (h, two0, two_min, two_max, shift) per keyer,
    sel: (keyer, flags) per receiver.  f32 False: double.  f32 True: the float32 model."""

    def __init__(self, bank, sel, W, f32=False, a_on=0.5, a_off=0.3, rel=1.0 / 16, relf=1.0 / 64, ratio=4.0):
        self.W, self.f32 = int(W), f32
        self.h = np.stack([np.asarray(b[0], np.float32).astype(np.float64) for b in bank])
        assert self.h.shape == (len(bank), self.W) and np.isfinite(self.h).all()
        self.two0, self.two_min, self.two_max, self.shift = (np.array([int(b[i]) for b in bank], np.int64) for i in (1, 2, 3, 4))
        assert all(512 <= a <= b <= c <= 1 << 28 and 0 <= s <= 8
                   for a, b, c, s in zip(self.two_min, self.two0, self.two_max, self.shift))
        self.par = [float(np.float32(v)) for v in (a_on, a_off, rel, relf, ratio)]
        a_on, a_off, rel, relf, ratio = self.par
        assert 0 < a_off <= a_on < 1 and 0 <= rel <= 1 and 0 <= relf <= 1 and ratio >= 1
        self.nrx = len(sel)
        self.keyer = np.array([int(s[0]) for s in sel], np.int64)
        fl = np.array([int(s[1]) for s in sel], np.int64)
        assert ((0 <= self.keyer) & (self.keyer < len(bank))).all() and not (fl & ~(ON | FIXED | RESTART)).any()
        self.on, self.fixed = (fl & ON) != 0, (fl & FIXED) != 0
        self.reset()

    def _restart(self, rows):
        """meter, key and timing as at create with the receiver's keyer; the counters stay"""
        self.key[rows], self.primed[rows] = False, False
        self.hi[rows], self.lo[rows], self.pk[rows], self.fl[rows] = 0.0, np.inf, 0.0, 0.0
        self.thr_on[rows], self.thr_off[rows] = np.inf, np.inf
        self.two[rows] = self.two0[self.keyer[rows]]
        self.nel[rows], self.code[rows], self.word[rows], self.first[rows], self.last[rows] = 0, 1, False, True, 0
        self.start[rows], self.t_up[rows], self.t_down[rows] = 0, 0, 0

    def reset(self):
        K = self.nrx
        self.m = 0
        self.hist = np.zeros((K, self.W - 1), np.complex128)           # float32 values
        self.key, self.primed = np.zeros(K, bool), np.zeros(K, bool)
        self.hi, self.lo, self.pk, self.fl = (np.zeros(K) for _ in range(4))
        self.thr_on, self.thr_off = np.zeros(K), np.zeros(K)
        self.two, self.nel, self.code, self.last = (np.zeros(K, np.int64) for _ in range(4))
        self.word, self.first = np.zeros(K, bool), np.zeros(K, bool)
        self.start, self.t_up, self.t_down = (np.zeros(K, np.int64) for _ in range(3))
        self.chars, self.marks = np.zeros(K, np.int64), np.zeros(K, np.int64)
        self._restart(np.arange(K))

    def set_rx(self, rx, keyer, flags):
        assert 0 <= rx < self.nrx and 0 <= keyer < self.two0.size and not flags & ~(ON | FIXED | RESTART)
        on = bool(flags & ON)
        clear = bool(flags & RESTART) or (on and not self.on[rx])
        rekey = keyer != self.keyer[rx]
        self.keyer[rx], self.on[rx], self.fixed[rx] = keyer, on, bool(flags & FIXED)
        if clear:
            self.hist[rx] = 0.0
        if clear or rekey:
            self._restart(np.array([rx]))

    # -- envelope: the rows of the ON receivers
    def _filter(self, h, zz, n):
        W = self.W
        if not self.f32:
            if not n:
                return np.zeros((zz.shape[0], 0)), np.zeros((zz.shape[0], 0))
            win = np.lib.stride_tricks.sliding_window_view(zz, W, axis=1)
            out = np.matmul(win, h[:, ::-1, None].astype(np.complex128))[..., 0]
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
                ht = hh[:, t:t + 1].copy()
                fma(ht, zr[:, a:b], 0)
                fma(ht, zi[:, a:b], 1)
            re[r0:r0 + 32], im[r0:r0 + 32] = acc[0], acc[1]
        return re, im

    def envelope(self, z):
        """-> p [nrx, n] (float32 values with f32, double otherwise); OFF rows +0, and nothing carried moves"""
        z = np.asarray(z).reshape(self.nrx, -1).astype(np.complex64).astype(np.complex128)
        n = z.shape[1]
        rows = np.flatnonzero(self.on)
        p = np.zeros((self.nrx, n), np.float32 if self.f32 else np.float64)
        if rows.size:
            zz = np.concatenate([self.hist[rows], z[rows]], axis=1)
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                yr, yi = self._filter(self.h[self.keyer[rows]], zz, n)
                if self.f32:
                    pp = _f32(yi.astype(np.float64) * yi + (yr * yr).astype(np.float64))
                else:
                    pp = yi * yi + yr * yr
                pp = np.where(pp <= F32_MAX, pp, 0).astype(p.dtype)   # NaN and infinity compare false
            p[rows] = pp
            self.hist[rows] = zz[:, zz.shape[1] - (self.W - 1):]
        return p

    def _fma(self, a, b, c):
        """fmaf in the model's arithmetic: one rounding with f32 (the double sum of float32 values, then rounded)"""
        with np.errstate(invalid="ignore", over="ignore"):
            return _f32(a * b + c).astype(np.float64) if self.f32 else a * b + c

    def _op(self, x):
        return _f32(x).astype(np.float64) if self.f32 else x

    def track(self, p):
        """meter, key and timing over the samples p [nrx, n] -> (one CHAR array per receiver: the characters emitted in
        these samples; dist [nrx]: the least |p - threshold compared| and |pk - ratio fl| met, not yet over the peak)"""
        K, n = p.shape
        out = [[] for _ in range(K)]
        on = self.on
        a_on, a_off, rel, relf, ratio = self.par
        kk = self.keyer
        two_min, two_max, shift = self.two_min[kk], self.two_max[kk], self.shift[kk]
        dist = np.full(K, np.inf)
        pd = p.astype(np.float64)
        for i in range(n):
            m = self.m + i
            pi = pd[:, i]
            prev = self.key
            with np.errstate(invalid="ignore"):
                thr = np.where(prev, self.thr_off, self.thr_on)
                dist = np.where(on & np.isfinite(thr), np.minimum(dist, np.abs(pi - thr)), dist)
                key = np.where(pi > self.thr_on, True, np.where(pi < self.thr_off, False, prev)) & on
            key = np.where(on, key, prev)
            # 4a. emission
            emit = on & ~prev & (self.nel > 0) & (m - self.t_up == (self.two + 255) >> 8)
            for j in np.flatnonzero(emit):
                flags = (WORD if self.word[j] else 0) | (LONG if self.nel[j] > 15 else 0)
                out[j].append((self.start[j], self.code[j], self.nel[j], flags, self.two[j]))
            self.chars += emit
            self.nel = np.where(emit, 0, self.nel)
            self.code = np.where(emit, 1, self.code)
            # 4b. rising edge
            rise = on & key & ~prev
            self.t_down = np.where(rise, m, self.t_down)
            begin = rise & (self.nel == 0)
            self.start = np.where(begin, m, self.start)
            gap = np.minimum(m - self.t_up, 1 << 40)
            self.word = np.where(begin, self.first | ((gap << 9) >= 5 * self.two), self.word)
            # 4c. falling edge
            fall = on & ~key & prev
            dur = np.minimum(m - self.t_down, 1 << 24)
            dash = ((dur << 8) >= self.two).astype(np.int64)
            self.code = np.where(fall & (self.nel < 15), self.code << 1 | dash, self.code)
            self.nel = np.where(fall, np.minimum(self.nel + 1, 255), self.nel)
            self.marks += fall
            a, b = np.minimum(dur, self.last), np.maximum(dur, self.last)
            trk = fall & ~self.fixed & (self.last > 0) & (b >= 2 * a) & (b <= 4 * a)
            step = (((a + b) << 7) - self.two) >> shift               # int64: an arithmetic shift
            self.two = np.where(trk, np.clip(self.two + step, two_min, two_max), self.two)
            self.last = np.where(fall, dur, self.last)
            self.t_up = np.where(fall, m, self.t_up)
            self.first = np.where(fall, False, self.first)
            self.key = key
            # 3. the block meter
            self.hi = np.where(on, np.maximum(self.hi, pi), self.hi)
            self.lo = np.where(on, np.minimum(self.lo, pi), self.lo)
            if m & 63 == 63:
                with np.errstate(invalid="ignore", over="ignore"):
                    pk = np.where(self.primed, np.maximum(self.hi, self._fma(rel, self._op(self.fl - self.pk), self.pk)), self.hi)
                    fl = np.where(self.primed, np.minimum(self.lo, self._fma(relf, self._op(pk - self.fl), self.fl)), self.lo)
                    span = self._op(pk - fl)
                    rf = self._op(ratio * fl)
                    good = (pk >= rf) & (span > 0)
                    t_on = np.where(good, self._fma(a_on, span, fl), np.inf)
                    t_off = np.where(good, self._fma(a_off, span, fl), np.inf)
                    dist = np.where(on, np.minimum(dist, np.abs(pk - rf)), dist)
                self.pk, self.fl = np.where(on, pk, self.pk), np.where(on, fl, self.fl)
                self.thr_on, self.thr_off = np.where(on, t_on, self.thr_on), np.where(on, t_off, self.thr_off)
                self.primed = self.primed | on
                self.hi, self.lo = np.where(on, 0.0, self.hi), np.where(on, np.inf, self.lo)
        self.m += n
        return [np.array(c, CHAR) for c in out], dist

    def process(self, z):
        """-> (chars: a CHAR array per receiver, counts int64 [nrx], p [nrx, n], dist [nrx])"""
        p = self.envelope(z)
        chars, dist = self.track(p)
        return chars, np.array([c.size for c in chars], np.int64), p, dist

    def read(self):
        st = np.zeros(self.nrx, STATUS)
        st["chars"], st["marks"], st["two"], st["nel"], st["key"] = self.chars, self.marks, self.two, self.nel, self.key
        st["pk"], st["fl"] = self.pk, self.fl
        return st


def run_cuts(r, z, cuts=None, before=None):
    """all of z through r in the given batches (default: one); before(i, r) is called ahead of batch i -> (chars: a CHAR
    array per receiver, p [nrx, n], margin [nrx]: the least distance over the receiver's peak, the largest p of its row;
    inf where nothing was compared; status; peak [nrx])"""
    z = np.asarray(z)
    parts, ps, dist, off = [[] for _ in range(r.nrx)], [], np.full(r.nrx, np.inf), 0
    for i, b in enumerate(cuts or [z.shape[1]]):
        if before:
            before(i, r)
        chars, _, p, d = r.process(z[:, off:off + b])
        for j, c in enumerate(chars):
            parts[j].append(c)
        ps.append(p)
        dist = np.minimum(dist, d)
        off += b
    assert off == z.shape[1]
    p = np.concatenate(ps, axis=1)
    peak = p.astype(np.float64).max(axis=1, initial=0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.where(peak > 0, dist / np.where(peak > 0, peak, 1.0), np.inf)
    return [np.concatenate(q) for q in parts], p, margin, r.read(), peak


def distance(bank):
    """the least samples between two emissions: 1 + ((two_min + 255) >> 8), the least over the bank"""
    return min(1 + ((int(b[2]) + 255) >> 8) for b in bank)


def max_chars(bank, n):
    """pddc_morse_max_chars restated: n samples hold at most (n - 1) div D + 1 emissions, none for n = 0"""
    return (n - 1) // distance(bank) + 1 if n else 0
