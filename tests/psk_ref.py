"""The PSK decoder's reference: numpy, DESIGN.md 8 / include/perseus_ddc.h "psk" restated.  `PskRef` evaluates the
streaming definition in double, with f32=True the same operation order in float32 (fmaf as one rounding of the exact
double product plus the addend, double rounding aside, as in fsk_ref.py and morse_ref.py).  The clock, the decision and
the framing go sample by sample, all receivers side by side; the clock and the framing are exact integers.  Never the code
under test.

The GPU tolerance.  tests/test_psk_cpu.py::test_float32_model_against_double measures the float32 model's (d, x) pairs
against the double reference's on the GPU parity test's own inputs: case(W, 9) and case(W, 1024) for every window of
WINDOWS, every strobe of every receiver whose strobes fall on the same samples in both (all but a few of 1024, where the
two disagree on a comparator: those are the receivers whose margin does not hold).  d and x lie in [-1, 1], so the figure
is absolute.  Worst per W over both inputs is MODEL_WORST; TOL_PSK = 7 x the worst of them, the margin the fsk, morse,
tuner, demodulator, audio and receiver filter tests use.  Never taken from k_psk.

Decisions.  A receiver's characters, counts, strobe count and integer status are compared exactly where the reference's
margin holds: the least, over its strobes, of |d| (the bit is the sign of d; a strobe whose previous one is (0, 0), a
receiver's first, has dot = 0 in every arithmetic and is left out) and, where the clock's comparator is
consulted (a reversal with step > 0), of |p[m] - p[e]| / (p[m] + p[e]), is at least MARGIN = 4 TOL_PSK.  p[m] and p[e]
are sums of W squares' worth of roundings like d's numerator and denominator, so their relative difference carries an
error of d's size; 4 of them cover the two sides of the comparison twice over.  How near p[m] comes to p[e] at a
well-timed reversal is the noise's doing, so at a given margin some receivers of a large set fall below it
(test_gpu_psk.py caps them at 10 % of 1024 and at none of the small sets, whose seeds were chosen on the reference
alone)."""
import numpy as np

ON, RESTART = 0x1, 0x4
LONG = 0x1
CHAR = np.dtype([("start", np.uint64), ("code", np.uint16), ("nbits", np.uint8), ("flags", np.uint8), ("quality", np.float32)])
STATUS = np.dtype([("chars", np.uint32), ("symbols", np.uint32), ("acc", np.uint32), ("reg", np.uint32),
                   ("d_last", np.float32), ("x_last", np.float32)])
BACK = 128                                                            # filter outputs kept: 2 q at the most

WINDOWS = (1, 2, 16, 255, 256)
BIG_WINDOWS = (16, 255, 256)
MODEL_WORST = {1: 1.3745e-07, 2: 1.9279e-07, 16: 1.584e-06, 255: 6.407e-06, 256: 9.121e-06}
MODEL_WORST_PSK = max(MODEL_WORST.values())
TOL_PSK = 7 * MODEL_WORST_PSK
MARGIN = 4 * TOL_PSK
NOISE_DB = 18.0                                                       # the radio facts' noise, dB below the carrier


def cut_lists(n, TT, strobe=None, q=1):
    """the batch sizes every series of n samples is cut by, beside one batch: batches of 0 and 1 and odd ones; batches
    that end on and beside the kernel's tile seams (ends at TT - 1, TT, TT + 1, then an empty one, 2 TT, 3 TT, 3 TT + 2);
    forty batches of one sample and the rest; and, given a strobe's sample and the modem's q, batches that end just
    before strobe - 2 q, strobe - q, the strobe and the sample behind it (so that a batch begins with the early, the
    on-time and the late sample, and with the one behind the strobe)"""
    def fit(sizes):
        out = []
        for b in sizes:
            if sum(out) + b >= n:
                break
            out.append(b)
        return out + [n - sum(out)]
    lists = [fit([0, 1, 2, 30, 0, 31, 63, 64, 65, 1]), fit([TT - 1, 1, 1, 0, TT - 1, TT, 2]), fit([1] * 40)]
    if strobe is not None and strobe - 2 * q > 0:
        lists.append(fit([strobe - 2 * q, q, q, 1]))
    return lists


# ---- Varicode, restated -----------------------------------------------------------------------------------------------

VARICODE = (
    "1010101011 1011011011 1011101101 1101110111 1011101011 1101011111 1011101111 1011111101 1011111111 11101111 11101 "
    "1101101111 1011011101 11111 1101110101 1110101011 1011110111 1011110101 1110101101 1110101111 1101011011 1101101011 "
    "1101101101 1101010111 1101111011 1101111101 1110110111 1101010101 1101011101 1110111011 1011111011 1101111111 1 "
    "111111111 101011111 111110101 111011011 1011010101 1010111011 101111111 11111011 11110111 101101111 111011111 1110101 "
    "110101 1010111 110101111 10110111 10111101 11101101 11111111 101110111 101011011 101101011 110101101 110101011 "
    "110110111 11110101 110111101 111101101 1010101 111010111 1010101111 1010111101 1111101 11101011 10101101 10110101 "
    "1110111 11011011 11111101 101010101 1111111 111111101 101111101 11010111 10111011 11011101 10101011 11010101 "
    "111011101 10101111 1101111 1101101 101010111 110110101 101011101 101110101 101111011 1010101101 111110111 111101111 "
    "111111011 1010111111 101101101 1011011111 1011 1011111 101111 101101 11 111101 1011011 101011 1101 111101011 10111111 "
    "11011 111011 1111 111 111111 110111111 10101 10111 101 110111 1111011 1101011 11011111 1011101 111010101 1010110111 "
    "110111011 1010110101 1011010111 1110110101").split()
TEXT = "CQ CQ DE TEST TEST pse k"


def bits_of(text):
    """the bits that send `text`: each character's code and 00; a 0 is a phase reversal"""
    out = []
    for ch in text:
        out += [int(b) for b in VARICODE[ord(ch)]] + [0, 0]
    return out


def decode(records):
    """psk_varicode restated, over records or codes"""
    back = {int(b, 2): chr(i) for i, b in enumerate(VARICODE)}
    return "".join(back.get(int(c["code"]) if isinstance(c, np.void) else int(c), "\ufffd") for c in records)


def modem(W, sps, step=None, q=None):
    """psk_modem restated"""
    L = min(W, max(1, int(round(2.0 * sps))))
    t = np.arange(W, dtype=np.float64)
    w = np.where(t < L, 1.0 + np.cos(np.pi * (t - (L - 1) / 2.0) / sps), 0.0)
    inc = min(max(int(round(float(1 << 32) / sps)), 1), 1 << 29)
    q = int(round(sps / 4.0)) if q is None else int(q)
    q = min(max(q, 1), 64)
    while q > 1 and 4 * q * inc > (1 << 32):
        q -= 1
    return (w / w.sum()).astype(np.float32), inc, q, inc // 4 if step is None else int(step)


# ---- signals ----------------------------------------------------------------------------------------------------------

def bpsk(bits, sps, n=None, lead=0, snr_db=None, seed=0, freq=0.0, ppm=0.0, phase=0.0):
    """`bits` keyed the way PSK31 is: a symbol lasts T = sps (1 + ppm 1e-6) samples, symbol k's amplitude a_k = +-1
    changes sign with every 0, the baseband is sum a_k g(t - t_k) with the raised cosine g(t) = (1 + cos(pi t / T)) / 2
    over |t| <= T: flat where the sign stays, a cosine through zero where it turns.  Symbol k's middle is at t_k = lead +
    (k + phase) T.  The carrier has unit amplitude, `freq` cycles per sample off centre and a seeded phase; complex white
    noise snr_db below it (None: none).  -> complex64 [n]"""
    T = sps * (1.0 + ppm * 1e-6)
    a = np.cumprod(np.where(np.asarray(bits) > 0, 1.0, -1.0))
    if n is None:
        n = int(lead + (len(a) + 2) * T)
    t = np.arange(n, dtype=np.float64)
    base = np.zeros(n)
    for k, ak in enumerate(a):
        tk = lead + (k + phase) * T
        i0, i1 = max(int(np.ceil(tk - T)), 0), min(int(np.floor(tk + T)) + 1, n)
        if i1 > i0:
            base[i0:i1] += ak * 0.5 * (1.0 + np.cos(np.pi * (t[i0:i1] - tk) / T))
    rng = np.random.default_rng(seed)
    z = base * np.exp(2j * np.pi * (rng.uniform() + freq * t))
    if snr_db is not None:
        sigma = 10.0 ** (-snr_db / 20.0) / np.sqrt(2.0)
        z = z + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return z.astype(np.complex64)


PARITY_TEXTS = ("et o", "CQ", "de", "k a", "73", "Qe", "ni", "o t", " ee")
SMALL_SEEDS = {8: (9000, 9100, 9200, 9300, 9404, 9501, 9600, 9700, 9800), 16: tuple(range(9000, 9900, 100))}     # per samples per symbol
PARITY_SNR = 20.0
PARITY_SYMS = 80
_INPUTS = {}


def parity_bits(j):
    """what receiver j sends: six idle reversals, its text, idle reversals up to PARITY_SYMS symbols"""
    b = [0] * 6 + bits_of(PARITY_TEXTS[j % len(PARITY_TEXTS)])
    return b + [0] * (PARITY_SYMS - len(b))


def parity_inputs(nrx, sps):
    """the GPU parity test's series at sps samples per symbol: receiver j sends parity_bits(j), the clock (j mod 7 - 3) x
    100 ppm off, the first symbol's middle (j mod 8) / 8 of a symbol late, the carrier (j mod 5 - 2) / 8192 cycles per
    sample off centre, noise 20 dB below; 1, 5 and 9 receivers are the first rows of one array with SMALL_SEEDS"""
    key = (1024 if nrx == 1024 else 9, sps)
    if key not in _INPUTS:
        seeds = range(70000, 71024) if key[0] == 1024 else SMALL_SEEDS[sps]
        n = int((PARITY_SYMS + 3) * sps)
        _INPUTS[key] = np.stack([bpsk(parity_bits(j), sps, n, lead=sps, snr_db=PARITY_SNR, seed=seeds[j], freq=(j % 5 - 2) / 8192.0,
                                      ppm=(j % 7 - 3) * 100.0, phase=(j % 8) / 8.0) for j in range(key[0])])
    return _INPUTS[key][:nrx]


def tailed_modem(W, sps, seed, step=None, q=None):
    """modem(W, sps) whose taps behind the pulse are seeded values of modulus below 2e-4, so that every tap of a long
    window takes part in every output"""
    h, inc, q, step = modem(W, sps, step, q)
    L = min(W, max(1, int(round(2.0 * sps))))
    if W > L:
        h[L:] = np.random.default_rng(seed).uniform(-2e-4, 2e-4, W - L).astype(np.float32)
    return h, inc, q, step


def case(W, nrx):
    """The parity case of window W for nrx receivers -> (bank, sel, z):
      1    one tap, h = [1], 8 samples per symbol: inc = 2^29, q = 1, step = inc / 16
      2    two taps (0.5, 0.5), 8 samples per symbol, q = 1, step = inc: a whole symbol per reversal at the most
      16   16 samples per symbol, the pulse cut to 16 taps, q = 4; the odd receivers on a second modem with step = 0
      255, 256   a bank of 16 tailed modems at 16 samples per symbol, receiver j on modem (7 j + 3) mod 16: modem b has
           inc = 2^28 - (b mod 4) 9973, no power of two from b mod 4 = 1 on (at the most 112 ppm slow), q = 1 + (b div 4)
           mod 4,
           step = (0, inc / 64, inc / 16, inc / 8)[b mod 4]
    (q = 64 at inc = 2^24 has a case of its own: slow_case)"""
    if W == 1:
        return [(np.ones(1, np.float32), 1 << 29, 1, 1 << 25)], [(0, ON)] * nrx, parity_inputs(nrx, 8)
    if W == 2:
        return [(np.full(2, 0.5, np.float32), 1 << 29, 1, 1 << 29)], [(0, ON)] * nrx, parity_inputs(nrx, 8)
    if W == 16:
        h, inc, q, step = modem(16, 16)
        return [(h, inc, q, step), (h, inc, q, 0)], [(j & 1, ON) for j in range(nrx)], parity_inputs(nrx, 16)
    bank = []
    for b in range(16):
        inc = (1 << 28) - (b % 4) * 9973
        h = tailed_modem(W, 16, 100 * W + b)[0]
        bank.append((h, inc, 1 + (b // 4) % 4, (0, inc // 64, inc // 16, inc // 8)[b % 4]))
    return bank, [((7 * j + 3) % 16, ON) for j in range(nrx)], parity_inputs(nrx, 16)


SLOW_SPS, SLOW_SYMS = 256, 12


def slow_case(nrx=5):
    """q = 64 at inc = 2^24, 256 samples per symbol, W = 256: SLOW_SYMS symbols of reversals and ones"""
    h, inc, q, step = modem(256, SLOW_SPS)
    assert inc == 1 << 24 and q == 64
    bits = [0, 0, 0, 1, 0, 1, 1, 0, 0, 0, 1, 0]
    z = np.stack([bpsk(bits, SLOW_SPS, (SLOW_SYMS + 2) * SLOW_SPS, lead=SLOW_SPS, snr_db=PARITY_SNR, seed=9950 + j, phase=j / 8.0)
                  for j in range(nrx)])
    return [(h, inc, q, step)], [(0, ON)] * nrx, z


# ---- the definition ---------------------------------------------------------------------------------------------------

def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


class PskRef:
    """The streaming definition: batches of [nrx, n] complex values.  bank: (h, inc, q, step) per modem, sel: (modem,
    flags) per receiver.  f32 False: double.  f32 True: the float32 model."""

    def __init__(self, bank, sel, W, f32=False):
        self.W, self.f32 = int(W), f32
        self.h = np.stack([np.asarray(b[0], np.float32).astype(np.float64) for b in bank])
        assert self.h.shape == (len(bank), self.W) and np.isfinite(self.h).all()
        self.inc, self.q, self.step = (np.array([int(b[i]) for b in bank], np.int64) for i in (1, 2, 3))
        assert all(1 <= i <= 1 << 29 and 1 <= q <= 64 and 4 * q * i <= 1 << 32 and 0 <= s <= i
                   for i, q, s in zip(self.inc, self.q, self.step))
        self.nrx = len(sel)
        self.modem = np.array([int(s[0]) for s in sel], np.int64)
        fl = np.array([int(s[1]) for s in sel], np.int64)
        assert ((0 <= self.modem) & (self.modem < len(bank))).all() and not (fl & ~(ON | RESTART)).any()
        self.on = (fl & ON) != 0
        self.reset()

    def _restart(self, rows):
        """inputs, outputs, clock, pair and framing as at create; the counters stay"""
        self.hist[rows] = 0.0
        self.yhist[rows] = 0.0
        self.acc[rows], self.reg[rows], self.nb[rows], self.start[rows] = 0, 0, 0, 0
        self.v[rows], self.pv[rows], self.qmin[rows], self.d_last[rows], self.x_last[rows] = 0.0, 0.0, 0.0, 0.0, 0.0

    def reset(self):
        K = self.nrx
        self.m = 0
        self.hist = np.zeros((K, self.W - 1), np.complex128)           # float32 values
        self.yhist = np.zeros((K, BACK), np.complex128)
        self.acc, self.reg, self.nb, self.start = (np.zeros(K, np.int64) for _ in range(4))
        self.v = np.zeros(K, np.complex128)
        self.pv, self.qmin, self.d_last, self.x_last = (np.zeros(K) for _ in range(4))
        self.chars, self.symbols = np.zeros(K, np.int64), np.zeros(K, np.int64)

    def set_rx(self, rx, modem, flags):
        assert 0 <= rx < self.nrx and 0 <= modem < self.inc.size and not flags & ~(ON | RESTART)
        on = bool(flags & ON)
        clear = bool(flags & RESTART) or (on and not self.on[rx]) or modem != self.modem[rx]
        self.modem[rx], self.on[rx] = modem, on
        if clear:
            self._restart(np.array([rx]))

    def _filter(self, h, zz, n):
        W = self.W
        if not self.f32:
            if not n:
                return np.zeros((zz.shape[0], 0)), np.zeros((zz.shape[0], 0))
            win = np.lib.stride_tricks.sliding_window_view(zz, W, axis=1)
            hr = h[:, ::-1, None]                                     # real taps on real parts: an infinity stays one
            return np.matmul(win.real, hr)[..., 0], np.matmul(win.imag, hr)[..., 0]
        # the float32 model: the accumulators hold float32 values in double; a block of rows at a time stays in the cache
        R = zz.shape[0]
        re, im = np.zeros((R, n)), np.zeros((R, n))
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

    def _op(self, x):
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            return _f32(x).astype(np.float64) if self.f32 else x

    def _power(self, y):
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            return self._op(y.imag * y.imag + self._op(y.real * y.real))

    def process(self, z):
        """-> (chars: a CHAR array per receiver, counts int64 [nrx], sym: a float64 [nsym, 2] array per receiver, dist
        [nrx]: the least |d| and comparator distance met in this batch, inf where none; strobes: a list of sample indices m
        per receiver)"""
        z = np.asarray(z).reshape(self.nrx, -1).astype(np.complex64).astype(np.complex128)
        K, n = z.shape
        out, syms, strobes = [[] for _ in range(K)], [[] for _ in range(K)], [[] for _ in range(K)]
        dist = np.full(K, np.inf)
        rows = np.flatnonzero(self.on)
        if rows.size and n:
            zz = np.concatenate([self.hist[rows], z[rows]], axis=1)
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                yr, yi = self._filter(self.h[self.modem[rows]], zz, n)
            Y = np.empty((rows.size, BACK + n), np.complex128)
            Y[:, :BACK], Y.real[:, BACK:], Y.imag[:, BACK:] = self.yhist[rows], yr, yi
            self.hist[rows] = zz[:, zz.shape[1] - (self.W - 1):]
            self.yhist[rows] = Y[:, Y.shape[1] - BACK:]
            mm = self.modem[rows]
            inc, q, step = self.inc[mm], self.q[mm], self.step[mm]
            acc = self.acc[rows]
            for i in range(n):
                a2 = (acc + inc) & 0xFFFFFFFF
                hit = np.flatnonzero(a2 < acc)
                acc = a2
                for k in hit:
                    j = rows[k]
                    acc[k] = self._strobe(j, Y[k], BACK + i, int(q[k]), int(step[k]), int(acc[k]), self.m + i, out[j], syms[j], dist)
                    strobes[j].append(self.m + i)
            self.acc[rows] = acc
        self.m += n
        return ([np.array(c, CHAR) for c in out], np.array([len(c) for c in out], np.int64),
                [np.array(s, np.float64).reshape(-1, 2) for s in syms], dist, strobes)

    def _strobe(self, j, Y, i, q, step, acc, m, out, syms, dist):
        op = self._op
        u, pu = Y[i - q], self._power(Y[i - q])
        v, pv = self.v[j], self.pv[j]
        with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
            dot = op(u.imag * v.imag + op(u.real * v.real))
            cross = op(u.imag * v.real + -op(u.real * v.imag))
            s = op(pu + pv)
            d = op(op(dot + dot) / s) if s > 0 else 0.0
            x = op(op(cross + cross) / s) if s > 0 else 0.0
        bit = 1 if dot > 0 else 0
        if np.isfinite(d) and pv > 0:                                  # (behind a zero pair dot is 0 in every arithmetic)
            dist[j] = min(dist[j], abs(d))
        if not bit:
            pm, pe = self._power(Y[i]), self._power(Y[i - 2 * q])
            if step > 0 and pm + pe > 0 and np.isfinite(pm + pe):
                dist[j] = min(dist[j], abs(pm - pe) / (pm + pe))
            if pm > pe:
                acc = acc - step if acc >= step else 0
            elif pe > pm:
                acc = acc + step
        ad = abs(d)
        if self.reg[j] or bit:
            if not self.reg[j]:
                self.start[j], self.nb[j], self.qmin[j] = m - q, 0, ad
            self.reg[j] = (self.reg[j] << 1 | bit) & 0xFFFFFFFF
            self.nb[j] = min(self.nb[j] + 1, 255)
            self.qmin[j] = np.fmin(self.qmin[j], ad)
            if not self.reg[j] & 3:
                nbits = int(self.nb[j]) - 2
                out.append((int(self.start[j]) & 0xFFFFFFFFFFFFFFFF, (int(self.reg[j]) >> 2) & 0xFFFF, nbits, LONG if nbits > 16 else 0,
                            self.qmin[j]))
                self.chars[j] += 1
                self.reg[j] = 0
        syms.append((d, x))
        self.v[j], self.pv[j], self.d_last[j], self.x_last[j] = u, pu, d, x
        self.symbols[j] += 1
        return acc

    def read(self):
        st = np.zeros(self.nrx, STATUS)
        st["chars"], st["symbols"], st["acc"], st["reg"] = self.chars, self.symbols, self.acc, self.reg
        st["d_last"], st["x_last"] = self.d_last, self.x_last
        return st


def run_cuts(r, z, cuts=None, before=None):
    """all of z through r in the given batches (default: one); before(i, r) is called ahead of batch i -> (chars: a CHAR
    array per receiver, sym: a [nsym, 2] array per receiver, margin [nrx], status, strobes: sample indices per receiver)"""
    z = np.asarray(z)
    K = r.nrx
    parts, sy, st, dist, off = [[] for _ in range(K)], [[] for _ in range(K)], [[] for _ in range(K)], np.full(K, np.inf), 0
    for i, b in enumerate(cuts or [z.shape[1]]):
        if before:
            before(i, r)
        chars, _, sym, d, strobes = r.process(z[:, off:off + b])
        for j in range(K):
            parts[j].append(chars[j])
            sy[j].append(sym[j])
            st[j] += strobes[j]
        dist = np.minimum(dist, d)
        off += b
    assert off == z.shape[1]
    return [np.concatenate(c) for c in parts], [np.concatenate(s) for s in sy], dist, r.read(), st


def distance(bank):
    """the least samples between two strobes: floor((2^32 - step) / inc), the least over the bank"""
    return min(((1 << 32) - int(b[3])) // int(b[1]) for b in bank)


def max_syms(bank, n):
    """pddc_psk_max_syms restated: n samples hold at most (n - 1) div D + 1 strobes, none for n = 0"""
    return (n - 1) // distance(bank) + 1 if n else 0


def max_chars(bank, n):
    """pddc_psk_max_chars restated: emissions lie at least 3 strobes apart"""
    s = max_syms(bank, n)
    return (s - 1) // 3 + 1 if s else 0


# ---- the radio facts' signals -------------------------------------------------------------------------------------------

RADIO_SPS = (16, 40)
RADIO_W = 80
RADIO_SEEDS = 20
RADIO_WANT = TEXT[3:]                                                 # the text from the second word on


def radio_case(snr_db, seeds=RADIO_SEEDS, step=None, phases=8, ppms=(-200.0, 200.0), freq=0.0, sps_list=RADIO_SPS, idle=64):
    """TEXT behind eight idle reversals, with raised-cosine keying: for each of `seeds` seeds, each samples-per-symbol of
    sps_list, each clock error of ppms and each of `phases` starting phases (k / phases of a symbol) one receiver, noise
    snr_db below the carrier; the rows of the faster modem are filled up with noise alone.  W = 80 takes both pulses whole.
    -> (bank, sel, z)"""
    bits = [0] * idle + bits_of(TEXT) + [0] * 4
    bank = [modem(RADIO_W, s, step=None if step is None else modem(RADIO_W, s)[1] // step) for s in sps_list]
    n = int((len(bits) + 3) * max(sps_list))
    rows, sel = [], []
    for b, sps in enumerate(sps_list):
        for seed in range(seeds):
            for ppm in ppms:
                for k in range(phases):
                    rows.append(bpsk(bits, sps, n, lead=sps, snr_db=snr_db, seed=1000 * sps + 50 * seed + k + (7 if ppm > 0 else 0),
                                     freq=freq, ppm=ppm, phase=k / phases))
                    sel.append((b, ON))
    return bank, sel, np.stack(rows)


def radio_read(chars):
    """how many receivers read RADIO_WANT"""
    return sum(RADIO_WANT in decode(c) for c in chars)


# ---- the capacity bounds' input ------------------------------------------------------------------------------------------

def advancing_case(bits=None, n=1200):
    """W = 1, h = [1], inc = 2^29, q = 1, step = inc: D = 7.  The input makes the receiver decide `bits` (default: zeros
    throughout; the first strobe's bit is 0 whatever comes, its pair being zero) and advances its clock at every
    reversal: around each strobe m the real amplitude falls linearly from m - 4 on, so p[m - 2] > p[m], and its sign
    turns where the bit is 0.  The strobes are where the clock's own rule puts them, from the first at sample 7: 7 samples
    behind a reversal (acc = 0 + step), 8 behind a 1 (acc = 0).  -> (bank, sel, z [1, n], D, the first strobe)"""
    bank, sel = [(np.ones(1, np.float32), 1 << 29, 1, 1 << 29)], [(0, ON)]
    z = np.zeros(n + 16)
    m, sign, k = 7, 1.0, 0
    while m - 4 < n:
        bit = 0 if k == 0 or bits is None else int(bits[(k - 1) % len(bits)])
        if not bit and k:
            sign = -sign
        nxt = m + (8 if bit else 7)
        z[m - 4:nxt - 4] = sign * (8.0 - np.arange(nxt - m))
        m, k = nxt, k + 1
    return bank, sel, z[None, :n].astype(np.complex64), 7, 7
