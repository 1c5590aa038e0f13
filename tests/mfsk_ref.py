"""The MFSK decoder's reference: numpy, include/perseus_ddc.h "mfsk" restated.  `MfskRef` evaluates the streaming
definition in double, with f32=True the same operation order in float32 (fmaf as one rounding of the exact double product
plus the addend, double rounding aside, as in fsk_ref.py and psk_ref.py).  The filters go modem by modem, the best and the
runner-up tone by tone, the clock sample by sample, all receivers side by side; the clock and the counter are exact
integers.  Written from the header, never from the code under test.

The GPU tolerance.  tests/test_mfsk_cpu.py::test_float32_model_against_double measures the float32 model's quality and
best against the double reference's on the GPU parity test's own inputs: case(W, 9) for every window of WINDOWS and
case(W, 1024) for BIG_WINDOWS, and slow_case; quality at every strobe of every receiver whose strobes fall on the same
samples in both, best at every sample.  quality lies in [0, 1] and best, with filters of unit sum on a carrier of unit
amplitude, near 1, so the figure is absolute.  The worst per case is MODEL_WORST; TOL_MFSK = 7 x the worst of them, the
factor the other decoders' tests use.  Never taken from k_mfsk.

Decisions.  A receiver's records (start, tone, second), count and integer status are compared exactly where the
reference's margin holds: the smaller of the least quality over its strobes (tone and runner-up are as far apart as the
arithmetic's error, relative to their sum) and the least |b[m] - b[m - 2 q]| / (b[m] + b[m - 2 q]) over its strobes where
that is not exactly 0 (the clock's comparator) is at least MARGIN = 4 TOL_MFSK.  How near b[m] comes to b[m - 2 q] at a
well-timed strobe is the noise's doing, so at a given margin some receivers of a large set fall below it
(test_gpu_mfsk.py lets at most a quarter of 1024 go and none of the small sets, whose seeds were chosen on the reference
alone)."""
import numpy as np

ON, REVERSE, RESTART = 0x1, 0x2, 0x4
MAX_TONES = 32
SYM = np.dtype([("start", np.uint64), ("tone", np.uint8), ("second", np.uint8), ("flags", np.uint16), ("quality", np.float32)])
STATUS = np.dtype([("symbols", np.uint32), ("acc", np.uint32), ("skip", np.uint32), ("tone_last", np.uint32), ("q_last", np.float32)])
BACK = 128                                                            # per-sample results kept: 2 q at the most

WINDOWS = (1, 2, 16, 255, 256)
BIG_WINDOWS = (16, 256)
# test_mfsk_cpu.py::test_float32_model_against_double, the run of this file's first commit (numpy on the CPU): worst
# |float32 model - double| of quality and best per window over the sets of 9 and of 1024 receivers; "slow" is slow_case
MODEL_WORST = {1: 1.192e-07, 2: 2.409e-07, 16: 7.543e-07, 255: 4.439e-06, 256: 6.190e-06, "slow": 2.432e-06}
TOL_MFSK = 7 * max(MODEL_WORST.values())
MARGIN = 4 * TOL_MFSK
PARITY_SNR = 20.0                                                     # noise, dB below the carrier
PARITY_SYMS = 60


def cut_lists(n, TT, strobe=None, q=1):
    """the batch sizes every series of n samples is cut by, beside one batch: batches of 0 and 1 and odd ones; batches
    that end on and beside the kernel's tile seams; forty batches of one sample and the rest; and, given a strobe's sample
    and the modem's q, batches that end just before strobe - 2 q, strobe - q, the strobe and the sample behind it (so
    that a batch begins with the early, the on-time and the late sample, and with the one behind the strobe)"""
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


# ---- modems and signals, in cycles per sample --------------------------------------------------------------------------

def clock(sps, q=None, step=None):
    """inc, q and step of mfsk_modem restated for sps samples per symbol"""
    inc = min(max(int(round(float(1 << 32) / sps)), 1), 1 << 29)
    q = int(round(sps / 4.0)) if q is None else int(q)
    q = min(max(q, 1), 64)
    while q > 1 and 4 * q * inc > (1 << 32):
        q -= 1
    return inc, q, inc // 64 if step is None else int(step)


def filters(freqs, W, sps, window="rect"):
    """mfsk_modem's taps restated: h_k[t] = w[t] exp(2 pi i f_k t) over L = min(W, round(sps)) samples, freqs in cycles per
    sample -> complex64 [M, W]"""
    L = min(W, max(1, int(round(sps))))
    t = np.arange(W, dtype=np.float64)
    w = np.where(t < L, 1.0 if window == "rect" else 1.0 - np.cos(2.0 * np.pi * (t + 0.5) / L), 0.0)
    w = w / w.sum()
    return (w[None, :] * np.exp(2j * np.pi * np.asarray(freqs, np.float64)[:, None] * t[None, :])).astype(np.complex64)


def modem(freqs, W, sps, q=None, step=None, window="rect"):
    """-> (h, inc, q, step), what Mfsk's bank takes"""
    return (filters(freqs, W, sps, window),) + clock(sps, q, step)


def tone_freqs(M, sps):
    """M centred tones a baud apart, orthogonal over a boxcar of one symbol -- or, where M bauds are more than the sample
    rate holds (M > sps), 1 / M of the rate apart: neighbours then overlap and the qualities are small, which suits a
    test of the arithmetic"""
    return (np.arange(M) - (M - 1) / 2.0) / float(max(sps, M))


def encode(tones, freqs, sps, n=None, lead=0.0, ppm=0.0, snr_db=None, seed=0):
    """mfsk_encode restated: symbol k lasts T = sps (1 + ppm 1e-6) samples from lead + k T on at freqs[tones[k]] cycles per
    sample, continuous phase, unit amplitude inside the symbols and zero outside; complex white noise snr_db below the
    carrier over the whole series (None: none) and a seeded carrier phase.  -> complex64 [n]"""
    tones, freqs = np.asarray(tones, np.int64), np.asarray(freqs, np.float64)
    T = sps * (1.0 + ppm * 1e-6)
    if n is None:
        n = int(np.ceil(lead + (tones.size + 1) * T))
    k = np.floor((np.arange(n, dtype=np.float64) - lead) / T).astype(np.int64)
    inside = (k >= 0) & (k < tones.size)
    f = np.where(inside, freqs[tones[np.clip(k, 0, tones.size - 1)]], 0.0)
    phase = np.concatenate([[0.0], np.cumsum(f[:-1])])
    rng = np.random.default_rng(seed)
    z = inside * np.exp(2j * np.pi * (phase + rng.uniform()))
    if snr_db is not None:
        sigma = 10.0 ** (-snr_db / 20.0) / np.sqrt(2.0)
        z = z + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return z.astype(np.complex64)


def tailed(h, sps, seed):
    """h whose taps behind the symbol are seeded values of modulus below 2e-4, so that every tap of a long window takes
    part in every output"""
    h = h.copy()
    L = min(h.shape[1], max(1, int(round(sps))))
    if h.shape[1] > L:
        v = np.random.default_rng(seed).uniform(-2e-4, 2e-4, (h.shape[0], h.shape[1] - L, 2)).astype(np.float32)
        h[:, L:] = v[..., 0] + 1j * v[..., 1]
    return h


BANK_TONES = (2, 3, 8, 31, 32)
# seeds of the nine receivers of the small sets per window, chosen on the double reference so that every margin holds
# (test_mfsk_cpu.py::test_small_sets_hold_their_margin)
SMALL_SEEDS = {1: (9000, 9100, 9200, 9300, 9400, 9500, 9601, 9700, 9800), 2: (9000, 9101, 9200, 9300, 9400, 9501, 9600, 9701, 9800),
               16: (9001, 9105, 9200, 9300, 9400, 9501, 9600, 9700, 9800), 255: (9000, 9101, 9200, 9300, 9400, 9500, 9600, 9700, 9806),
               256: (9000, 9103, 9200, 9300, 9400, 9501, 9603, 9701, 9800)}
_CASES = {}


def case_sps(W):
    """samples per symbol of the parity case of window W"""
    return 16 if W in (16, 255) else 8


def case_bank(W):
    """The parity case's bank -> (bank, freqs per modem):
      1    M = 2, one tap each: h_0 = 1, h_1 = 0.5 i -- tone 0 always wins, quality 0.6; 8 samples per symbol, q = 1,
           step = inc / 4
      2    M = 3, two taps, tones a third of a cycle per sample apart; 8 samples per symbol, q = 2, step = inc
      16, 255, 256   a bank of 16 modems at 16 (W = 16, 255) or 8 (W = 256) samples per symbol: modem b has M = (2, 3, 8,
           31, 32)[b mod 5] tones a baud apart, the taps behind the symbol tailed, inc = 2^32 / sps - (b mod 3) 9973, step
           = (0, inc / 64, inc / 4, inc)[b mod 4], q = (1, sps / 4)[(b div 4) mod 2]
    (q = 64 has a case of its own: slow_case)"""
    sps = case_sps(W)
    if W == 1:
        inc, q, step = clock(8, 1)
        return [(np.array([[1.0], [0.5j]], np.complex64), inc, q, inc // 4)], [tone_freqs(2, 8)]
    if W == 2:
        f = np.array([-1.0, 0.0, 1.0]) / 3.0
        inc, q, _ = clock(8)
        return [(filters(f, 2, 2), inc, q, inc)], [f]
    bank, freqs = [], []
    for b in range(16):
        M = BANK_TONES[b % 5]
        f = tone_freqs(M, sps)
        inc = (1 << 32) // sps - (b % 3) * 9973
        bank.append((tailed(filters(f, W, sps), sps, 100 * W + b), inc, (1, sps // 4)[(b // 4) % 2], (0, inc // 64, inc // 4, inc)[b % 4]))
        freqs.append(f)
    return bank, freqs


def case_lead(sps, q, j):
    """where receiver j's first symbol begins: a clock that starts at 0 strobes at the samples k sps - 1 and decides at
    q before them, and a symbol's filter output peaks at its last sample; the lead puts that peak (j mod 8) / 8 - 1 / 2 of
    half a symbol from the decision, so that a fixed clock (step = 0) reads too, a quarter symbol off at the most"""
    return sps - q + ((j % 8) / 8.0 - 0.5) * sps / 2.0


def case(W, nrx):
    """The parity case of window W for nrx receivers -> (bank, sel, z): receiver j is on modem (7 j + 3) mod the bank's
    size, every fifth one REVERSE, and hears PARITY_SYMS seeded random tones of its modem, the clock (j mod 7 - 3) x 100
    ppm off, the first symbol at case_lead, noise 20 dB below over the whole series; 1, 5 and 9 receivers are the first
    rows of one array with SMALL_SEEDS"""
    key = (W, 1024 if nrx == 1024 else 9)
    if key not in _CASES:
        bank, freqs = case_bank(W)
        sps, K = case_sps(W), key[1]
        seeds = range(70000, 71024) if K == 1024 else SMALL_SEEDS[W]
        n = (PARITY_SYMS + 3) * sps
        sel = [((7 * j + 3) % len(bank), ON | (REVERSE if j % 5 == 4 else 0)) for j in range(K)]
        rows = []
        for j in range(K):
            f = freqs[sel[j][0]]
            tones = np.random.default_rng(seeds[j] + 5).integers(0, len(f), PARITY_SYMS)
            rows.append(encode(tones, f, sps, n, lead=case_lead(sps, bank[sel[j][0]][2], j), ppm=(j % 7 - 3) * 100.0, snr_db=PARITY_SNR,
                               seed=seeds[j]))
        _CASES[key] = (bank, sel, np.stack(rows))
    bank, sel, z = _CASES[key]
    return bank, sel[:nrx], z[:nrx]


SLOW_SPS, SLOW_SYMS = 256, 12


def slow_case(nrx=5):
    """q = 64 at inc = 2^24, 256 samples per symbol, W = 256, M = 8: SLOW_SYMS symbols"""
    f = tone_freqs(8, SLOW_SPS)
    h, inc, q, step = modem(f, 256, SLOW_SPS)
    assert inc == 1 << 24 and q == 64
    z = np.stack([encode(np.random.default_rng(9950 + j).integers(0, 8, SLOW_SYMS), f, SLOW_SPS, (SLOW_SYMS + 2) * SLOW_SPS,
                         lead=SLOW_SPS * j / 8.0, snr_db=PARITY_SNR, seed=9950 + j) for j in range(nrx)])
    return [(h, inc, q, inc // 4)], [(0, ON)] * nrx, z


# ---- the definition ---------------------------------------------------------------------------------------------------

def _f32(x):
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


class MfskRef:
    """The streaming definition: batches of [nrx, n] complex values.  bank: (h [M, W], inc, q, step) per modem, sel:
    (modem, flags) per receiver.  f32 False: double.  f32 True: the float32 model."""

    def __init__(self, bank, sel, W, f32=False):
        self.W, self.f32 = int(W), f32
        self.h = [np.asarray(b[0], np.complex64).astype(np.complex128) for b in bank]
        assert all(h.ndim == 2 and 2 <= h.shape[0] <= MAX_TONES and h.shape[1] == self.W and np.isfinite(h).all() for h in self.h)
        self.M = np.array([h.shape[0] for h in self.h], np.int64)
        self.inc, self.q, self.step = (np.array([int(b[i]) for b in bank], np.int64) for i in (1, 2, 3))
        assert all(1 <= i <= 1 << 29 and 1 <= q <= 64 and 4 * q * i <= 1 << 32 and 0 <= s <= i
                   for i, q, s in zip(self.inc, self.q, self.step))
        self.nrx = len(sel)
        self.modem = np.array([int(s[0]) for s in sel], np.int64)
        fl = np.array([int(s[1]) for s in sel], np.int64)
        assert ((0 <= self.modem) & (self.modem < len(bank))).all() and not (fl & ~(ON | REVERSE | RESTART)).any()
        self.on, self.rev = (fl & ON) != 0, (fl & REVERSE) != 0
        self.trace = None                                             # a list: (receiver, strobe m, quality, comparator distance) per strobe
        self.reset()

    def _restart(self, rows):
        """inputs, per-sample results and clock as at create; the counter stays"""
        self.hist[rows] = 0.0
        self.back[rows] = 0.0
        self.acc[rows], self.skip[rows], self.tone_last[rows], self.q_last[rows] = 0, 0, 0, 0.0

    def reset(self):
        K = self.nrx
        self.m = 0
        self.hist = np.zeros((K, self.W - 1), np.complex128)           # float32 values
        self.back = np.zeros((K, 4, BACK))                            # a, b, s, r of the last BACK samples
        self.acc, self.skip, self.tone_last, self.symbols = (np.zeros(K, np.int64) for _ in range(4))
        self.q_last = np.zeros(K)

    def set_rx(self, rx, modem, flags):
        assert 0 <= rx < self.nrx and 0 <= modem < self.inc.size and not flags & ~(ON | REVERSE | RESTART)
        on = bool(flags & ON)
        clear = bool(flags & RESTART) or (on and not self.on[rx]) or modem != self.modem[rx]
        self.modem[rx], self.on[rx], self.rev[rx] = modem, on, bool(flags & REVERSE)
        if clear:
            self._restart(np.array([rx]))

    def _powers(self, h, zz, n):
        """p_k of n samples of the rows zz ([R, W - 1 + n]) through the filters h ([M, W]) -> [R, M, n]"""
        W, R, M = self.W, zz.shape[0], h.shape[0]
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            if not self.f32:
                out = np.empty((R, M, n))
                hr, hi = np.ascontiguousarray(h.real[:, ::-1].T), np.ascontiguousarray(h.imag[:, ::-1].T)      # [W, M], tap W-1 first
                for r0 in range(0, R, 16):
                    win = np.lib.stride_tricks.sliding_window_view(zz[r0:r0 + 16], W, axis=1)                   # [r, n, W]
                    wr, wi = np.ascontiguousarray(win.real), np.ascontiguousarray(win.imag)
                    re = wr @ hr - wi @ hi
                    im = wi @ hr + wr @ hi
                    out[r0:r0 + 16] = np.transpose(im * im + re * re, (0, 2, 1))
                return out
            zr, zi = np.ascontiguousarray(zz.real)[:, None, :], np.ascontiguousarray(zz.imag)[:, None, :]
            re, im = np.zeros((R, M, n)), np.zeros((R, M, n))
            for t in range(W):
                a, b = W - 1 - t, W - 1 - t + n
                hr, hi = h.real[None, :, t, None], h.imag[None, :, t, None]
                re = _f32(hr * zr[:, :, a:b] + re)
                re = _f32(-hi * zi[:, :, a:b] + re)
                im = _f32(hr * zi[:, :, a:b] + im)
                im = _f32(hi * zr[:, :, a:b] + im)
            return _f32(im * im + _f32(re * re))

    @staticmethod
    def _pick(P):
        """best and runner-up over the tones, k ascending -> a, b, s, r [R, n]"""
        R, M, n = P.shape
        a, s = np.zeros((R, n), np.int64), np.zeros((R, n), np.int64)
        b, r = np.zeros((R, n)), np.zeros((R, n))
        with np.errstate(invalid="ignore"):
            for k in range(M):
                pk = P[:, k]
                g = pk > b
                g2 = ~g & (pk > r)
                r, s = np.where(g, b, r), np.where(g, a, s)
                b, a = np.where(g, pk, b), np.where(g, k, a)
                r, s = np.where(g2, pk, r), np.where(g2, k, s)
        return a, b, s, r

    def _op(self, x):
        return _f32(x) if self.f32 else x

    def process(self, z):
        """-> (syms: a SYM array per receiver, counts int64 [nrx], best float64 [nrx, n] (+0 where OFF), dist [nrx]: the
        least quality and comparator distance met in this batch, inf where none; strobes: a list of sample indices m per
        receiver)"""
        z = np.asarray(z).reshape(self.nrx, -1).astype(np.complex64).astype(np.complex128)
        K, n = z.shape
        out, strobes = [[] for _ in range(K)], [[] for _ in range(K)]
        dist, best = np.full(K, np.inf), np.zeros((K, n))
        rows = np.flatnonzero(self.on)
        if rows.size and n:
            zz = np.concatenate([self.hist[rows], z[rows]], axis=1)
            S = np.empty((rows.size, 4, BACK + n))
            S[:, :, :BACK] = self.back[rows]
            for b in np.unique(self.modem[rows]):
                sub = np.flatnonzero(self.modem[rows] == b)
                res = self._pick(self._powers(self.h[b], zz[sub], n))
                for i in range(4):
                    S[sub, i, BACK:] = res[i]
            self.hist[rows] = zz[:, zz.shape[1] - (self.W - 1):]
            self.back[rows] = S[:, :, S.shape[2] - BACK:]
            best[rows] = S[:, 1, BACK:]
            mm = self.modem[rows]
            inc, q, step = self.inc[mm], self.q[mm], self.step[mm]
            acc = self.acc[rows]
            for i in range(n):
                a2 = (acc + inc) & 0xFFFFFFFF
                hit = np.flatnonzero(a2 < acc)
                acc = a2
                for k in hit:
                    j = rows[k]
                    if self.skip[j]:                                  # the wrap a late correction borrowed from: no strobe
                        self.skip[j] = 0
                        continue
                    acc[k] = self._strobe(j, S[k], BACK + i, int(q[k]), int(step[k]), int(acc[k]), self.m + i, out[j], dist)
                    strobes[j].append(self.m + i)
            self.acc[rows] = acc
        self.m += n
        return [np.array(c, SYM) for c in out], np.array([len(c) for c in out], np.int64), best, dist, strobes

    def _strobe(self, j, S, i, q, step, acc, m, out, dist):
        op = self._op
        a, b, s, r = int(S[0, i - q]), S[1, i - q], int(S[2, i - q]), S[3, i - q]
        M = int(self.M[self.modem[j]])
        tone, second = (M - 1 - a, M - 1 - s) if self.rev[j] else (a, s)
        with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
            tot = op(b + r)
            quality = float(op(op(b - r) / tot)) if tot > 0 else 0.0
            bl, be = S[1, i], S[1, i - 2 * q]
            if not np.isnan(quality):
                dist[j] = min(dist[j], quality)
            cmp = abs(bl - be) / (bl + be) if np.isfinite(bl + be) and bl != be else np.inf
            dist[j] = min(dist[j], cmp)
        if self.trace is not None:
            self.trace.append((j, m, quality, cmp))
        if bl > be:
            if acc < step:
                self.skip[j] = 1
            acc = (acc - step) & 0xFFFFFFFF
        elif be > bl:
            acc = acc + step
        out.append(((m - q) & 0xFFFFFFFFFFFFFFFF, tone, second, 0, quality))
        self.tone_last[j], self.q_last[j] = tone, quality
        self.symbols[j] += 1
        return acc

    def read(self):
        st = np.zeros(self.nrx, STATUS)
        st["symbols"], st["acc"], st["skip"], st["tone_last"], st["q_last"] = self.symbols, self.acc, self.skip, self.tone_last, self.q_last
        return st


def run_cuts(r, z, cuts=None, before=None):
    """all of z through r in the given batches (default: one); before(i, r) is called ahead of batch i -> (syms: a SYM array
    per receiver, best [nrx, n], margin [nrx], status, strobes: sample indices per receiver)"""
    z = np.asarray(z)
    K = r.nrx
    parts, bs, st, dist, off = [[] for _ in range(K)], [], [[] for _ in range(K)], np.full(K, np.inf), 0
    for i, b in enumerate(cuts or [z.shape[1]]):
        if before:
            before(i, r)
        syms, _, best, d, strobes = r.process(z[:, off:off + b])
        for j in range(K):
            parts[j].append(syms[j])
            st[j] += strobes[j]
        bs.append(best)
        dist = np.minimum(dist, d)
        off += b
    assert off == z.shape[1]
    return [np.concatenate(c) for c in parts], np.concatenate(bs, axis=1), dist, r.read(), st


def distance(bank):
    """the least samples between two strobes: floor((2^32 - step) / inc), the least over the bank"""
    return min(((1 << 32) - int(b[3])) // int(b[1]) for b in bank)


def max_syms(bank, n):
    """pddc_mfsk_max_syms restated: n samples hold at most (n - 1) div D + 1 strobes, none for n = 0"""
    return (n - 1) // distance(bank) + 1 if n else 0


# ---- the clock's and ALE's signals ------------------------------------------------------------------------------------

CLOCK_SPS = (8.0, 16.0, 78.125)
CLOCK_SYMS, CLOCK_SETTLE = 160, 64
CLOCK_SNR = 15.0                                                      # noise, dB below the carrier (the clock facts' level)
CLOCK_SEEDS = 20


def clock_step(sps, inc):
    """a 64th of a symbol per strobe, at most a sample: step counts samples (inc is one), so it grows with the symbol"""
    return min(inc, int(round(inc * sps / 64.0)))


def clock_case(sps, seeds=CLOCK_SEEDS, snr_db=CLOCK_SNR, phases=8, ppms=(-200.0, 200.0), M=8):
    """CLOCK_SYMS random tones of M, a baud apart, at sps samples per symbol, W = one symbol: for each seed, each clock
    error of ppms and each of `phases` starting phases (k / phases of a symbol) one receiver -> (bank, sel, z, tones per
    receiver, lead per receiver, T per receiver)"""
    W = int(round(sps))
    f = tone_freqs(M, sps)
    h, inc, q, _ = modem(f, W, sps)
    bank = [(h, inc, q, clock_step(sps, inc))]
    n = int((CLOCK_SYMS + 2) * sps * 1.001)
    rows, tones, leads, Ts = [], [], [], []
    for seed in range(seeds):
        for ppm in ppms:
            for k in range(phases):
                sd = int(1000 * sps) + 50 * seed + k + (7 if ppm > 0 else 0)
                t = np.random.default_rng(sd + 3).integers(0, M, CLOCK_SYMS)
                rows.append(encode(t, f, sps, n, lead=sps * k / phases, ppm=ppm, snr_db=snr_db, seed=sd))
                tones.append(t)
                leads.append(sps * k / phases)
                Ts.append(sps * (1.0 + ppm * 1e-6))
    return bank, [(0, ON)] * len(rows), np.stack(rows), tones, np.array(leads), np.array(Ts)


ALE_RATE = 9765.625                                                   # 78.125 samples per symbol at 125 baud
# a call whose tones hold no accepted word at a wrong offset (ale_words' docstring: about one offset in a hundred does)
ALE_CALL = [("TO", "KK6"), ("TIS", "OAM"), ("DATA", "89@")]
ALE_LEAD_SYMS = 40                                                    # seeded random tones in front, for the clock to settle on
