"""The SITOR decoder's reference: numpy, DESIGN.md 8 / include/perseus_ddc.h "sitor" restated.  `SitorRef` evaluates the
streaming definition in double, with f32=True the same operation order in float32.  The discriminator is fsk's, so it is
fsk_ref.FskRef's `discriminate` (the double sum, and the float32 model with fmaf as one rounding of the exact double product
plus the addend); the clock, the framing (rules a - c) and the bounds are restated here in Python integers, sample by sample,
all receivers side by side.  Never the code under test.

The GPU tolerance.  tests/test_sitor_cpu.py::test_float32_model_against_double measures the float32 model's d at the strobes
against the double reference's on the GPU parity test's own inputs: case(W, 9) for every window of WINDOWS and case(W, 1024)
for those of BIG_WINDOWS, every receiver, at the strobes the double reference's clock gives (`model_d_at` evaluates the
float32 operation sequence at those samples alone, which is what `soft` holds).  Worst |d_model - d_ref| per W is in
MODEL_WORST; TOL_SITOR = 7 x the largest, the margin every decoder here uses.  Never taken from k_sitor.

Decisions.  They are integer, and every sample's decision can be a transition that moves the clock.  So a receiver's
records, counts, nsoft and integer status are compared exactly where the least |d| of the double reference over all its
samples, from the first full window on (W - 1 samples behind zero history), is at least MARGIN = 4 TOL_SITOR: an error of
TOL_SITOR on either side cannot turn a decision.  A two-tone signal passes d = 0 at every change of tone; what the sample
next to that point reads is the noise's doing, so some receivers of a large set fall below the margin: none of the small
sets may (their seeds are chosen on this reference), and at most a quarter of the 1024 (test_sitor_cpu.py asserts both on
the reference).  The series is 30 character slots behind 4 phasing pairs, 266 bits, 4352 samples: on it the reference keeps
all but one or two of the 1024 above MARGIN (the tones change on whole samples, where the window holds as much of the one
as of the other and the two tones' cross terms, not the noise alone, decide what the sample reads).

The M.476 table is the project's, restated; it is unverified against the Recommendation's text."""
import numpy as np

import fsk_ref
from fsk_ref import two_tone

ON, REVERSE, RESTART = 0x1, 0x2, 0x4
VALID = 0x1
CHAR = np.dtype([("start", np.uint64), ("code", np.uint16), ("flags", np.uint16), ("quality", np.float32)])
STATUS = np.dtype([("chars", np.uint32), ("symbols", np.uint32), ("errors", np.uint32), ("reframes", np.uint32),
                   ("locked", np.uint32), ("acc", np.uint32), ("reg", np.uint32), ("d_last", np.float32)])
INT_STATUS = ("chars", "symbols", "errors", "reframes", "locked", "acc", "reg")

WINDOWS = (1, 2, 16, 255, 256)
BIG_WINDOWS = (16, 255, 256)
MODEL_WORST = {1: 8.345e-08, 2: 1.435e-07, 16: 5.516e-07, 255: 2.760e-06, 256: 2.791e-06}
MODEL_WORST_SITOR = max(MODEL_WORST.values())
TOL_SITOR = 7 * MODEL_WORST_SITOR
MARGIN = 4 * TOL_SITOR
BELOW_CAP = 256                                                       # of 1024 receivers

ALPHA, BETA, REPEAT, LTRS, FIGS, BLANK = 0x0F, 0x33, 0x66, 0x5A, 0x36, 0x6A
PHASE_A = ALPHA << 21 | BETA << 14 | ALPHA << 7 | BETA
PHASE_B = BETA << 21 | ALPHA << 14 | BETA << 7 | ALPHA
LETTERS = {"J": 0x17, "F": 0x1B, "C": 0x1D, "K": 0x1E, "W": 0x27, "Y": 0x2B, "P": 0x2D, "Q": 0x2E, "G": 0x35, "M": 0x39,
           "X": 0x3A, "V": 0x3C, "A": 0x47, "S": 0x4B, "I": 0x4D, "U": 0x4E, "D": 0x53, "R": 0x55, "E": 0x56, "N": 0x59,
           " ": 0x5C, "Z": 0x63, "L": 0x65, "H": 0x69, "\n": 0x6C, "O": 0x71, "B": 0x72, "T": 0x74, "\r": 0x78}
OTHERS = {"alpha": ALPHA, "beta": BETA, "repeat": REPEAT, "letters": LTRS, "figures": FIGS, "blank": BLANK}
TEXT = "ZCZC EA12 THE QUICK BROWN FOX 0123456789 JUMPS OVER THE LAZY DOG\r\nNNNN"


def weight(code):
    return bin(int(code) & 0x7F).count("1")


def encode(text, phasing=16):
    """sitor_encode restated: -> (slot codes, bits); DX slots even, RX slots odd and five behind; beta fills DX, alpha RX"""
    codes, figs = [], False
    for ch in text:
        tab, other = (fsk_ref.FIGS, fsk_ref.LTRS) if figs else (fsk_ref.LTRS, fsk_ref.FIGS)
        if ch not in tab or ch == "\0":
            assert ch in other and ch != "\0", ch
            figs = not figs
            tab = other
            codes.append(FIGS if figs else LTRS)
        codes.append(LETTERS[fsk_ref.LTRS[tab.index(ch)]])
    P, N = phasing, len(codes)
    slots = [BETA if k % 2 == 0 else ALPHA for k in range(2 * (P + N) + 6)]
    for i, c in enumerate(codes):
        slots[2 * (P + i)] = slots[2 * (P + i) + 5] = c
    return np.array(slots, np.uint8), np.array([(c >> k) & 1 for c in slots for k in range(7)], np.uint8)


def modem(W, sps, shift=1.7, step=None, lock=3, unlock=4, inc=None):
    """sitor_modem restated: boxcars of min(W, round(sps)) samples with sum 1 under exp(+-2 pi i (shift / 2 sps) t)"""
    L = min(W, max(1, int(round(sps))))
    t = np.arange(W, dtype=np.float64)
    w = (t < L) / float(L)
    f = shift / (2.0 * sps)
    if inc is None:
        inc = min(max(int(round(2.0 ** 32 / sps)), 1), 1 << 29)
    return ((w * np.exp(2j * np.pi * f * t)).astype(np.complex64), (w * np.exp(-2j * np.pi * f * t)).astype(np.complex64), inc,
            inc // 8 if step is None else step, lock, unlock)


def keying(bits, sps, lead=0, ppm=0.0, n=None):
    """the line of a synchronous bit series, a value per sample, True = space (bit 0): `lead` samples of mark, then bit k
    from sample lead + k sps (1 + ppm 1e-6) on, mark behind the last; n samples (default: two bits behind the last)"""
    T = sps * (1.0 + ppm * 1e-6)
    if n is None:
        n = lead + int(np.ceil((len(bits) + 2) * T))
    k = np.floor((np.arange(n) - lead) / T).astype(np.int64)
    b = np.asarray(bits, np.uint8)
    inside = (k >= 0) & (k < b.size)
    return inside & (b[np.clip(k, 0, b.size - 1)] == 0)


# ---- the clock and the framing, restated in Python integers ------------------------------------------------------------

M32 = (1 << 32) - 1


def clock(acc, inc):
    """one sample -> (acc, strobe)"""
    a2 = (acc + inc) & M32
    return a2, a2 < acc


def correct(acc, step):
    return acc + step if acc < (1 << 31) else acc - step


class Frame:
    """what a receiver's framing carries, and rules a - c"""

    def __init__(self):
        self.chars = self.symbols = self.errors = self.reframes = 0
        self.restart()

    def restart(self):
        self.reg = self.seen = self.nb = self.bad = self.locked = 0
        self.start, self.qmin = 0, 0.0

    def strobe(self, space, m, q, lock, unlock, rule_b=True):
        """-> a record (start, code, flags, quality) or None"""
        out = None
        self.symbols += 1
        self.reg = (self.reg >> 1) | ((0 if space else 1) << 27)
        self.seen = min(self.seen + 1, 28)
        if self.locked:
            if self.nb == 0:
                self.start, self.qmin = m, q
            else:
                self.qmin = float(np.fmin(self.qmin, q))
            self.nb += 1
            if self.nb == 7:
                code = self.reg >> 21
                ok = weight(code) == 4
                out = (self.start, code, VALID if ok else 0, self.qmin)
                self.chars += 1
                self.nb = 0
                if ok:
                    self.bad = 0
                else:
                    self.errors += 1
                    self.bad += 1
                if self.bad >= unlock:
                    self.locked = self.seen = 0
        if rule_b and self.reg in (PHASE_A, PHASE_B):
            if not (self.locked and self.nb == 0):
                self.reframes += 1
            self.locked, self.nb, self.bad = 1, 0, 0
        elif (not self.locked and lock > 0 and self.seen >= 7 * lock
              and all(weight(self.reg >> (21 - 7 * g)) == 4 for g in range(lock))):
            self.locked, self.nb, self.bad = 1, 0, 0
        return out


def frame_bits(bits, lock=3, unlock=4, rule_b=True, frame=None, m0=0, every=16):
    """a bit series (1 = mark) through the framing alone, strobe k at sample m0 + every k -> (records as a CHAR array, frame)"""
    f = frame or Frame()
    out = []
    for k, b in enumerate(bits):
        r = f.strobe(not b, m0 + every * k, 1.0, lock, unlock, rule_b)
        if r:
            out.append(r)
    return np.array(out, CHAR), f


def distance(bank):
    """the least distance of two strobes the bounds are made with: 2^31 div inc, the least over the bank"""
    return min((1 << 31) // int(b[2]) for b in bank)


def max_syms(bank, n):
    return (n - 1) // distance(bank) + 1 if n else 0


def max_chars(bank, n):
    s = max_syms(bank, n)
    return (s - 1) // 7 + 1 if s else 0


# ---- the definition ---------------------------------------------------------------------------------------------------

class SitorRef:
    """The streaming definition: batches of [nrx, n] complex values.  bank: (hm, hs, inc, step, lock, unlock) per modem,
    sel: (modem, flags) per receiver.  f32 False: double.  f32 True: the float32 model.  rule_b False: the framing
    without the phasing words (for the radio facts' comparison only)."""

    def __init__(self, bank, sel, W, f32=False, rule_b=True):
        self.W, self.f32, self.rule_b = int(W), f32, rule_b
        self.inc = np.array([int(b[2]) for b in bank], np.int64)
        self.step = np.array([int(b[3]) for b in bank], np.int64)
        self.lock = [int(b[4]) for b in bank]
        self.unlock = [int(b[5]) for b in bank]
        assert all(1 <= i <= 1 << 29 for i in self.inc) and (self.step <= self.inc).all() and (self.step >= 0).all()
        assert all(k in (0, 2, 3, 4) for k in self.lock) and all(1 <= u <= 15 for u in self.unlock)
        # the discriminator: fsk's, with a stand-in for the fields its modems have and these have not
        self.disc = fsk_ref.FskRef([(b[0], b[1], int(b[2]), 5) for b in bank], [(int(s[0]), int(s[1])) for s in sel], W, f32=f32)
        self.nrx = len(sel)
        self.reset()

    def reset(self):
        K = self.nrx
        self.disc.reset()
        self.m = 0
        self.acc = np.zeros(K, np.int64)
        self.prev = np.zeros(K, bool)
        self.frames = [Frame() for _ in range(K)]
        self.d_last = np.zeros(K, np.float64)
        self.age = np.zeros(K, np.int64)                               # samples since zero history

    def set_rx(self, rx, modem, flags):
        on_before, modem_before = bool(self.disc.on[rx]), int(self.disc.modem[rx])
        self.disc.set_rx(rx, modem, flags)
        if flags & RESTART or (flags & ON and not on_before):
            self.acc[rx], self.prev[rx], self.age[rx] = 0, False, 0
            self.frames[rx].restart()
        if modem != modem_before:
            self.frames[rx].restart()

    def process(self, z, want_strobes=False):
        """-> (chars: a CHAR array per receiver, counts int64 [nrx], soft: an array of d per receiver, margin [nrx]: the
        least |d| over this batch's samples from the receiver's first full window on, inf where there is none);
        with want_strobes a fifth: the strobes' sample indices within the batch, per receiver"""
        space, d, _ = self.disc.discriminate(z)
        K, n = space.shape
        on = self.disc.on.copy()
        full = on[:, None] & (self.age[:, None] + np.arange(n)[None, :] >= self.W - 1)
        with np.errstate(invalid="ignore"):
            ad = np.abs(d.astype(np.float64))
            margin = np.where(full & ~np.isnan(ad), ad, np.inf).min(axis=1, initial=np.inf)
            margin = np.where((full & np.isnan(ad)).any(axis=1), 0.0, margin)
        self.age += np.where(on, n, 0)
        md = self.disc.modem
        inc, step = self.inc[md], self.step[md]
        out, soft, where = [[] for _ in range(K)], [[] for _ in range(K)], [[] for _ in range(K)]
        half = 1 << 31
        for i in range(n):
            sp = space[:, i]
            a2 = (self.acc + inc) & M32
            strobe = on & (a2 < self.acc)
            self.acc = np.where(on, a2, self.acc)
            for j in np.flatnonzero(strobe):
                b = md[j]
                r = self.frames[j].strobe(bool(sp[j]), self.m + i, float(ad[j, i]), self.lock[b], self.unlock[b], self.rule_b)
                if r:
                    out[j].append(r)
                soft[j].append(d[j, i])
                where[j].append(i)
            tr = on & (sp != self.prev)
            self.acc = np.where(tr, np.where(self.acc < half, self.acc + step, self.acc - step), self.acc)
            self.prev = np.where(on, sp, self.prev)
        if n:
            self.d_last = np.where(on, d[:, n - 1].astype(np.float64), self.d_last)
        self.m += n
        chars = [np.array(c, CHAR) for c in out]
        res = (chars, np.array([c.size for c in chars], np.int64), [np.array(s, d.dtype) for s in soft], margin)
        return res + ([np.array(w, np.int64) for w in where],) if want_strobes else res

    def read(self):
        st = np.zeros(self.nrx, STATUS)
        for name in ("chars", "symbols", "errors", "reframes", "locked", "reg"):
            st[name] = [getattr(f, name) for f in self.frames]
        st["acc"], st["d_last"] = self.acc, self.d_last
        return st


def run_cuts(r, z, cuts=None, before=None):
    """all of z through r in the given batches (default: one); before(i, r) is called ahead of batch i -> (chars: a CHAR
    array per receiver, soft: an array per receiver, margin [nrx], status)"""
    z = np.asarray(z)
    parts, softs, margin, off = [[] for _ in range(r.nrx)], [[] for _ in range(r.nrx)], np.full(r.nrx, np.inf), 0
    for i, b in enumerate(cuts or [z.shape[1]]):
        if before:
            before(i, r)
        chars, _, soft, mg = r.process(z[:, off:off + b])
        for j in range(r.nrx):
            parts[j].append(chars[j])
            softs[j].append(soft[j])
        margin = np.minimum(margin, mg)
        off += b
    assert off == z.shape[1]
    return [np.concatenate(p) for p in parts], [np.concatenate(s) for s in softs], margin, r.read()


def model_d_at(bank, sel, W, z, where):
    """the float32 model's d of receiver j at the samples where[j] of one batch behind zero history: the definition's
    operation sequence (four fmaf per tap, t ascending, each one rounding of the exact double expression; the powers; the
    correctly rounded division) at those samples alone -> an array of float32 per receiver"""
    f = np.float32
    z = np.asarray(z).astype(np.complex64)
    zz = np.concatenate([np.zeros((z.shape[0], W - 1), np.complex64), z], axis=1)
    out = []

    def fma(a, b, c):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f)

    for j, (md, flags) in enumerate(sel):
        pos = np.asarray(where[j], np.int64)
        if not flags & ON or not pos.size:
            out.append(np.zeros(0, f))
            continue
        acc = [np.zeros(pos.size, f) for _ in range(4)]               # M.re, M.im, S.re, S.im
        for t in range(W):
            v = zz[j, pos + (W - 1) - t]
            zr, zi = v.real.astype(f), v.imag.astype(f)
            for k, h in ((0, bank[md][0]), (2, bank[md][1])):
                hr = np.full(pos.size, np.complex64(h[t]).real, f)
                hi = np.full(pos.size, np.complex64(h[t]).imag, f)
                acc[k] = fma(hr, zr, acc[k])
                acc[k] = fma(-hi, zi, acc[k])
                acc[k + 1] = fma(hr, zi, acc[k + 1])
                acc[k + 1] = fma(hi, zr, acc[k + 1])
        pm = fma(acc[1], acc[1], acc[0] * acc[0])
        ps = fma(acc[3], acc[3], acc[2] * acc[2])
        if flags & REVERSE:
            pm, ps = ps, pm
        s = pm + ps
        with np.errstate(invalid="ignore", divide="ignore"):
            out.append(np.where(s > 0, (pm - ps) / np.where(s > 0, s, f(1)), f(0)).astype(f))
    return out


# ---- cuts ---------------------------------------------------------------------------------------------------------------

def cut_lists(n, TT, strobe=None, trans=None, both=None):
    """psk_ref.cut_lists' kinds of cuts for this decoder: batches of 0 and 1 and odd ones; batches that end on and beside
    the kernel's tile seams; forty batches of one sample and the rest; and, given their sample indices, cuts just before,
    on and behind a strobe, on and behind a transition, and on and behind a sample that is both (a cut "on" a sample ends a
    batch with it, one "behind" it begins the next batch with the sample after it)"""
    def fit(sizes):
        out = []
        for b in sizes:
            if sum(out) + b >= n:
                break
            out.append(b)
        return out + [n - sum(out)]
    lists = [fit([0, 1, 2, 30, 0, 31, 63, 64, 65, 1]), fit([TT - 1, 1, 1, 0, TT - 1, TT, 2]), fit([1] * 40)]
    for at in (strobe, trans, both):
        if at is not None and at > 1:
            lists.append(fit([at - 1, 1, 1, 1]))                       # batches end before it, on it, behind it
    return lists


def events(r, z):
    """for a fresh one-receiver reference r and its series z [1, n]: (a strobe's sample, a transition's, one that is both
    or None), each behind the first full window and not the series' last samples"""
    z = np.asarray(z)
    space, _, _ = fsk_ref.FskRef([(r.disc.hm[0], r.disc.hs[0], 1, 5)], [(0, ON)], r.W).discriminate(z[:1])
    tr = np.flatnonzero(space[0, 1:] != space[0, :-1]) + 1
    _, _, _, _, where = r.process(z[:1], want_strobes=True)
    st = where[0]
    lo, hi = r.W + 2, z.shape[1] - 4
    st, tr = st[(st > lo) & (st < hi)], tr[(tr > lo) & (tr < hi)]
    both = np.intersect1d(st, tr)
    return int(st[len(st) // 2]), int(tr[len(tr) // 2]), int(both[0]) if both.size else None


# ---- the parity test's inputs --------------------------------------------------------------------------------------------

PARITY_PHASING = 4
PARITY_CHARS = 12                                                      # 2 (4 + 12) + 6 = 38 slots: 30 character slots behind 4 phasing pairs
PARITY_SNR = 20.0
PARITY_SPS = (16, 8)
PARITY_PPM = 300.0                                                     # the modem's bit is that much longer than the sender's
PARITY_N = 38 * 7 * 16 + 96
SOURCE = "THE QUICK BROWN FOX JUMPS OVER THE LAZY DOG "
SMALL_SEEDS = (9000, 9100, 9200, 9300, 9400, 9500, 9600, 9700, 9800)
FAST_SEEDS = (400, 500, 600, 700, 800, 900, 1000, 1100, 1200)
_INPUTS = {}


def parity_text(j):
    """receiver j's twelve letters: a stretch of SOURCE, from another place for every receiver"""
    return "".join(SOURCE[(5 * j + i) % len(SOURCE)] for i in range(PARITY_CHARS))


def parity_inc(sps):
    """no power of two: the modem's clock runs PARITY_PPM slow against the sender's sps samples per bit (slow, because
    inc may not exceed 2^29 at 8 samples per bit)"""
    return int(round(2.0 ** 32 / sps)) - int(round(2.0 ** 32 / sps * PARITY_PPM * 1e-6))


def parity_row(j, sps, tones, seed, reverse=False, snr=PARITY_SNR):
    """receiver j's series: a lead of 3 + j mod 11 samples of mark, then encode(parity_text(j), 4) at sps samples per bit,
    tones at +-tones cycles per sample (exchanged for a REVERSE receiver), noise 20 dB below the tone"""
    _, bits = encode(parity_text(j), PARITY_PHASING)
    line = keying(bits, sps, lead=3 + j % 11, ppm=0.0, n=PARITY_N)
    mark, space = (tones, -tones) if not reverse else (-tones, tones)
    return two_tone(line, mark, space, snr, seed, PARITY_N)


def bank16(W):
    """16 modems in a window of W >= 16: modems 0 .. 7 at 16 samples per bit (tones +-3/32), 8 .. 15 at 8 (tones +-3/16);
    boxcar pairs with fsk_ref.tailed_modem's small seeded tail behind them, so that every tap of a long window takes part;
    inc no power of two; step 0, inc / 16, inc / 4, inc by b mod 4; lock 3, 0, 2, 4 by (b + b div 4) mod 4; unlock 4"""
    bank = []
    for b in range(16):
        sps = PARITY_SPS[b // 8]
        L = sps
        t = np.arange(W, dtype=np.float64)
        w = (t < L) / float(L)
        f = 3.0 / (2.0 * sps)                                          # +-3/32 at 16, +-3/16 at 8: three cycles apart over a bit
        hm = (w * np.exp(2j * np.pi * f * t)).astype(np.complex64)
        hs = (w * np.exp(-2j * np.pi * f * t)).astype(np.complex64)
        if W > L:
            tail = np.random.default_rng(100 * W + b).uniform(-2e-3, 2e-3, (2, W - L, 2))
            hm[L:] = (tail[0, :, 0] + 1j * tail[0, :, 1]).astype(np.complex64)
            hs[L:] = (tail[1, :, 0] + 1j * tail[1, :, 1]).astype(np.complex64)
        inc = parity_inc(sps)
        bank.append((hm, hs, inc, (0, inc // 16, inc // 4, inc)[b % 4], (3, 0, 2, 4)[(b + b // 4) % 4], 4))
    return bank


def sel16(nrx):
    """receiver j on modem (7 j + 3) mod 16, every fifth REVERSE"""
    return [((7 * j + 3) % 16, ON | (REVERSE if j % 5 == 4 else 0)) for j in range(nrx)]


def parity_inputs(nrx):
    """the rows of sel16's receivers; 1, 5 and 9 receivers are the first rows of one array, whose seeds are chosen so that
    every window leaves those receivers' margins above MARGIN (test_sitor_cpu.py asserts it)"""
    key = 1024 if nrx == 1024 else 9
    if key not in _INPUTS:
        seeds = range(50000, 51024) if key == 1024 else SMALL_SEEDS
        rows = []
        for j, (md, flags) in enumerate(sel16(key)):
            sps = PARITY_SPS[md // 8]
            rows.append(parity_row(j, sps, 3.0 / (2.0 * sps), seeds[j], bool(flags & REVERSE)))
        _INPUTS[key] = np.stack(rows)
    return _INPUTS[key][:nrx]


def fast_inputs(nrx):
    """the rows of the W = 2 case: 8 samples per bit, tones at +-1/4 cycles per sample (a boxcar of two samples of the
    one tone is blind to the other), nine receivers at the most"""
    assert nrx <= 9
    if "fast" not in _INPUTS:
        _INPUTS["fast"] = np.stack([parity_row(j, 8, 0.25, FAST_SEEDS[j], j % 5 == 4) for j in range(9)])
    return _INPUTS["fast"][:nrx]


def case(W, nrx):
    """The parity case of window W for nrx receivers -> (bank, sel, z):
      1    one tap, hm = [1], hs = [0.5]: d = 0.6 for every sample; the odd receivers are REVERSE and read space
           throughout; nothing ever locks, the strobes and soft values are all there is
      2    boxcars of two samples at +-1/4, 8 samples per bit, two modems (step inc / 8 and 0, lock 3 and 0): fast_inputs
      16, 255, 256   bank16(W), sel16(nrx), parity_inputs(nrx)"""
    if W == 1:
        one = np.ones(1, np.complex64)
        return ([(one, 0.5 * one, parity_inc(16), parity_inc(16) // 8, 3, 4)],
                [(0, ON | (REVERSE if j & 1 else 0)) for j in range(nrx)], parity_inputs(nrx))
    if W == 2:
        t = np.arange(2)
        hm, hs = (0.5 * np.exp(2j * np.pi * 0.25 * t)).astype(np.complex64), (0.5 * np.exp(-2j * np.pi * 0.25 * t)).astype(np.complex64)
        inc = parity_inc(8)
        return ([(hm, hs, inc, inc // 8, 3, 4), (hm, hs, inc, 0, 0, 4)],
                [(j % 2, ON | (REVERSE if j % 5 == 4 else 0)) for j in range(nrx)], fast_inputs(nrx))
    return bank16(W), sel16(nrx), parity_inputs(nrx)


def reads(text, want):
    """a receiver has read `want` whole: its text ends with it, but for the U+FFFD of the invalid characters that the
    steady mark behind the transmission gives until the framing unlocks.  What stands in front of it is acquisition: while
    the clock pulls in, a character of the phasing sequence can come out as another of weight four, which no
    constant-ratio check can tell"""
    return text.rstrip("\ufffd").endswith(want)


def case_text(W, j):
    """what receiver j of case(W, .) reads where nothing goes wrong; None: no text is expected"""
    return None if W == 1 else parity_text(j)


# ---- the radio facts' signals -------------------------------------------------------------------------------------------

RADIO_SPS = (16, 40)
RADIO_W = 40
RADIO_SEEDS = 20
RADIO_TEXT = "ZCZC EA12\r\nGALE WARNING NR 345\r\nNNNN"
RADIO_LEADS = (0, 3, 7, 11, 17)
NOISE_DB = 5.0                                                        # the radio facts' noise, dB below the tone (test_sitor_cpu.py)


def radio_case(snr_db, seeds=RADIO_SEEDS, step_div=8, lock=3, ppms=(-200.0, 200.0), sps_list=RADIO_SPS, cut_bits=0):
    """RADIO_TEXT in mode B behind 16 phasing pairs at 170 Hz shift for 100 baud (1.7 bauds): for each of `seeds` seeds,
    each samples-per-bit of sps_list and each clock error of ppms one receiver, its lead one of RADIO_LEADS by the seed,
    noise snr_db below the tone in the sample rate's bandwidth; step = inc / step_div (0: a fixed clock); with cut_bits
    the first cut_bits bits of the transmission are left out (a receiver that joins mid-message).  -> (bank, sel, z)"""
    _, bits = encode(RADIO_TEXT, 16)
    bits = bits[cut_bits:]
    bank = []
    for s in sps_list:
        m = modem(RADIO_W, s, lock=lock)
        bank.append(m[:3] + (m[2] // step_div if step_div else 0, lock, 4))
    n = int((len(bits) + 4) * max(sps_list)) + max(RADIO_LEADS)
    rows, sel = [], []
    for b, sps in enumerate(sps_list):
        f = 1.7 / (2.0 * sps)
        for seed in range(seeds):
            for ppm in ppms:
                line = keying(bits, sps, lead=RADIO_LEADS[seed % len(RADIO_LEADS)], ppm=ppm, n=n)
                rows.append(two_tone(line, f, -f, snr_db, 1000 * sps + 50 * seed + (7 if ppm > 0 else 0), n))
                sel.append((b, ON))
    return bank, sel, np.stack(rows)


# ---- the capacity bounds' input ------------------------------------------------------------------------------------------

def advancing_decisions(bits, inc=1 << 29, step=1 << 29, n=None):
    """The adversarial decision series for a clock with (inc, step): the decision alternates at every sample of a bit's
    first half (acc < 2^31 behind the sample's increment), so the clock is advanced there every time, and holds through
    the second half -- but for one more change, in the second half's first sample, where the next strobe must read the
    other value so that it reads bits[k] (1 = mark).  The strobes lie where the clock's own rule puts them.
    -> (space bool [n], the strobes' samples)"""
    acc, prev, sp, strobes, k = 0, False, [], [], 0
    while k < len(bits) and (n is None or len(sp) < n):
        acc, strobe = clock(acc, inc)
        if strobe:
            strobes.append(len(sp))
            k += 1
        if acc < (1 << 31):
            cur = not prev                                             # a strobe's sample too: it reads the turned value
        else:
            # second half: hold what the strobe's sample will turn into bits[k]; put right on the half's first sample
            hold = bool(bits[k]) if k < len(bits) else prev
            cur = hold if acc - inc < (1 << 31) else prev
        if cur != prev:
            acc = correct(acc, step)
        prev = cur
        sp.append(cur)
    sp = np.array(sp, bool)
    return (sp if n is None else sp[:n]), np.array(strobes, np.int64)


def advancing_case(nbits=220):
    """W = 2, hm = [1/2, 1/2] (it passes a constant), hs = [1/2, -1/2] (an alternation): a real series whose sign turns
    where the decision is space.  inc = step = 2^29, lock 2, unlock 15: D = 4.  The decisions are advancing_decisions' for
    phasing and text.  -> (bank, sel, z [1, n], the decisions)"""
    _, bits = encode("NAVTEX", 6)
    sp, _ = advancing_decisions(list(bits[:nbits]))
    sign = np.where(np.cumsum(sp) % 2 == 0, 1.0, -1.0)
    hm, hs = np.array([0.5, 0.5], np.complex64), np.array([0.5, -0.5], np.complex64)
    return [(hm, hs, 1 << 29, 1 << 29, 2, 15)], [(0, ON)], sign[None, :].astype(np.complex64), sp
