"""The squelch's definition (include/perseus_ddc.h) in numpy float32, vectorised over the receivers and
sequential in m: every product, sum and comparison is one float32 operation in the definition's order, so the device's
outputs are compared with these bit for bit.  Block sums are B successive float32 additions (never np.sum); np.fmin and
np.fmax stand for fminf and fmaxf."""
import numpy as np

GATE, RELATIVE = 0x1, 0x2
FLAG_SETS = (0, GATE, RELATIVE, GATE | RELATIVE)
UP = 1.03125                                     # the tests' floor rise per block (exact in float32)
STATUS = np.dtype([("level", np.float32), ("floor", np.float32), ("peak", np.float32), ("open", np.uint32),
                   ("opens", np.uint32)])
F32 = np.float32


def rx_ok(open_thr, close_thr, flags):
    o, c = F32(open_thr), F32(close_thr)
    return not (int(flags) & ~(GATE | RELATIVE)) and bool(np.isfinite(o) and np.isfinite(c) and 0 <= c <= o)


class SquelchRef:
    """streaming: process(z, a) batch by batch, set_rx between batches, read()"""

    def __init__(self, rx, block, attack, hang, ramp, up=1.0):
        rx = [tuple(r) for r in rx]
        K = len(rx)
        assert 1 <= K <= 1024 and 1 <= block <= 4096 and 1 <= attack <= 65535 and 1 <= hang <= 65535 and 1 <= ramp <= 65536
        assert np.isfinite(F32(up)) and F32(up) >= 1 and all(rx_ok(*r) for r in rx)
        self.K, self.B, self.attack, self.hang, self.R, self.up = K, int(block), int(attack), int(hang), int(ramp), F32(up)
        self.invB, self.invR = F32(1.0) / F32(self.B), F32(1.0) / F32(self.R)
        self.othr = np.array([r[0] for r in rx], dtype=F32)
        self.cthr = np.array([r[1] for r in rx], dtype=F32)
        self.flags = np.array([r[2] for r in rx], dtype=np.int64)
        self.reset()

    def reset(self):
        K = self.K
        self.N = 0
        self.s = np.zeros(K, F32)
        self.f = np.full(K, np.inf, F32)
        self.level = np.zeros(K, F32)
        self.peak = np.zeros(K, F32)
        self.open = np.zeros(K, bool)
        self.run = np.zeros(K, np.int64)
        self.opens = np.zeros(K, np.int64)
        self.c = np.where(self.flags & GATE, 0, self.R).astype(np.int64)
        # what the tests' preconditions count
        self.open_events = self.close_events = self.reversals = 0

    def set_rx(self, j, open_thr, close_thr, flags):
        if not 0 <= j < self.K or not rx_ok(open_thr, close_thr, flags):
            raise ValueError("squelch_ref: set_rx")
        self.othr[j], self.cthr[j], self.flags[j] = open_thr, close_thr, flags

    def read(self, clear_peak=False):
        st = np.zeros(self.K, STATUS)
        st["level"], st["floor"], st["peak"], st["open"], st["opens"] = self.level, self.f, self.peak, self.open, self.opens
        if clear_peak:
            self.peak = np.zeros(self.K, F32)
        return st

    def _block_end(self):
        L = self.s * self.invB
        self.s = np.zeros(self.K, F32)
        was = self.open
        rel = (self.flags & RELATIVE) != 0
        with np.errstate(invalid="ignore", over="ignore"):
            self.f = np.where(was, self.f, np.fmin(L, self.f * self.up)).astype(F32)
            to = np.where(rel, self.f * self.othr, self.othr).astype(F32)
            tc = np.where(rel, self.f * self.cthr, self.cthr).astype(F32)
            run_closed = np.where(L >= to, self.run + 1, 0)
            run_open = np.where(~(L >= tc), self.run + 1, 0)
        opening = ~was & (run_closed >= self.attack)
        closing = was & (run_open >= self.hang)
        self.run = np.where(was, run_open, run_closed)
        self.run[opening | closing] = 0
        self.opens = self.opens + opening
        self.open = (was & ~closing) | opening
        self.peak = np.fmax(self.peak, L)
        self.level = L
        gated = (self.flags & GATE) != 0
        self.open_events += int(opening.sum())
        self.close_events += int(closing.sum())
        self.reversals += int(((opening | closing) & gated & (self.c > 0) & (self.c < self.R)).sum())
        return L

    def process(self, z, a):
        """z complex64 [K, n], a float32 [K, n] -> (out float32 [K, n], levels float32 [K, blocks], states uint8)"""
        z = np.asarray(z)
        a = np.asarray(a)
        assert z.dtype == np.complex64 and a.dtype == F32 and z.shape == a.shape and z.shape[0] == self.K
        n = z.shape[1]
        re, im = np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            p = (re * re) + (im * im)                               # float32 products, one float32 sum
        assert p.dtype == F32
        out = np.empty((self.K, n), F32)
        levels, states = [], []
        gated = (self.flags & GATE) != 0
        zero = np.zeros(self.K, F32)
        for i in range(n):
            with np.errstate(invalid="ignore", over="ignore"):
                self.s = self.s + p[:, i]
            rise = self.open | ~gated
            self.c = np.where(rise, np.minimum(self.c + 1, self.R), np.maximum(self.c - 1, 0))
            g = self.c.astype(F32) * self.invR
            ai = a[:, i]
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                out[:, i] = np.where(self.c == self.R, ai, np.where(self.c == 0, zero, ai * g))
            self.N += 1
            if self.N % self.B == 0:
                levels.append(self._block_end())
                states.append(self.open.astype(np.uint8))
        lv = np.stack(levels, axis=1) if levels else np.zeros((self.K, 0), F32)
        stt = np.stack(states, axis=1) if states else np.zeros((self.K, 0), np.uint8)
        return out, lv, stt


def squelch_ref(z64, a32, rx, **params):
    """one shot -> (out, levels, states, status, the SquelchRef)"""
    r = SquelchRef(rx, **params)
    out, lv, st = r.process(z64, a32)
    return out, lv, st, r.read(), r


def run_cuts(ref, z, a, cuts):
    """z, a through ref in batches of the given sizes -> (out, levels, states)"""
    outs, off = [], 0
    for b in cuts:
        outs.append(ref.process(z[:, off:off + b], a[:, off:off + b]))
        off += b
    assert off == z.shape[1]
    return tuple(np.concatenate([o[i] for o in outs], axis=1) for i in range(3))


def keyed_series(K, n, seed):
    """complex64 [K, n]: complex normal noise (unit variance per component) times a per-receiver envelope that steps
    between 0.03 and 1.0 in segments of seeded random length (40 .. 2500 samples); every receiver starts in a random one
    of the two.  All values are finite and p = re re + im im is never subnormal."""
    rng = np.random.default_rng(seed)
    env = np.empty((K, n), F32)
    for j in range(K):
        hi, at = bool(rng.integers(0, 2)), 0
        while at < n:
            ln = int(rng.integers(40, 2501))
            env[j, at:at + ln] = 1.0 if hi else 0.03
            hi, at = not hi, at + ln
    w = rng.standard_normal((K, n, 2), dtype=F32)
    z = np.ascontiguousarray((w[..., 0] + 1j * w[..., 1]).astype(np.complex64) * env)
    p = z.real * z.real + z.imag * z.imag
    assert z.dtype == np.complex64 and np.isfinite(p).all() and p.min() >= np.finfo(F32).tiny
    return z


def audio_series(K, n, seed):
    """seeded random float32 [K, n], standard normal"""
    return np.random.default_rng(seed).standard_normal((K, n), dtype=F32)


def interleaved_rx(K):
    """thresholds and flag sets interleaved receiver by receiver: flag set j mod 4 (all four combinations); absolute
    thresholds between the keyed series' two powers (0.0018 and 2), relative ones as factors of the floor; three
    hysteresis widths, one of them none (close == open)"""
    rx = []
    for j in range(K):
        flags = FLAG_SETS[j % 4]
        v = (j // 4) % 3
        if flags & RELATIVE:
            o, c = (60.0, 20.0) if v == 0 else (35.0, 35.0) if v == 1 else (150.0, 8.0)
        else:
            o, c = (0.5, 0.125) if v == 0 else (0.25, 0.25) if v == 1 else (1.0, 0.03125)
        rx.append((o * (1.0 + (j % 7) / 16.0), c, flags))
    return rx


def param_sets(TT):
    """(B, attack, hang, R) of the GPU parity test; B = 3 cuts a tile into more than 64 segments and leaves a tail in it
    (no B that divides 256 does both); the last one completes no block within 3000 samples"""
    return [(1, 1, 1, 1), (3, 1, 2, 2), (48, 2, 3, 37), (TT, 1, 2, 4096), (1000, 1, 1, 300), (4096, 1, 1, 8)]


def params(B, attack, hang, R, up=UP):
    return dict(block=B, attack=attack, hang=hang, ramp=R, up=up)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == F32 else x
