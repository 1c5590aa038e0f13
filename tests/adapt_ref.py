"""The adaptive filter's definition (include/perseus_ddc.h) in numpy float32, vectorised over the receivers
and the taps and sequential in m: every product, sum, difference and quotient is one float32 operation in the definition's
order and grouping, so the device's outputs are compared with these bit for bit.  The tree sum is the halving tree,
v = v[:, :h] + v[:, h:2 * h] level by level (never np.sum).  numpy keeps float32 denormals and divides correctly rounded."""
import numpy as np

OFF, NR, NOTCH = 0, 1, 2
MODES = (OFF, NR, NOTCH)
RESTART = 0x1
TAPS = (16, 32, 64, 128)
MAX_DELAY = 256
EPS = 1.0e-6
F32 = np.float32
TINY = np.finfo(np.float32).tiny                  # the smallest normal float32


def bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def rx_ok(mode, mu, leak, flags=0):
    m, g = F32(mu), F32(leak)
    return int(mode) in MODES and not (int(flags) & ~RESTART) and bool(np.isfinite(m) and np.isfinite(g) and 0 < m < 2 and 0 <= g < 1)


def tree(v):
    """[K, T] -> [K]: for h = T/2 .. 1: v_k = v_k + v_(k+h) for k < h"""
    h = v.shape[1] // 2
    while h >= 1:
        v = v[:, :h] + v[:, h:2 * h]
        h //= 2
    return v[:, 0]


class AdaptRef:
    """streaming: process(x) batch by batch, set_rx between batches, weights"""

    def __init__(self, rx, taps, delay, eps=EPS, count=False):
        rx = [tuple(r) for r in rx]
        self.count = count                                           # count the denormal products (slower)
        K = len(rx)
        assert 1 <= K <= 1024 and taps in TAPS and 1 <= delay <= MAX_DELAY and np.isfinite(F32(eps)) and F32(eps) > 0
        assert all(rx_ok(*r) for r in rx)
        self.K, self.T, self.D, self.eps = K, int(taps), int(delay), F32(eps)
        self.mode = np.array([r[0] for r in rx], np.int64)
        self.mu = np.array([r[1] for r in rx], F32)
        self.lam = (F32(1.0) - np.array([r[2] for r in rx], F32)).astype(F32)
        self.reset()

    def reset(self):
        self.weights = np.zeros((self.K, self.T), F32)
        self.hist = np.zeros((self.K, self.D + self.T - 1), F32)     # the last D + T - 1 inputs, the oldest first
        self.restart = np.zeros(self.K, bool)
        self.denormals = np.zeros(self.K, np.int64)                  # denormal products met (the tests' preconditions)

    def set_rx(self, j, mode, mu, leak, flags=0):
        if not 0 <= j < self.K or not rx_ok(mode, mu, leak, flags):
            raise ValueError("adapt_ref: set_rx")
        self.mode[j], self.mu[j], self.lam[j] = mode, mu, F32(1.0) - F32(leak)
        if flags & RESTART:
            self.restart[j] = True

    def process(self, x):
        """x: float32 [K, n] -> float32 [K, n]"""
        x = np.ascontiguousarray(x, dtype=F32)
        K, n = x.shape
        assert K == self.K
        out = np.empty((K, n), F32)
        if n == 0:
            return out
        # a restart is honoured by the batch that has a sample
        self.weights[self.restart] = 0
        self.restart[:] = False
        H, T, D = self.D + self.T - 1, self.T, self.D
        xx = np.concatenate([self.hist, x], axis=1)                  # xx[:, H + i] is this batch's sample i
        w = self.weights
        on = (self.mode != OFF)[:, None]
        mu, lam, eps = self.mu, self.lam[:, None], self.eps
        # non-finite samples are data like any other (include/perseus_ddc.h, "Non-finite samples"): no warnings
        with np.errstate(under="ignore", over="ignore", invalid="ignore"):
            for i in range(n):
                # u_k = x[m - D - k], k = 0 .. T - 1
                u = xx[:, H + i - D - T + 1:H + i - D + 1][:, ::-1]
                wu, uu = w * u, u * u
                if self.count:
                    self.denormals += np.count_nonzero((wu != 0) & (np.abs(wu) < TINY), axis=1) + np.count_nonzero((uu != 0) & (uu < TINY), axis=1)
                y = tree(wu)
                p = tree(uu)
                e = xx[:, H + i] - y
                g = (mu * e) / (p + eps)
                w = np.where(on, (w * lam) + (g[:, None] * u), w)
                out[:, i] = np.where(self.mode == NR, y, np.where(self.mode == NOTCH, e, xx[:, H + i]))
        self.weights = np.ascontiguousarray(w, dtype=F32)
        self.hist = np.ascontiguousarray(xx[:, n:])
        return out


def adapt_ref(x, rx, taps, delay, eps=EPS, cuts=None, count=False):
    """-> (out, weights, the AdaptRef after the run)"""
    r = AdaptRef(rx, taps, delay, eps, count)
    return run_cuts(r, x, cuts), r.weights.copy(), r


def run_cuts(r, x, cuts=None):
    outs, off = [], 0
    for b in cuts or [x.shape[1]]:
        outs.append(r.process(x[:, off:off + b]))
        off += b
    assert off == x.shape[1]
    return np.concatenate(outs, axis=1)


# ---- the GPU tests' inputs ------------------------------------------------------------------------------------------

MUS = (0.25, 0.5, 1.0, 0.0625, 1.5)
LEAKS = (2.0 ** -10, 0.0, 2.0 ** -6, 2.0 ** -14)
ZERO_ROW, SILENT_ROW, SILENT_FROM, TINY_ROW, TINIER_ROW = 5, 10, 1000, 13, 14      # modes NOTCH, NR, NR, NOTCH


K0, N0 = 1024, 3000
GPU_SETS = ((64, 1), (16, 1), (32, 7), (128, 256), (64, 255))      # (T, D): the first at K0 receivers, the others at 37


def gpu_series():
    """the GPU tests' input, [K0, N0]; the cases with fewer receivers take its first rows"""
    return audio_series(K0, N0, 21)


def interleaved_rx(K):
    """modes, steps and leaks interleaved receiver by receiver: receiver j has mode j mod 3, step MUS[j mod 5] and leak
    LEAKS[j mod 4], so every group of 16 consecutive receivers -- every lane group of a wave -- holds every mode"""
    return [(MODES[j % 3], MUS[j % 5], LEAKS[j % 4]) for j in range(K)]


def audio_series(K, n, seed):
    """[K, n] float32: per receiver one or two tones of seeded frequency, amplitude and phase plus noise of a seeded level;
    row ZERO_ROW is zeros; row SILENT_ROW is zeros from sample SILENT_FROM on (P = 0 then, and the weights decay by the
    leak alone); row TINY_ROW is the series scaled by 2^-70, so that u u and w u are denormal or underflow while x is
    normal; row TINIER_ROW is scaled by 2^-80, so that g u and with it the weights themselves are denormal"""
    rng = np.random.default_rng(seed)
    m = np.arange(n, dtype=np.float64)[None, :]
    f1, f2 = rng.uniform(0.01, 0.45, (K, 1)), rng.uniform(0.01, 0.45, (K, 1))
    a1, a2 = rng.uniform(0.1, 0.8, (K, 1)), rng.uniform(0.0, 0.3, (K, 1)) * (rng.random((K, 1)) < 0.5)
    sigma = 10.0 ** rng.uniform(-3.0, -0.7, (K, 1))
    x = a1 * np.cos(2 * np.pi * f1 * m + rng.uniform(0, 6.28, (K, 1))) + a2 * np.cos(2 * np.pi * f2 * m + rng.uniform(0, 6.28, (K, 1)))
    x = x + sigma * rng.standard_normal((K, n))
    if K > ZERO_ROW:
        x[ZERO_ROW] = 0.0
    if K > SILENT_ROW:
        x[SILENT_ROW, SILENT_FROM:] = 0.0
    if K > TINY_ROW:
        x[TINY_ROW] *= 2.0 ** -70
    if K > TINIER_ROW:
        x[TINIER_ROW] *= 2.0 ** -80
    return x.astype(F32)


def tone_noise(n, seed, f=0.0731, amp=0.5, phase=0.3, sigma=0.05):
    """the CPU tests' input: (tone, noise) in double"""
    m = np.arange(n, dtype=np.float64)
    return amp * np.cos(2 * np.pi * f * m + phase), sigma * np.random.default_rng(seed).standard_normal(n)


def tone_part(x, f, lo=0):
    """amplitude of the component of x[lo:] at the frequency f (cycles per sample): least squares on cos and sin"""
    m = np.arange(lo, len(x), dtype=np.float64)
    A = np.stack([np.cos(2 * np.pi * f * m), np.sin(2 * np.pi * f * m)], axis=1)
    c, *_ = np.linalg.lstsq(A, np.asarray(x[lo:], np.float64), rcond=None)
    return float(np.hypot(c[0], c[1])), A @ c
