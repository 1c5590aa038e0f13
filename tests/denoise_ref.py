"""The spectral noise reduction's definition (include/perseus_ddc.h, pddc_denoise_*) restated in numpy: the reference the
tests compare against, never the code under test.

  oneshot()   the whole series at once, frames indexed straight from the definition; double
  Stream      the streaming form: process() / set_rx() batch by batch, carrying what the definition says is carried;
              double by default, and with dtype=np.float32 the independent float32 model (scipy.fft.rfft / irfft on
              float32, the recursion in float32) from which the GPU comparison's tolerance is derived
  rows(), receivers(), changes()   the inputs of the GPU tests, shared with the CPU test that measures MODEL_WORST on them

Parameters reach the device as float32, so the references take every parameter through float32 first: the comparison
measures the arithmetic, not a parameter's rounding.

Tolerance of the GPU comparison.  Metric: max_m |out - ref| / max_m |ref| per row, the worst row with non-zero ref.
MODEL_WORST is that metric for the float32 model against the double reference on the very inputs of the GPU tests,
rounded up; tests/test_denoise_cpu.py re-measures it (and requires it <= 1e-5: above that the inputs are badly chosen).
TOL_DENOISE = 8 x MODEL_WORST, the scope's factor for the same reason: the device's transform is another operation order
of an O(eps log N) algorithm than scipy's.
"""
import numpy as np
import scipy.fft

OFF, NR = 0, 1
RESTART, HOLD = 1, 2

DEFAULTS = dict(smooth=0.3, up=0.02, down=0.3, nmin=1.0e-4, eps=1.0e-20)
RX_DEFAULT = (NR, 2.0, 0.1, 0.98)

MODEL_WORST = 2.0e-6          # measured 1.5e-6 (out, at 1024 / 512; N: 5.1e-7) by test_denoise_cpu.py, rounded up
TOL_DENOISE = 8 * MODEL_WORST

SIZES = [(256, 128, 1024), (256, 64, 37), (512, 256, 37), (512, 128, 37), (1024, 512, 37), (1024, 256, 37)]
N_GPU = 3000


def window(nfft, hop):
    """denoise_window of the package, restated, as the device holds it: float32"""
    i = np.arange(nfft, dtype=np.float64)
    w = np.sqrt(0.5 - 0.5 * np.cos(2.0 * np.pi * (i + 0.5) / nfft))
    return (w / np.sqrt(nfft / (2.0 * hop))).astype(np.float32)


def _f32(v, dtype):
    return dtype(np.float32(v))


class _Rx:
    """the per-receiver settings as columns [K, 1] of `dtype`"""

    def __init__(self, rx, dtype):
        self.dtype = dtype
        K = len(rx)
        self.off = np.zeros((K, 1), bool)
        self.hold = np.zeros((K, 1), bool)
        self.first = np.ones((K, 1), bool)
        self.beta = np.zeros((K, 1), dtype)
        self.gmin = np.zeros((K, 1), dtype)
        self.alpha = np.zeros((K, 1), dtype)
        for j, r in enumerate(rx):
            self.set(j, *r, at_create=True)

    def set(self, j, mode, beta, gmin, alpha, flags=0, at_create=False):
        self.off[j] = mode == OFF
        self.beta[j] = _f32(beta, self.dtype)
        self.gmin[j] = _f32(gmin, self.dtype)
        self.alpha[j] = _f32(alpha, self.dtype)
        self.hold[j] = bool(flags & HOLD)
        if flags & RESTART and not at_create:
            self.first[j] = True


def _frame(X, st, rx, par, dtype):
    """steps 2 - 12 of the definition for one frame of every receiver: X [K, B] complex -> Y; st = [S, N, A] updated"""
    one = dtype(1)
    a, up, down, nmin, eps = (_f32(par[k], dtype) for k in ("smooth", "up", "down", "nmin", "eps"))
    S, N, A = st
    re, im = X.real.astype(dtype), X.imag.astype(dtype)
    with np.errstate(all="ignore"):
        P = re * re + im * im
        S1 = S + a * (P - S)
        r = N + up * N
        r2 = nmin * S1
        r = np.where(r < r2, r2, r)
        N1 = np.where(S1 > N, np.where(r < S1, r, S1), N + down * (S1 - N))
        keep = rx.hold & ~rx.first
        S = np.where(rx.first, P, np.where(keep, S, S1))
        N = np.where(rx.first, P, np.where(keep, N, N1))
        A = np.where(rx.first, dtype(0), A)
        Nb = rx.beta * N + eps
        t = P / Nb - one
        xi = rx.alpha * (A / Nb) + (one - rx.alpha) * np.where(t > 0, t, dtype(0))
        g = xi / (one + xi)
        G = np.where(g > rx.gmin, g, rx.gmin)
        G = np.where(rx.off, one, G).astype(dtype)
        A = (G * G) * P
        Y = G * X
    st[0], st[1], st[2] = S.astype(dtype), N.astype(dtype), A.astype(dtype)
    rx.first[:] = False
    return Y


def _transforms(dtype):
    if dtype is np.float32:
        # scipy keeps float32 (numpy.fft would go through double); irfft carries the 1/nfft
        return (lambda f: scipy.fft.rfft(f, axis=1)), (lambda Y, n: scipy.fft.irfft(Y, n=n, axis=1).astype(np.float32))
    return (lambda f: np.fft.rfft(f, axis=1)), (lambda Y, n: np.fft.irfft(Y, n=n, axis=1))


class Stream:
    """The streaming form.  process(x [K, n]) -> out [K, n]; set_rx() between batches; noise() -> N [K, B]."""

    def __init__(self, nfft, hop, w, rx, dtype=np.float64, **par):
        self.nfft, self.hop, self.dtype = nfft, hop, dtype
        self.par = dict(DEFAULTS, **par)
        self.w = np.asarray(w).astype(dtype)[None, :]
        self.K = K = len(rx)
        self.rx = _Rx(rx, dtype)
        self.fwd, self.inv = _transforms(dtype)
        self.reset()

    def reset(self):
        """everything carried, the first-frame mark included; the receivers' settings stay"""
        K, nfft, hop, dtype = self.K, self.nfft, self.hop, self.dtype
        self.rx.first[:] = True
        B = nfft // 2 + 1
        self.st = [np.zeros((K, B), dtype) for _ in range(3)]
        self.inputs = np.zeros((K, nfft - hop), dtype)     # since the start of the oldest incomplete frame (x[m] = 0, m < 0)
        self.sums = np.zeros((K, nfft), dtype)             # partial overlap sums, from the oldest unfinished y on
        self.ready = np.zeros((K, hop), dtype)             # finished y not yet emitted: out[0 .. hop) = 0
        self.q = 0                                         # frames completed

    def set_rx(self, j, mode, beta, gmin, alpha, flags=0):
        self.rx.set(j, mode, beta, gmin, alpha, flags)

    def noise(self):
        return self.st[1].copy()

    def process(self, x):
        nfft, hop = self.nfft, self.hop
        x = np.asarray(x).astype(self.dtype).reshape(self.K, -1)
        n = x.shape[1]
        self.inputs = np.concatenate([self.inputs, x], axis=1)
        done = [self.ready]
        while self.inputs.shape[1] >= nfft:
            f = self.inputs[:, :nfft] * self.w
            Y = _frame(self.fwd(f), self.st, self.rx, self.par, self.dtype)
            with np.errstate(all="ignore"):
                term = self.inv(Y, nfft) * self.w
                # ascending q, starting from the first term itself: the last hop values are this frame's alone
                self.sums[:, :nfft - hop] = self.sums[:, :nfft - hop] + term[:, :nfft - hop]
            self.sums[:, nfft - hop:] = term[:, nfft - hop:]
            y = self.sums[:, :hop].copy()
            if self.q < nfft // hop - 1:
                y[:] = 0                                   # y[m], m < 0: out[m] = 0 for m < nfft
            done.append(y)
            self.sums[:, :nfft - hop] = self.sums[:, hop:].copy()
            self.inputs = self.inputs[:, hop:]
            self.q += 1
        ready = np.concatenate(done, axis=1)
        out, self.ready = ready[:, :n].copy(), ready[:, n:].copy()
        return out


def oneshot(x, nfft, hop, w, rx, events=(), **par):
    """The whole series at once, double.  events: (position, j, mode, beta, gmin, alpha, flags): a set_rx issued when
    `position` samples had been fed; it governs every frame whose last sample has index >= position.
    -> (out [K, n], N [K, B] after the last complete frame)"""
    par = dict(DEFAULTS, **par)
    x = np.asarray(x, np.float64)
    K, n = x.shape
    wd = np.asarray(w, np.float64)[None, :]
    rxs = _Rx(rx, np.float64)
    st = [np.zeros((K, nfft // 2 + 1)) for _ in range(3)]
    xp = np.concatenate([np.zeros((K, nfft)), x], axis=1)              # xp[:, nfft + m] = x[m]
    y = np.zeros((K, n + 2 * nfft))                                     # y[:, nfft + m]
    events = sorted(events, key=lambda e: e[0])
    e = 0
    for q in range(n // hop):
        last = (q + 1) * hop - 1
        while e < len(events) and events[e][0] <= last:
            rxs.set(*events[e][1:])
            e += 1
        lo = (q + 1) * hop - nfft
        X = np.fft.rfft(xp[:, nfft + lo:nfft + lo + nfft] * wd, axis=1)
        Y = _frame(X, st, rxs, par, np.float64)
        with np.errstate(all="ignore"):
            y[:, nfft + lo:nfft + lo + nfft] += np.fft.irfft(Y, n=nfft, axis=1) * wd
    out = np.zeros((K, n))
    out[:, nfft:] = y[:, nfft:n]                                        # out[m] = y[m - nfft]; only finished y are read
    return out, st[1]


def metric(got, ref):
    """max_m |got - ref| / max_m |ref| per row, the worst row with non-zero ref"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    top = np.abs(ref).max(axis=1)
    rows = top > 0
    return float((np.abs(got - ref).max(axis=1)[rows] / top[rows]).max())


# ---- the inputs of the GPU tests --------------------------------------------------------------------------------------

ZERO_ROW, SILENT_ROW = 5, 6


def rows(K, n=N_GPU, seed=1):
    """[K, n] float32: noise plus keyed, warbling tones at levels spread over 70 dB; row ZERO_ROW is zeros, row SILENT_ROW
    goes silent after 1000 samples.  A row depends on its index alone, so a slice of the many is the few."""
    m = np.arange(n, dtype=np.float64)
    x = np.zeros((K, n), np.float32)
    for j in range(K):
        rng = np.random.default_rng(seed * 100003 + j)
        level = 10.0 ** (-70.0 * (j % 11) / 10.0 / 20.0)
        f0 = 0.02 + 0.4 * rng.random()
        period = 500 + int(400 * rng.random())
        keyed = ((m + rng.integers(0, period)) // period) % 2 == 0
        phase = 2.0 * np.pi * (f0 * m + 3.0 * np.sin(2.0 * np.pi * m / 700.0))
        x[j] = (level * (0.1 * rng.standard_normal(n) + keyed * np.sin(phase))).astype(np.float32)
    if K > ZERO_ROW:
        x[ZERO_ROW] = 0
    if K > SILENT_ROW:
        x[SILENT_ROW, 1000:] = 0
    return x


_RXS = [(NR, 2.0, 0.1, 0.98), (OFF, 2.0, 0.1, 0.98), (NR, 1.0, 0.0, 0.9), (NR, 4.0, 0.25, 0.0), (NR, 3.0, 1.0, 0.5),
        (NR, 2.0, 0.05, 0.98, HOLD), (NR, 1.5, 0.1, 0.7)]


def receivers(K):
    """modes and (beta, gmin, alpha) interleaved row by row; 7 settings against blocks of 4"""
    return [_RXS[j % len(_RXS)] for j in range(K)]


def changes(K):
    """set_rx calls between batches: (position, j, mode, beta, gmin, alpha, flags) -- mode, parameters, HOLD on and off,
    RESTART, on rows spread over the blocks"""
    ev = []
    for j in range(K):
        k = j % 5
        if k == 0:
            ev += [(700, j, OFF, 2.0, 0.1, 0.98, 0), (1900, j, NR, 2.0, 0.1, 0.98, 0)]
        elif k == 1:
            ev += [(1100, j, NR, 3.0, 0.2, 0.5, HOLD), (2300, j, NR, 3.0, 0.2, 0.5, 0)]
        elif k == 2:
            ev += [(1500, j, NR, 2.0, 0.1, 0.98, RESTART)]
        elif k == 3:
            ev += [(700, j, NR, 1.0, 0.3, 0.9, RESTART | HOLD), (1900, j, OFF, 1.0, 0.3, 0.9, HOLD)]
    return ev


CHANGE_POSITIONS = (700, 1100, 1500, 1900, 2300)


def cut_runs(nfft, hop, tile_frames, n=N_GPU):
    """Batch sizes for the cut tests: 0, 1, 2, hop - 1, hop, hop + 1, nfft - 1, nfft, nfft + 1, tile_frames hop -+ 1,
    3 nfft + 5 and the rest.  They are longer than n together at the large sizes, so they come as several runs, each a
    list of batch sizes that sums to n; a size above n (3 nfft + 5 at nfft 1024) is the whole series and drops out."""
    sizes = [0, 1, 2, hop - 1, hop, hop + 1, nfft - 1, nfft, nfft + 1, tile_frames * hop - 1, tile_frames * hop + 1, 3 * nfft + 5]
    runs, cur = [], []
    for b in sizes:
        if b >= n:
            continue
        if sum(cur) + b > n:
            runs.append(cur + [n - sum(cur)])
            cur = []
        cur.append(b)
    runs.append(cur + [n - sum(cur)])
    return runs


def stream_with_changes(K, x, nfft, hop, w, rx, events, cuts, dtype=np.float64):
    """the streaming reference fed x in batches that end at `cuts` (which hold every event's position)"""
    assert {e[0] for e in events} <= set(cuts), "a set_rx falls between batches"
    s = Stream(nfft, hop, w, rx, dtype)
    out, at = [], 0
    for c in sorted(set(cuts) | {x.shape[1]}):
        for e in events:
            if e[0] == at:
                s.set_rx(*e[1:])
        out.append(s.process(x[:, at:c]))
        at = c
    return np.concatenate(out, axis=1), s.noise()
