"""The carrier stage's reference: numpy, DESIGN.md 8 / include/perseus_ddc.h "carrier" restated.  `CarrierRef()` evaluates
the definition in double, `CarrierRef(f32=True)` the same operation order in float32 (the phasor from the exact word in
double, rounded once; fmaf as one rounding of the exact double sum).  Never the code under test.

The GPU tolerances.  tests/test_carrier_cpu.py::test_float32_model_against_double measures the float32 model against the
double reference on am_carriers(1024, 3000, SEED) -- AM carriers at a nominal 9765.625 outputs per second, amplitude
0.1 .. 0.5, depth 0.2 .. 0.7, tone 300 .. 2500 Hz, offset within +-40 Hz, initial phase within +-0.35 half-turns, noise
sigma 0.003 -- with a 30 Hz loop (damping 0.7071), vmax 0.25, gamma 1/64, the Hilbert filter hilbert(127), every receiver
once in every mode; err = max |u - ref| / max |ref| per receiver, the worst receiver of each mode:
    DSB 6.204e-07   USB 5.539e-07   LSB 5.940e-07   OFF 0 (u is z, bit for bit)
and of what read() returns behind the 3000 outputs: theta 344 units of 2^-32 turns (5.0e-07 rad), freq (v) 4.58e-09 and
err (q) 1.20e-08 half-turns.
TOL = 7 x the worst case of each mode, the margin demod_ref.py and the tuner's tests use: it covers a device atan2f a few
ulp off numpy's.  Never taken from k_carrier.  The status is compared within the same figure as a phase: an error of TOL
in w, relative to |w|, is a rotation by TOL radians, that is TOL / (2 pi) turns for theta and TOL / pi half-turns for
freq and err, which are phases in half-turns (per output, and smoothed).
A narrower loop is looser in float32: v carries its rounding (half an ulp of 0.008 is 4.7e-10 half-turns per output)
until the loop has steered it out, which takes the longer the narrower the loop.  ::test_float32_model_on_the_gpu_receivers
measures the model on the GPU tests' own receivers (10 / 30 / 60 Hz interleaved, L = 3): worst err at 10 Hz 2.755e-06
(0.66 of that mode's TOL), at 30 Hz 5.557e-07, at 60 Hz 2.655e-07; theta 987 units, freq 4.9e-09, err 6.9e-08 half-turns.
The loop's detector wraps at |e| = 1: a last-bit difference there would send the two loops different ways.  The test
inputs keep the double reference's |e| below E_MAX at every sample of every receiver; the tests assert it."""
import numpy as np

MASK = 0xFFFFFFFF
OFF, DSB, USB, LSB = 0, 1, 2, 3
MODES = (OFF, DSB, USB, LSB)
MODE_NAMES = {OFF: "OFF", DSB: "DSB", USB: "USB", LSB: "LSB"}
RATE = 9765.625
PARAMS = dict(vmax=0.25, gamma=1.0 / 64, lock_thr=0.05)
BANDWIDTHS = (10.0, 30.0, 60.0)
E_MAX = 0.75
SEED = 9

MODEL_WORST_CARRIER = {OFF: 0.0, DSB: 6.204e-07, USB: 5.539e-07, LSB: 5.940e-07}
TOL_CARRIER = {k: 7 * v for k, v in MODEL_WORST_CARRIER.items()}

STATUS = np.dtype([("theta", np.uint32), ("freq", np.float32), ("err", np.float32), ("locked", np.uint32)])


def loop_gains(bandwidth_hz, rate_hz=RATE, damping=0.7071):
    """carrier_loop restated: wn = 2 pi bw / rate, kp = 2 damping wn, ki = wn^2"""
    wn = 2.0 * np.pi * bandwidth_hz / rate_hz
    return 2.0 * damping * wn, wn * wn


def hilbert(L, beta=8.0):
    """carrier_hilbert restated: 2 / (pi (k - D)) at odd k - D, 0 at even, under a Kaiser window -> float32 [L]"""
    D = (L - 1) // 2
    h = np.zeros(L)
    for k in range(L):
        if (k - D) % 2:
            h[k] = 2.0 / (np.pi * (k - D))
    return (h * np.kaiser(L, beta)).astype(np.float32)


class CarrierRef:
    """The streaming definition: batches of [K, n] complex values, set_rx between them.  rx: (mode, kp, ki) per receiver,
    h the Hilbert taps.  f32 False: double (parameters and taps are the float32 values the device gets).  f32 True: the
    float32 model.  After process(): self.e [K, n], the detector's output (0 where the loop is off)."""

    def __init__(self, rx, h, vmax, gamma, lock_thr, f32=False):
        self.ft, self.ct = (np.float32, np.complex64) if f32 else (np.float64, np.complex128)
        self.f32 = f32
        ft = self.ft
        self.vmax, self.gamma = ft(np.float32(vmax)), ft(np.float32(gamma))
        self.lock_thr = np.float32(lock_thr)
        self.invpi = np.float32(1.0 / np.pi) if f32 else 1.0 / np.pi
        self.h = np.asarray(h, np.float32).astype(np.float64)
        self.L = self.h.size
        if self.L < 3 or self.L > 255 or not self.L & 1 or not np.all(np.isfinite(self.h)):
            raise ValueError("taps")
        self.K = len(rx)
        for r in rx:
            self._check(*r)
        self.mode = np.array([r[0] for r in rx], np.int64)
        self.kp = np.array([np.float32(r[1]) for r in rx], ft)
        self.ki = np.array([np.float32(r[2]) for r in rx], ft)
        self.reset()

    @staticmethod
    def _check(mode, kp, ki):
        kp, ki = np.float32(kp), np.float32(ki)
        if mode not in MODES or not (0 < kp <= 0.5) or not (0 <= ki <= 0.25):
            raise ValueError((mode, kp, ki))

    def reset(self):
        K = self.K
        self.m = 0
        self.theta = np.zeros(K, np.int64)
        self.v, self.q = np.zeros(K, self.ft), np.zeros(K, self.ft)
        self.hist = np.zeros((K, self.L - 1), self.ct)

    def set_rx(self, j, mode, kp, ki):
        if not 0 <= j < self.K:
            raise ValueError(j)
        self._check(mode, kp, ki)
        if mode != self.mode[j]:
            self.theta[j] = 0
            self.v[j] = self.q[j] = 0
            self.hist[j] = 0
        self.mode[j], self.kp[j], self.ki[j] = mode, np.float32(kp), np.float32(ki)

    def _fma(self, a, b, c):
        if not self.f32:
            return a * b + c
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)

    def process(self, z):
        ft = self.ft
        z = np.asarray(z).astype(self.ct).reshape(self.K, -1)
        n = z.shape[1]
        self.e = np.zeros((self.K, n), ft)
        if n == 0:
            return np.zeros((self.K, 0), self.ct)
        on = self.mode != OFF
        zr, zi = (np.ascontiguousarray(p[on], dtype=ft) for p in (z.real, z.imag))
        kp, ki = self.kp[on], self.ki[on]
        theta, v, q = self.theta[on], self.v[on], self.q[on]
        wr, wi, E = np.zeros(zr.shape, ft), np.zeros(zr.shape, ft), np.zeros(zr.shape, ft)
        # non-finite samples are data like any other (include/perseus_ddc.h, "Non-finite samples"): no warnings
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            for m in range(n if zr.shape[0] else 0):
                ph = np.exp(-2j * np.pi * theta.astype(np.float64) / 2.0 ** 32).astype(self.ct)
                c, s = ph.real.astype(ft), ph.imag.astype(ft)
                x, y = zr[:, m], zi[:, m]
                a = x * c - y * s
                b = x * s + y * c
                e = (np.arctan2(b, a) * self.invpi).astype(ft)
                # fminf / fmaxf, as the header spells them: a NaN operand is dropped, so a NaN e leaves v = -vmax
                v = np.fmin(self.vmax, np.fmax(-self.vmax, self._fma(ki, e, v))).astype(ft)
                step = self._fma(kp, e, v).astype(ft)
                # a NaN step adds 0 to theta (the header's rule; C leaves the conversion of a NaN undefined)
                turn = np.rint(np.where(np.isnan(step), 0.0, step.astype(np.float64)) * 2.0 ** 31).astype(np.int64)
                theta = (theta + turn) & MASK
                q = self._fma(self.gamma, (np.abs(e) - q).astype(ft), q).astype(ft)
                wr[:, m], wi[:, m], E[:, m] = a, b, e
        self.theta[on], self.v[on], self.q[on] = theta, v, q
        self.e[on] = E
        w = z.copy()
        won = np.empty(wr.shape, self.ct)
        won.real, won.imag = wr, wi
        w[on] = won
        u = w.copy()
        ssb = (self.mode == USB) | (self.mode == LSB)
        if np.any(ssb):
            H, D = self.L - 1, (self.L - 1) // 2
            ext = np.concatenate([self.hist[ssb], w[ssb]], axis=1)
            xi = np.ascontiguousarray(ext.imag, dtype=np.float64)
            acc = np.zeros((xi.shape[0], n), ft)
            sign = np.where(self.mode[ssb] == USB, -1.0, 1.0).astype(ft)[:, None]
            dre = np.ascontiguousarray(ext.real[:, H - D:H - D + n], dtype=ft)
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                for k in range(self.L):
                    t = xi[:, H - k:H - k + n] * self.h[k]
                    t += acc
                    acc[...] = t                    # one rounding to ft: fmaf
                re = dre + sign * acc
            # the two parts are put side by side: x + 1j y would make a NaN of y where x is infinite
            us = np.empty(re.shape, self.ct)
            us.real, us.imag = re, ext.imag[:, H - D:H - D + n]
            u[ssb] = us
        self.hist = np.concatenate([self.hist, w], axis=1)[:, n:].copy()
        self.m += n
        return u

    def read(self):
        st = np.zeros(self.K, STATUS)
        st["theta"], st["freq"], st["err"] = self.theta, self.v, self.q
        st["locked"] = st["err"] < self.lock_thr
        return st


def run_cuts(r, z, cuts=None, before=None):
    """all of z through r in the given batches (default: one); before(i, r) is called ahead of batch i"""
    outs, es, off = [], [], 0
    for i, b in enumerate(cuts or [z.shape[1]]):
        if before:
            before(i, r)
        outs.append(r.process(z[:, off:off + b]))
        es.append(r.e)
        off += b
    assert off == z.shape[1]
    r.e = np.concatenate(es, axis=1)
    return np.concatenate(outs, axis=1)


def err_rows(out, ref):
    """max |out - ref| / max |ref| per receiver"""
    d = np.max(np.abs(np.asarray(out, np.complex128) - ref), axis=1)
    return d / np.max(np.abs(ref), axis=1)


def theta_diff(a, b):
    """a - b as signed 32-bit phase words"""
    return ((np.asarray(a, np.int64) - np.asarray(b, np.int64) + (1 << 31)) & MASK) - (1 << 31)


def bits(x):
    """complex64 / float32 -> uint32 view"""
    return np.ascontiguousarray(x).view(np.uint32)


def am_carriers(K, n, seed=SEED, rate=RATE, max_offset=40.0, max_phase=0.35, noise=0.003):
    """K AM carriers beside the tuned frequency: amplitude 0.1 .. 0.5, depth 0.2 .. 0.7, tone 300 .. 2500 Hz, offset within
    +-max_offset Hz, initial phase within +-max_phase half-turns, seeded noise.  -> (complex64 [K, n], the offsets in Hz)"""
    rng = np.random.default_rng(seed)
    off = rng.uniform(-max_offset, max_offset, K)
    p0 = rng.uniform(-max_phase, max_phase, K) * np.pi
    amp = rng.uniform(0.1, 0.5, K)
    tone = rng.uniform(300.0, 2500.0, K)
    dep = rng.uniform(0.2, 0.7, K)
    t = np.arange(n) / rate
    env = amp[:, None] * (1.0 + dep[:, None] * np.cos(2.0 * np.pi * tone[:, None] * t[None, :]))
    z = env * np.exp(1j * (2.0 * np.pi * off[:, None] * t[None, :] + p0[:, None]))
    z = z + noise * (rng.standard_normal((K, n)) + 1j * rng.standard_normal((K, n)))
    return z.astype(np.complex64), off


def interleaved_rx(K):
    """modes and loop bandwidths interleaved receiver by receiver: receiver j has mode j mod 4 and bandwidth (j // 4) mod 3"""
    return [(MODES[j % 4],) + loop_gains(BANDWIDTHS[(j // 4) % 3]) for j in range(K)]
