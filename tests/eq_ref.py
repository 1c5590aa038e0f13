"""The equaliser's definition (include/perseus_ddc.h) in numpy float64, vectorised over the receivers and
sequential in m and s: every product, sum and difference is one binary64 operation in the definition's order and grouping,
and the output is rounded once to float32, so the device's outputs and states are compared with these bit for bit.  Also
the section designs once more (the RBJ cookbook and the two one-pole sections, written here independently of the
library's), the design sets the issue measured, and the GPU tests' input series and receiver sets."""
import numpy as np

import adapt_ref as AR

RESTART = 0x1
SECTIONS = (1, 2, 4, 8)
MAX_RX = 1024
F32, F64 = np.float32, np.float64
LOWPASS, HIGHPASS, BANDPASS, NOTCH, PEAK, LOWSHELF, HIGHSHELF, LOWPASS1, HIGHPASS1 = range(9)
KINDS = tuple(range(9))
GROUP = 8                                         # receivers of one wave (csrc/ddc_eq.h, kEqGroup)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int64 if x.dtype == np.float64 else np.int32)


def section_ok(c):
    """all five finite, |a2| < 1, |a1| < 1 + a2"""
    b0, b1, b2, a1, a2 = (float(v) for v in c)
    return bool(np.isfinite([b0, b1, b2, a1, a2]).all() and abs(a2) < 1.0 and abs(a1) < 1.0 + a2)


def design(kind, rate, f, q=0.7071, gain_db=0.0):
    """(b0, b1, b2, a1, a2), a0 = 1"""
    assert kind in KINDS and 0.0 < f < 0.5 * rate and q > 0.0
    if kind in (LOWPASS1, HIGHPASS1):
        k = np.tan(np.pi * f / rate)
        a1 = (k - 1.0) / (k + 1.0)
        return (k / (1.0 + k), k / (1.0 + k), 0.0, a1, 0.0) if kind == LOWPASS1 else (1.0 / (1.0 + k), -1.0 / (1.0 + k), 0.0, a1, 0.0)
    w = 2.0 * np.pi * f / rate
    cs, al, A = np.cos(w), np.sin(w) / (2.0 * q), 10.0 ** (gain_db / 40.0)
    r = 2.0 * np.sqrt(A) * al
    b, a = {
        LOWPASS: (((1 - cs) / 2, 1 - cs, (1 - cs) / 2), (1 + al, -2 * cs, 1 - al)),
        HIGHPASS: (((1 + cs) / 2, -(1 + cs), (1 + cs) / 2), (1 + al, -2 * cs, 1 - al)),
        BANDPASS: ((al, 0.0, -al), (1 + al, -2 * cs, 1 - al)),
        NOTCH: ((1.0, -2 * cs, 1.0), (1 + al, -2 * cs, 1 - al)),
        PEAK: ((1 + al * A, -2 * cs, 1 - al * A), (1 + al / A, -2 * cs, 1 - al / A)),
        LOWSHELF: ((A * ((A + 1) - (A - 1) * cs + r), 2 * A * ((A - 1) - (A + 1) * cs), A * ((A + 1) - (A - 1) * cs - r)),
                   ((A + 1) + (A - 1) * cs + r, -2 * ((A - 1) + (A + 1) * cs), (A + 1) + (A - 1) * cs - r)),
        HIGHSHELF: ((A * ((A + 1) + (A - 1) * cs + r), -2 * A * ((A - 1) + (A + 1) * cs), A * ((A + 1) + (A - 1) * cs - r)),
                    ((A + 1) - (A - 1) * cs + r, 2 * ((A - 1) - (A + 1) * cs), (A + 1) - (A - 1) * cs - r)),
    }[kind]
    return tuple(float(v / a[0]) for v in (b[0], b[1], b[2], a[1], a[2]))


def response(sections, rate, freqs):
    """H(f) of a cascade, complex128"""
    z1 = np.exp(-2j * np.pi * np.asarray(freqs, F64) / rate)
    h = np.ones(z1.shape, np.complex128)
    for b0, b1, b2, a1, a2 in sections:
        h = h * ((b0 + b1 * z1 + b2 * z1 * z1) / (1.0 + a1 * z1 + a2 * z1 * z1))
    return h


class EqRef:
    """streaming: process(x) batch by batch, set_rx between batches, state"""

    def __init__(self, rx, sections, keep_double=False):
        self.keep_double, self.double = keep_double, None           # the last batch's outputs before the rounding
        rx = [[tuple(float(v) for v in c) for c in r] for r in rx]
        K, S = len(rx), int(sections)
        assert 1 <= K <= MAX_RX and S in SECTIONS
        self.K, self.S = K, S
        self.nsec = np.zeros(K, np.int64)
        self.coef = np.zeros((K, S, 5), F64)
        for j, r in enumerate(rx):
            self._set(j, r)
        self.reset()

    def _set(self, j, r):
        if not 0 <= j < self.K or len(r) > self.S or not all(len(c) == 5 and section_ok(c) for c in r):
            raise ValueError("eq_ref: sections")
        self.nsec[j] = len(r)
        self.coef[j] = 0.0
        if r:
            self.coef[j, :len(r)] = np.array(r, F64)

    def reset(self):
        self.state = np.zeros((self.K, self.S, 2), F64)
        self.restart = np.zeros(self.K, bool)

    def set_rx(self, j, sections, flags=0):
        if int(flags) & ~RESTART:
            raise ValueError("eq_ref: flags")
        self._set(j, [tuple(float(v) for v in c) for c in sections])
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
        self.state[self.restart] = 0.0
        self.restart[:] = False
        xd = x.astype(F64)
        yd = np.empty((K, n), F64) if self.keep_double else None
        runs = [self.nsec > s for s in range(self.S)]
        used = [s for s in range(self.S) if runs[s].any()]
        c = [[np.ascontiguousarray(self.coef[:, s, k]) for k in range(5)] for s in range(self.S)]
        s1 = [self.state[:, s, 0].copy() for s in range(self.S)]
        s2 = [self.state[:, s, 1].copy() for s in range(self.S)]
        # non-finite samples are data like any other (include/perseus_ddc.h, "Non-finite samples"): no warnings
        with np.errstate(under="ignore", over="ignore", invalid="ignore"):
            for m in range(n):
                v = xd[:, m]
                for s in used:
                    b0, b1, b2, a1, a2 = c[s]
                    run = runs[s]
                    y = (b0 * v) + s1[s]
                    n1 = ((b1 * v) - (a1 * y)) + s2[s]
                    n2 = (b2 * v) - (a2 * y)
                    s1[s] = np.where(run, n1, s1[s])
                    s2[s] = np.where(run, n2, s2[s])
                    v = np.where(run, y, v)
                out[:, m] = v.astype(F32)
                if self.keep_double:
                    yd[:, m] = v
        self.double = yd
        off = self.nsec == 0
        out.view(np.uint32)[off] = x.view(np.uint32)[off]           # OFF: the words
        for s in range(self.S):
            # sections that did not run are at rest behind a batch
            self.state[:, s, 0] = np.where(runs[s], s1[s], 0.0)
            self.state[:, s, 1] = np.where(runs[s], s2[s], 0.0)
        return out


def eq_ref(x, rx, sections, cuts=None):
    """-> (out, state, the EqRef after the run)"""
    r = EqRef(rx, sections)
    return AR.run_cuts(r, x, cuts), r.state.copy(), r


# ---- the design sets of the issue's measurement ----------------------------------------------------------------------

RATES = (9765.625, 48000.0)


def design_sets():
    """name -> (rate, cascade): the three designs of the float32-against-binary64 table at both rates, and a voice chain
    (high cut, low cut, de-emphasis, two shelves) at both: eight sets"""
    sets = {}
    for rate in RATES:
        tag = f"@{rate:g}"
        sets["notch20" + tag] = (rate, [design(NOTCH, rate, 20.0, 30.0)])
        sets["hum" + tag] = (rate, [design(NOTCH, rate, f, 30.0) for f in (50.0, 100.0, 150.0)])
        sets["cwpeak" + tag] = (rate, [design(PEAK, rate, 700.0, 20.0, 18.0)] * 2)
        sets["voice" + tag] = (rate, [design(HIGHPASS, rate, 300.0), design(LOWPASS, rate, 2700.0), design(LOWPASS1, rate, 1.0 / (2 * np.pi * 750e-6)),
                                      design(LOWSHELF, rate, 400.0, 0.7071, -6.0), design(HIGHSHELF, rate, 2000.0, 0.7071, 4.0)])
    return sets


# ---- the GPU tests' inputs ------------------------------------------------------------------------------------------

K0, N0, FEW = 1024, 3000, 37
ZERO_ROW, SILENT_ROW, SILENT_FROM, DENORMAL_ROW = AR.ZERO_ROW, AR.SILENT_ROW, AR.SILENT_FROM, 21
RATE = RATES[0]


def pool():
    """the single sections the receivers' cascades are drawn from: every kind, the narrow notches and the peak among them"""
    r = RATE
    return [design(NOTCH, r, 20.0, 30.0), design(PEAK, r, 700.0, 20.0, 18.0), design(LOWPASS1, r, 212.2), design(HIGHPASS, r, 300.0),
            design(NOTCH, r, 50.0, 30.0), design(LOWSHELF, r, 400.0, 0.7071, -6.0), design(LOWPASS, r, 2700.0), design(BANDPASS, r, 800.0, 4.0),
            design(HIGHSHELF, r, 2000.0, 0.7071, 4.0), design(HIGHPASS1, r, 100.0), design(NOTCH, r, 1000.0, 10.0)]


def nsec_of(j, S):
    """0 .. S, so that over 8 (S + 1) consecutive receivers every place of a wave's 8 receivers sees every count"""
    return (j % GROUP + j // GROUP) % (S + 1)


def interleaved_rx(K, S, first=0):
    """receiver j: nsec_of(first + j, S) sections, section s the pool's (3 j + s)-th: counts and designs interleaved receiver
    by receiver.  The zero, silent and denormal rows have at least one section."""
    p = pool()
    rx = []
    for j in range(first, first + K):
        ns = nsec_of(j, S)
        if j in (ZERO_ROW, SILENT_ROW, DENORMAL_ROW):
            ns = max(ns, 1)
        rx.append([p[(3 * j + s) % len(p)] for s in range(ns)])
    return rx


def gpu_series():
    """the GPU tests' input, [K0, N0] (the adaptive filter's: tones and noise, a row of zeros, a row that goes silent, two
    tiny rows), with row DENORMAL_ROW scaled so that its values and outputs are float32 denormals"""
    x = AR.audio_series(K0, N0, 33)
    x[DENORMAL_ROW] = (x[DENORMAL_ROW].astype(F64) * 2.0 ** -128).astype(F32)
    return x
