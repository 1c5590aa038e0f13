"""The receiver filter's reference: numpy, DESIGN.md 8 / include/perseus_ddc.h "rxfilter" restated.  `RxFilterRef`
evaluates the streaming definition in double, with f32=True the same operation order in float32 (fmaf as one rounding of
the exact double product plus the addend: a float32 product is exact in double, and the sum of it and a float32 rounds
to float32 as the fused operation does, double rounding aside).  Never the code under test.

The GPU tolerance.  tests/test_rxfilter_cpu.py::test_float32_model_against_double measures the float32 model against the
double reference on the GPU parity test's own inputs (parity_inputs: 9 x 700 and 1024 x 300 complex values, re and im
uniform in [-1, 1]) with every (B, T) of SHAPES, the bank parity_bank gives them and receiver j on filter
(7 j + 3) mod B; worst |model - ref| (complex modulus) per (B, T) over both inputs:
    (1, 1) 0.000e+00   (3, 2) 4.215e-08   (4, 64) 7.679e-07   (64, 255) 1.634e-06   (5, 256) 1.415e-06
TOL_RXFILTER = 7 x the worst of them, the margin the tuner's, the demodulator's and the audio tests use.  Never taken from
k_rxfilter."""
import numpy as np

SHAPES = ((1, 1), (3, 2), (4, 64), (64, 255), (5, 256))
MODEL_WORST = {(1, 1): 0.0, (3, 2): 4.215e-08, (4, 64): 7.679e-07, (64, 255): 1.634e-06, (5, 256): 1.415e-06}
MODEL_WORST_RXFILTER = max(MODEL_WORST.values())
TOL_RXFILTER = 7 * MODEL_WORST_RXFILTER
CUTS = [0, 1, 2, 30, 0, 31, 255, 256, 125]


def select(nrx, B):
    """the parity test's filter of receiver j: (7 j + 3) mod B"""
    return [(7 * j + 3) % B for j in range(nrx)]


class RxFilterRef:
    """The streaming definition: batches of [nrx, n] complex values.  f32 False: double.  f32 True: the float32 model."""

    def __init__(self, bank, sel, f32=False):
        b = np.asarray(bank, np.float32)
        assert b.ndim == 2
        self.B, self.T = b.shape
        self.sel = [int(s) for s in sel]
        assert all(0 <= s < self.B for s in self.sel)
        self.nrx, self.f32 = len(self.sel), f32
        self.bank = b.astype(np.float64)                               # float32 values, held in double
        self.reset()

    def reset(self):
        self.m = 0
        self.hist = np.zeros((self.nrx, self.T - 1), np.complex128)     # float32 values where f32

    def set_rx(self, rx, f):
        assert 0 <= rx < self.nrx and 0 <= f < self.B
        self.sel[rx] = int(f)

    def process(self, z):
        T = self.T
        z = np.asarray(z).reshape(self.nrx, -1).astype(np.complex64).astype(np.complex128)
        n = z.shape[1]
        zz = np.concatenate([self.hist, z], axis=1)                    # zz[:, T - 1 + i] = z[m + i]
        h = self.bank[self.sel]                                        # [nrx, T]
        # non-finite samples are data like any other (include/perseus_ddc.h, "Non-finite samples"): no warnings
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            if self.f32:
                re = np.zeros((self.nrx, n), np.float32)
                im = np.zeros((self.nrx, n), np.float32)
                for t in range(T):
                    seg = zz[:, T - 1 - t:T - 1 - t + n]
                    re = (h[:, t:t + 1] * seg.real + re.astype(np.float64)).astype(np.float32)
                    im = (h[:, t:t + 1] * seg.imag + im.astype(np.float64)).astype(np.float32)
                # the taps are real, so the two parts never mix: side by side (re + 1j im would make a NaN of re
                # where im is not finite, and +0 of a re that is -0: the model now keeps that sign, as the device does)
                out = np.empty((self.nrx, n), np.complex128)
                out.real, out.imag = re, im
            else:
                out = np.zeros((self.nrx, n), np.complex128)
                for t in range(T):
                    out += h[:, t:t + 1] * zz[:, T - 1 - t:T - 1 - t + n]
        self.hist = zz[:, zz.shape[1] - (T - 1):]
        self.m += n
        return out


def run_cuts(r, z, cuts=None, before=None):
    """all of z through r in the given batches (default: one); before(i, r) is called ahead of batch i"""
    outs, off = [], 0
    for i, b in enumerate(cuts or [z.shape[1]]):
        if before:
            before(i, r)
        outs.append(r.process(z[:, off:off + b]))
        off += b
    assert off == z.shape[1]
    return np.concatenate(outs, axis=1)


def rxfilter_ref(z, bank, sel, cuts=None):
    """z [nrx, n] -> complex128 [nrx, n]"""
    return run_cuts(RxFilterRef(bank, sel), np.asarray(z), cuts)


def rxfilter_model32(z, bank, sel, cuts=None):
    """the float32 model of the same operation order -> complex128 holding float32 values"""
    return run_cuts(RxFilterRef(bank, sel, f32=True), np.asarray(z), cuts)


def kaiser_bank(rate, half_widths, ntaps, beta=8.0):
    """rxfilter_bank restated: one Kaiser-windowed sinc per half width, fc = half_width / rate, double, sum 1, rounded once"""
    t = np.arange(ntaps, dtype=np.float64) - (ntaps - 1) / 2.0
    rows = [np.sinc(2.0 * (hw / rate) * t) * np.kaiser(ntaps, float(beta)) for hw in half_widths]
    return np.stack([(h / h.sum()).astype(np.float32) for h in rows])


def parity_bank(B, T):
    """B filters of T taps: half widths spread over 0.02 .. 0.45 of the rate"""
    return kaiser_bank(1.0, [0.02 + 0.43 * (f + 1) / B for f in range(B)], T)


def parity_inputs(nrx):
    """the GPU parity test's series: re and im uniform in [-1, 1], 700 values per receiver (nrx = 1024: 300); 1, 5 and 9
    receivers are the first rows of one array"""
    if nrx == 1024:
        v = np.random.default_rng(1024).uniform(-1.0, 1.0, (1024, 300, 2)).astype(np.float32)
    else:
        assert nrx <= 9
        v = np.random.default_rng(9).uniform(-1.0, 1.0, (9, 700, 2)).astype(np.float32)[:nrx]
    return np.ascontiguousarray(v).view(np.complex64)[..., 0]
