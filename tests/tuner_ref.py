"""The tuner's reference: numpy in double on top of tests/channelizer_ref.py (include/perseus_ddc.h "tuner").
tests/test_tuner_cpu.py pins this restatement against the project's oracle DDC, against the direct sum with the shifted
prototype and against a closed form.  Never the code under test."""
import numpy as np

MASK = 0xFFFFFFFF
CASES_TR = ((1, 1), (64, 4), (512, 64))
# The GPU tolerances.  tests/test_tuner_cpu.py::test_float32_models_against_double measures the independent float32
# models against the double reference (2^19 LCG samples, seed 12345; M in 1024, 4096, both hops, the (T, R) above, Kaiser
# and random h, the receiver set of the GPU parity test, P = 4).  Tuner alone (complex64 rows in): 6.9e-8 .. 8.46e-7; the
# chain channelizer_model_f32 -> tuner model: 1.6e-7 .. 8.86e-7; both worst at M = 1024, D = 512, T = 512 (a float32 sum
# of 512 terms; T = 64: up to 4.6e-7, T = 1: up to 2.0e-7).  TOL = 7 x the worst case of each.
MODEL_WORST_TUNER = 8.46e-7
MODEL_WORST_CHAIN = 8.86e-7
TOL_TUNER = 7 * MODEL_WORST_TUNER               # 5.92e-6
TOL_CHAIN = 7 * MODEL_WORST_CHAIN               # 6.20e-6


def channel_of(nchan, freg):
    """(channel, residue) of a 32-bit word: the nearest centre, wrapping to 0 at the top; residue signed"""
    b = int(nchan).bit_length() - 1
    f = int(freg) & MASK
    k = ((f + (1 << (31 - b))) & MASK) >> (32 - b)
    r = (f - (k << (32 - b))) & MASK
    return k, r - (1 << 32) if r >= 1 << 31 else r


def noutputs_of(nrows, ntaps, decim):
    return (nrows - ntaps) // decim + 1 if nrows >= ntaps else 0


def receiver_set(nchan, nrx, seed=2024):
    """The receivers of the parity tests: every boundary residue on channels 0, 1, M/2 and M - 1, the word that wraps to
    channel 0, two identical words, the rest seeded random"""
    b = int(nchan).bit_length() - 1
    sh, half = 32 - b, 1 << (31 - b)
    words = []
    for k in (0, 1, nchan // 2, nchan - 1):
        for r in (-half, -1, 0, 1, half - 1):
            words.append(((k << sh) + r) & MASK)
    words.append(MASK - 5)                       # above the top channel's upper edge: wraps to channel 0
    words += [0x12345678, 0x12345678]
    rng = np.random.default_rng(seed + nchan)
    words = words[:nrx]
    words += [int(v) for v in rng.integers(0, 1 << 32, max(0, nrx - len(words)), dtype=np.uint64)]
    return words


def kaiser_lowpass(ntaps, decim, beta=8.0):
    """Tuner's tuner_lowpass restated: -6 dB at 0.35 / decim cycles per row, sum 1, rounded once"""
    t = np.arange(ntaps, dtype=np.float64) - (ntaps - 1) / 2.0
    h = np.sinc(2.0 * 0.35 / decim * t) * np.kaiser(ntaps, beta)
    return (h / h.sum()).astype(np.float32)


def random_lowpass(ntaps, seed=None):
    rng = np.random.default_rng(7 * ntaps + 1 if seed is None else seed)
    return rng.uniform(-1.0, 1.0, ntaps).astype(np.float32)


def kaiser_prototype_wide(nchan, taps_per_branch, beta=None):
    """tuner_prototype restated: cutoff fs / M"""
    n = nchan * taps_per_branch
    if beta is None:
        a = 14.36 * 0.8 * taps_per_branch + 7.95
        beta = 0.1102 * (a - 8.7) if a > 50 else 0.5842 * max(a - 21.0, 0.0) ** 0.4 + 0.07886 * max(a - 21.0, 0.0)
    t = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    w = np.sinc(2.0 * t / nchan) * np.kaiser(n, beta)
    return (w / w.sum()).astype(np.float32)


def phase_words(res, phi, hop, rows):
    """theta[s][j] = (r_j (s D) + phi_j) mod 2^32 in exact integers -> uint64 [len(rows), K]"""
    sd = (np.asarray(rows, dtype=np.uint64) * np.uint64(hop)) & np.uint64(MASK)
    r = np.asarray(res, dtype=np.int64).astype(np.uint64) & np.uint64(MASK)          # two's complement
    p = np.asarray(phi, dtype=np.uint64) & np.uint64(MASK)
    return (sd[:, None] * r[None, :] + p[None, :]) & np.uint64(MASK)


def mix(ycols, res, phi, hop, row0=0):
    """z[s][j] = y[s][k_j] exp(-2 pi i theta_j[s] / 2^32): ycols complex128 [rows, K] (the receivers' columns)"""
    th = phase_words(res, phi, hop, row0 + np.arange(ycols.shape[0]))
    return ycols * np.exp(-2j * np.pi * th.astype(np.float64) / 2.0 ** 32)


def fir_decim(z, h, decim):
    """out[m][j] = sum_t h[t] z[m R + T - 1 - t][j], complete windows only -> [outputs, K]"""
    h = np.asarray(h, dtype=np.float64)
    n = noutputs_of(z.shape[0], h.size, decim)
    out = np.zeros((n, z.shape[1]), np.complex128)
    for t in range(h.size):
        out += h[t] * z[h.size - 1 - t:h.size - 1 - t + (n - 1) * decim + 1:decim] if n else 0
    return out


def tuner_ref(y, nchan, hop, words, h, decim, phi=None, row0=0):
    """y complex128 [rows, M] (channelizer_ref's, all channels), the stream's rows from `row0` on -> [K, outputs]"""
    kr = [channel_of(nchan, f) for f in words]
    cols = np.array([k for k, _ in kr])
    res = [r for _, r in kr]
    phi = [0] * len(words) if phi is None else phi
    return fir_decim(mix(y[:, cols], res, phi, hop, row0), h, decim).T


class TunerRef:
    """The streaming definition with retunes, in double: rows are handed over in batches, z is made with the tuning in
    force when a row arrives, phi follows phi' = phi + (F - F') (s0 D)."""

    def __init__(self, nchan, hop, words, h, decim):
        self.nchan, self.hop, self.h, self.decim = nchan, hop, np.asarray(h, np.float64), decim
        self.words = [int(f) & MASK for f in words]
        self.phi = [0] * len(words)
        self.z = np.zeros((0, len(words)), np.complex128)
        self.done = 0                             # outputs delivered

    def set_freq(self, j, f):
        s0 = self.z.shape[0]
        self.phi[j] = (self.phi[j] + (self.words[j] - (int(f) & MASK)) * ((s0 * self.hop) & MASK)) & MASK
        self.words[j] = int(f) & MASK

    def process(self, y):
        kr = [channel_of(self.nchan, f) for f in self.words]
        z = mix(y[:, [k for k, _ in kr]], [r for _, r in kr], self.phi, self.hop, self.z.shape[0])
        self.z = np.concatenate([self.z, z], axis=0)
        out = fir_decim(self.z, self.h, self.decim)[self.done:]
        self.done += out.shape[0]
        return out.T


def tuner_model_f32(ycols64, res, phi, hop, h, decim, row0=0):
    """The INDEPENDENT float32 model: complex64 rows, the phasor from the exact word computed in double and rounded to
    complex64, complex64 product, float32 sum in ascending t.  ycols64 complex64 [rows, K] -> complex64 [K, outputs]"""
    th = phase_words(res, phi, hop, row0 + np.arange(ycols64.shape[0]))
    ph = np.exp(-2j * np.pi * th.astype(np.float64) / 2.0 ** 32).astype(np.complex64)
    z = (ycols64.astype(np.complex64) * ph).astype(np.complex64)
    h32 = np.asarray(h, dtype=np.float32)
    n = noutputs_of(z.shape[0], h32.size, decim)
    acc = np.zeros((n, z.shape[1]), np.complex64)
    for t in range(h32.size):
        if n:
            acc += (h32[t] * z[h32.size - 1 - t:h32.size - 1 - t + (n - 1) * decim + 1:decim]).astype(np.complex64)
    return acc.T


def err(y, ref):
    return float(np.max(np.abs(np.asarray(y, np.complex128) - ref)) / np.max(np.abs(ref)))
