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

# The shape cases of tests/test_gpu_tuner_shapes.py: every tile regime of k_tune (both group sizes, a move of 0, 1 and
# up to 4088 values between tiles, the full 64 KiB in the 32-receiver form) and the deep windows around s D = 2^31, 2^32.
CASES_TR_SHAPES = ((2, 1), (5, 4), (64, 64), (127, 3), (128, 1), (128, 64), (129, 1), (130, 7), (256, 16), (512, 1), (512, 63))
CASES_DEEP = ((64, 4), (128, 1), (512, 64))
SHAPES_GRID = (1024, 512, 1024 - 20, 64, 8300)  # M, hop, first, count (a range that wraps through channel 0), rows
DEEP_GRID = (4096, 4094, 4)                     # M, first, count
# Their tolerance.  tests/test_tuner_cpu.py::test_float32_model_on_the_shape_cases measures tuner_model_f32 against the
# double reference on the GPU tests' own inputs (gaussian_rows seed 99 rounded to complex64, Kaiser | random h).
# 8300 rows, the 1024 receivers of receiver_set_in:  (2, 1) 9.0e-8 | 1.28e-7, (5, 4) 1.72e-7 | 1.31e-7, (64, 64) 3.26e-7 |
# 3.09e-7, (127, 3) 6.17e-7 | 5.11e-7, (128, 1) 5.55e-7 | 4.64e-7, (128, 64) 4.66e-7 | 4.05e-7, (129, 1) 5.39e-7 | 5.88e-7,
# (130, 7) 6.51e-7 | 6.00e-7, (256, 16) 7.52e-7 | 6.15e-7, (512, 1) 1.430e-6 | 1.007e-6, (512, 63) 9.30e-7 | 8.47e-7.
# Deep windows (M = 4096, 16 receivers, 4096 rows from v - 2048 and w - 2048, hop 4096 and 2048): (64, 4) 3.1e-7 .. 4.5e-7,
# (128, 1) 3.7e-7 .. 5.6e-7, (512, 64) 5.4e-7 .. 1.573e-6 (57 outputs per receiver; random h, hop 4096, the window at w).
# Above TOL_TUNER's 8.46e-7 (Gaussian rows and a T = 512 sum at R = 1), hence a constant of their own.  TOL = 7 x the worst.
MODEL_WORST_TUNER_SHAPES = 1.574e-6
TOL_TUNER_SHAPES = 7 * MODEL_WORST_TUNER_SHAPES  # 1.10e-5


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


def receiver_set_in(nchan, first, count, nrx, seed=2024):
    """Receivers whose channels all lie in the range (first + i) mod nchan, i < count (it may wrap through channel 0):
    every boundary residue on the range's first and last channel and on channel 0 where the range contains it, two
    identical words, the rest seeded random over the range (channel and residue); cut to nrx"""
    b = int(nchan).bit_length() - 1
    sh, half = 32 - b, 1 << (31 - b)
    chans = [first % nchan, (first + count - 1) % nchan]
    if (0 - first) % nchan < count and 0 not in chans:
        chans.append(0)
    words = [((k << sh) + r) & MASK for k in chans for r in (-half, -1, 0, 1, half - 1)]
    rng = np.random.default_rng(seed + 3 * nchan + first)
    n = max(0, nrx - len(words) - 2) + 1
    ks = (first + rng.integers(0, count, n)) % nchan
    rs = rng.integers(-half, half, n)
    rest = [((int(k) << sh) + int(r)) & MASK for k, r in zip(ks, rs)]
    words += [rest[0], rest[0]] + rest[1:]
    return words[:nrx]


def columns_of(nchan, first, words):
    """the column of each word's channel in rows of the range that starts at `first`"""
    return np.array([(channel_of(nchan, f)[0] - first) % nchan for f in words])


def gaussian_rows(nrows, count, seed=99):
    """the seeded Gaussian complex64 rows of the GPU tests (test_gpu_tuner.random_rows) -> numpy complex64 [nrows, count]"""
    import torch
    gen = torch.Generator(device="cpu").manual_seed(seed)
    r = torch.randn((nrows, count, 2), generator=gen, dtype=torch.float32)
    return torch.view_as_complex(r).numpy()


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


def fir_decim_mm(z, h, decim, block=None):
    """fir_decim as matrix products in double: a block of B outputs is the banded matrix H[i][i R + T - 1 - t] = h[t]
    ([B, (B - 1) R + T], built once) times the block's rows of z, real and imaginary parts side by side.  The same sum
    in another order; tests/test_tuner_cpu.py pins it to fir_decim at 1e-13 relative"""
    h = np.asarray(h, dtype=np.float64)
    T = h.size
    n = noutputs_of(z.shape[0], T, decim)
    out = np.zeros((n, z.shape[1]), np.complex128)
    if n == 0:
        return out
    B = min(n, block or max(8, T // decim))
    H = np.zeros((B, (B - 1) * decim + T))
    for i in range(B):
        H[i, i * decim:i * decim + T] = h[::-1]
    zf = np.ascontiguousarray(z, dtype=np.complex128).view(np.float64)               # [rows, 2 K]
    of = out.view(np.float64)
    for m in range(0, n, B):
        c = min(B, n - m)
        of[m:m + c] = H[:c, :(c - 1) * decim + T] @ zf[m * decim:(m + c - 1) * decim + T]
    return out


def tuner_ref_range(rows, nchan, hop, first, words, h, decim, phi=None, row0=0, fir=fir_decim_mm):
    """tuner_ref on the rows of a channel range: rows [S, count] hold the channels (first + i) mod nchan -> [K, outputs]"""
    res = [channel_of(nchan, f)[1] for f in words]
    phi = [0] * len(words) if phi is None else phi
    y = np.asarray(rows)[:, columns_of(nchan, first, words)].astype(np.complex128)
    return fir(mix(y, res, phi, hop, row0), h, decim).T


def tuner_ref(y, nchan, hop, words, h, decim, phi=None, row0=0):
    """y complex128 [rows, M] (channelizer_ref's, all channels), the stream's rows from `row0` on -> [K, outputs]"""
    kr = [channel_of(nchan, f) for f in words]
    cols = np.array([k for k, _ in kr])
    res = [r for _, r in kr]
    phi = [0] * len(words) if phi is None else phi
    return fir_decim(mix(y[:, cols], res, phi, hop, row0), h, decim).T


class TunerRef:
    """The streaming definition with retunes, in double: rows are handed over in batches, z is made with the tuning in
    force when a row arrives, phi follows phi' = phi + (F - F') (s0 D).
    row0: the stream row of the first row it will be handed, with the words and the `phi` in force there; s0 and the
    phase then count from row0 + the rows held, so a window deep in the stream costs only its own rows.  Its output i
    is the window of rows row0 + i R ..: the stream's output row0 / R + i where R divides row0."""

    def __init__(self, nchan, hop, words, h, decim, row0=0, phi=None):
        self.nchan, self.hop, self.h, self.decim = nchan, hop, np.asarray(h, np.float64), decim
        self.words = [int(f) & MASK for f in words]
        self.row0 = int(row0)
        self.phi = [0] * len(words) if phi is None else [int(p) & MASK for p in phi]
        self.z = np.zeros((0, len(words)), np.complex128)
        self.done = 0                             # outputs delivered

    def set_freq(self, j, f):
        s0 = self.row0 + self.z.shape[0]
        self.phi[j] = (self.phi[j] + (self.words[j] - (int(f) & MASK)) * ((s0 * self.hop) & MASK)) & MASK
        self.words[j] = int(f) & MASK

    def process(self, y, first=0):
        """y [rows, M], or the rows of the range that starts at `first`"""
        kr = [channel_of(self.nchan, f) for f in self.words]
        cols = [(k - first) % self.nchan for k, _ in kr]
        z = mix(y[:, cols], [r for _, r in kr], self.phi, self.hop, self.row0 + self.z.shape[0])
        self.z = np.concatenate([self.z, z], axis=0)
        out = fir_decim(self.z, self.h, self.decim)[self.done:]
        self.done += out.shape[0]
        return out.T


def tuner_model_f32(ycols64, res, phi, hop, h, decim, row0=0):
    """The INDEPENDENT float32 model: complex64 rows, the phasor from the exact word computed in double and rounded to
    complex64, complex64 product, float32 sum in ascending t.  ycols64 complex64 [rows, K] -> complex64 [K, outputs]"""
    th = phase_words(res, phi, hop, row0 + np.arange(ycols64.shape[0]))
    ph = np.exp(-2j * np.pi * th.astype(np.float64) / 2.0 ** 32).astype(np.complex64)
    z = np.ascontiguousarray((ycols64.astype(np.complex64) * ph).astype(np.complex64))
    h32 = np.asarray(h, dtype=np.float32)
    T = h32.size
    n = noutputs_of(z.shape[0], T, decim)
    acc = np.zeros((n, z.shape[1]), np.complex64)
    # h is real: the complex64 product h[t] z is the two float32 products, so the sum runs on the float32 pairs, a
    # block of outputs at a time (the same operations in the same order, in cache)
    zf, af = z.view(np.float32), acc.view(np.float32)
    B = max(1, (1 << 19) // max(1, zf.shape[1]))
    for m in range(0, n, B):
        c = min(B, n - m)
        a, tmp = af[m:m + c], np.empty((c, zf.shape[1]), np.float32)
        for t in range(T):
            lo = m * decim + T - 1 - t
            np.multiply(zf[lo:lo + (c - 1) * decim + 1:decim], h32[t], out=tmp)
            a += tmp
    return acc.T


def err(y, ref):
    return float(np.max(np.abs(np.asarray(y, np.complex128) - ref)) / np.max(np.abs(ref)))
