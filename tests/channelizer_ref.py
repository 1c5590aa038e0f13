"""The channelizer's reference: numpy in double (include/perseus_ddc.h "channelizer").  The reference project
holds nothing like it; tests/test_channelizer_cpu.py pins this restatement against the project's own oracle DDC and
against closed forms.  Never the code under test."""
import numpy as np

SIZES = (1024, 2048, 4096)
TAPS = (1, 2, 4, 8)
MAX_PROTO = 16384
# The GPU tolerance.  tests/test_channelizer_cpu.py::test_float32_model_against_double measures the independent float32
# model against the double reference (2^19 LCG samples, seed 12345, all 22 (M, P, D), Kaiser and random prototype):
# e = 1.38e-7 .. 1.89e-7, worst at M = 1024, P = 8, D = M with the random prototype.  TOL = 7 x that worst case.
MODEL_WORST = 1.89e-7
TOL = 1.32e-6


def combos():
    """every (M, P, D) with P M <= 16384: 22 of them"""
    return [(m, p, d) for m in SIZES for p in TAPS if p * m <= MAX_PROTO for d in (m, m // 2)]


def nrows_of(length, proto_len, hop):
    return max(0, (length - proto_len) // hop + 1)


def kaiser_prototype(nchan, taps_per_branch, beta=8.0):
    """the documented default (Channelizer's channelizer_prototype), restated: Kaiser-windowed sinc, cutoff fs / (2 M),
    double, sum 1, rounded once"""
    n = nchan * taps_per_branch
    t = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
    w = np.sinc(t / nchan) * np.kaiser(n, beta)
    return (w / w.sum()).astype(np.float32)


def random_prototype(nchan, taps_per_branch, seed=None):
    rng = np.random.default_rng(nchan * 16 + taps_per_branch if seed is None else seed)
    return rng.uniform(0.05, 1.0, nchan * taps_per_branch).astype(np.float32)


def frames_view(x, proto_len, hop):
    n = nrows_of(x.size, proto_len, hop)
    return np.lib.stride_tricks.as_strided(x, shape=(n, proto_len), strides=(hop * x.strides[0], x.strides[0]),
                                           writeable=False)


def row_phase(nchan, hop, rows, dtype=np.complex128):
    """exp(-2 pi i k s D / M), [len(rows), M], from the integer (k s D) mod M"""
    k = np.arange(nchan, dtype=np.int64)
    s = np.asarray(rows, dtype=np.int64)
    e = (k[None, :] * ((s[:, None] * hop) % nchan)) % nchan
    return np.exp(-2j * np.pi * e / nchan).astype(dtype)


def channelizer_ref(x, nchan, hop, proto, row0=0, chunk=512):
    """x complex128 (the stream from the sample of row `row0` on) -> complex128 [rows, M]"""
    w = np.asarray(proto, dtype=np.float64)
    fr = frames_view(np.ascontiguousarray(x), w.size, hop)
    out = np.empty((fr.shape[0], nchan), np.complex128)
    for a in range(0, fr.shape[0], chunk):
        u = (fr[a:a + chunk] * w).reshape(-1, w.size // nchan, nchan).sum(axis=1)
        rows = row0 + np.arange(a, a + u.shape[0])
        out[a:a + chunk] = np.fft.fft(u, axis=1) * row_phase(nchan, hop, rows)
    return out


def channelizer_model_f32(x, nchan, hop, proto, chunk=512):
    """The INDEPENDENT float32 model: complex64 samples, float32 products added over the branches' taps in float32,
    scipy.fft on complex64, the sign of the hop M/2 case exact."""
    import scipy.fft
    w = np.asarray(proto, dtype=np.float32)
    p = w.size // nchan
    fr = frames_view(np.ascontiguousarray(x.astype(np.complex64)), w.size, hop)
    out = np.empty((fr.shape[0], nchan), np.complex64)
    for a in range(0, fr.shape[0], chunk):
        prod = (fr[a:a + chunk] * w).astype(np.complex64).reshape(-1, p, nchan)
        u = prod[:, 0, :].copy()
        for i in range(1, p):
            u += prod[:, i, :]
        rows = np.arange(a, a + u.shape[0])
        out[a:a + chunk] = scipy.fft.fft(u, axis=1) * row_phase(nchan, hop, rows, np.complex64)
    return out


def err(y, ref):
    return float(np.max(np.abs(np.asarray(y, np.complex128) - ref)) / np.max(np.abs(ref)))


# The weak-channel tests: a tone of amplitude 0.7 on one channel's centre and one 80 dB below it on another's, and the
# weak channel's error taken relative to its own reference value, row by row.  WEAK_MODEL_WORST is the independent float32
# model's worst over every (M, P, D) and the WEAK_CASES placements (tests/test_channelizer_cpu.py::test_weak_channel_model
# re-measures it): 1.4e-5 .. 2.67e-4, worst at M = 4096, P = 1, rounded up.  TOL_WEAK_CHAN = 7 x that, the factor of TOL,
# for the same reason; it is never taken from k_channelize.
WEAK_CASES = 8
WEAK_ROWS = 41
WEAK_MODEL_WORST = 2.8e-4
TOL_WEAK_CHAN = 7 * WEAK_MODEL_WORST


def weak_channels(nchan, seed=5):
    """WEAK_CASES pairs (strong channel, weak channel), the first pair fixed, the others seeded.  At least 8 channels apart
    as the scope's pairs are -- in fact at least 5 M / 16: with one tap per branch the Kaiser prototype's side lobes are
    still -109 dB 57 channels from a tone, which puts 0.3 dB of the strong tone into a weak channel there; they fall with
    the third power of the distance, and from 5 M / 16 on they move the weak channel by less than 0.005 dB at every M."""
    rng = np.random.default_rng(seed + nchan)
    pairs = [(nchan // 8 + 3, nchan // 2 + 9)]
    while len(pairs) < WEAK_CASES:
        ks = int(rng.integers(0, nchan))
        pairs.append((ks, (ks + int(rng.integers(5 * nchan // 16, nchan - 5 * nchan // 16 + 1))) % nchan))
    return pairs


def far_channel(nchan, ks, kw):
    """a channel far from both: half the band from the strong one, or a quarter where the weak one sits there"""
    apart = lambda a, b: min((a - b) % nchan, (b - a) % nchan)
    return next(k for k in ((ks + nchan // 2) % nchan, (ks + nchan // 4) % nchan) if apart(k, kw) >= 8)


def weak_packed(O, nchan, taps_per_branch, hop, ks, kw):
    """packed 24-bit samples of 0.7 exp(2 pi i ks n / M) + 0.7e-4 exp(2 pi i kw n / M), P M + 40 hop of them: WEAK_ROWS rows"""
    import spectrum_ref
    n = taps_per_branch * nchan + (WEAK_ROWS - 1) * hop
    return spectrum_ref.tone_packed(O, n, nchan, [(0.7, ks), (0.7e-4, kw)])


def weak_err(y, ref, kw):
    """max over the rows of |y[s, kw] - ref[s, kw]| / |ref[s, kw]|"""
    y, ref = np.asarray(y, np.complex128), np.asarray(ref, np.complex128)
    return float(np.max(np.abs(y[:, kw] - ref[:, kw]) / np.abs(ref[:, kw])))
