"""The panorama's reference: numpy in double.  The reference project holds no spectrum arithmetic, so
this restatement IS the definition; tests/test_spectrum_cpu.py pins it against closed forms.  Never the code under test."""
import numpy as np


def hann(n):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)).astype(np.float32)


def nseg_of(length, nfft, hop):
    return max(0, (length - nfft) // hop + 1)


def to_complex(O, packed):
    """packed bytes -> complex128 of the oracle's bit-exact float32 unpack"""
    f = O.unpack24_f32(packed).astype(np.float64)
    return f[0::2] + 1j * f[1::2]


def segments_view(x, nfft, hop):
    n = nseg_of(x.size, nfft, hop)
    return np.lib.stride_tricks.as_strided(x, shape=(n, nfft), strides=(hop * x.strides[0], x.strides[0]), writeable=False)


def spectrum_ref(x, nfft, hop, window, chunk=2048):
    """x complex128 -> (P float64[nfft], M float64[nfft], nseg): fft(x w), abs^2, summed / maxed over the complete segments"""
    w = np.asarray(window, dtype=np.float64)
    segs = segments_view(np.ascontiguousarray(x), nfft, hop)
    P = np.zeros(nfft)
    M = np.zeros(nfft)
    for a in range(0, segs.shape[0], chunk):
        X = np.fft.fft(segs[a:a + chunk] * w, axis=1)
        p = X.real ** 2 + X.imag ** 2
        P += p.sum(axis=0)
        np.maximum(M, p.max(axis=0), out=M)
    return P, M, segs.shape[0]


def spectrum_model_f32(x, nfft, hop, window, rows=None):
    """The INDEPENDENT float32 model: scipy.fft on complex64, float32 powers.  rows None: one float32 running sum over the
    segments; rows = G: the kernel's partial-sum structure -- segment s goes to float32 partial s mod G, the partials are
    then added in double."""
    import scipy.fft
    w = np.asarray(window, dtype=np.float32)
    segs = segments_view(np.ascontiguousarray(x.astype(np.complex64)), nfft, hop)
    n = segs.shape[0]
    if rows is None:
        P = np.zeros(nfft, np.float32)
        for a in range(0, n, 1024):
            X = scipy.fft.fft(segs[a:a + 1024] * w, axis=1)
            p = (X.real * X.real + X.imag * X.imag).astype(np.float32)
            for r in p:
                P += r
        return P.astype(np.float64)
    part = np.zeros((rows, nfft), np.float32)
    assert n % rows == 0 or n < rows
    step = rows if n >= rows else n
    for a in range(0, n, step):
        X = scipy.fft.fft(segs[a:a + step] * w, axis=1)
        part[:step] += (X.real * X.real + X.imag * X.imag).astype(np.float32)
    return part.astype(np.float64).sum(axis=0)


def err(P, Pref):
    return float(np.max(np.abs(np.asarray(P, np.float64) - Pref)) / np.max(Pref))


def tone_packed(O, n, nfft, tones):
    """sum of A exp(+2 pi i k n / nfft) over (A, k) in tones, quantised to 24 bits and packed"""
    t = np.arange(n)
    x = np.zeros(n, complex)
    for a, k in tones:
        x += a * np.exp(2j * np.pi * ((k * t) % nfft) / nfft)
    i = np.clip(np.rint(x.real * 8388607.0), -8388608, 8388607).astype(np.int64)
    q = np.clip(np.rint(x.imag * 8388607.0), -8388608, 8388607).astype(np.int64)
    return O.pack24(i, q).reshape(-1)


def dbfs(P, nseg, window):
    w = np.asarray(window, np.float64)
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(np.asarray(P, np.float64) / (nseg * w.sum() ** 2))


LEVEL_CASES = 8


def level_pairs(nfft, seed=9):
    """The placements of the level tests: LEVEL_CASES pairs (strong bin, weak bin), at least 8 bins apart; the first is
    (floor(0.23 N), N - floor(0.11 N)), the others are seeded"""
    rng = np.random.default_rng(seed + nfft)
    pairs = [(int(0.23 * nfft), nfft - int(0.11 * nfft))]
    while len(pairs) < LEVEL_CASES:
        k1 = int(rng.integers(0, nfft))
        pairs.append((k1, (k1 + int(rng.integers(8, nfft - 8))) % nfft))
    return pairs


def levels(d, k1, k2):
    """dBFS per bin -> (strong bin minus 20 log10(0.9), weak bin minus the level 100 dB below that, the highest bin
    further than 3 from either)"""
    nfft = len(d)
    far = np.ones(nfft, bool)
    for k in (k1, k2):
        far[(k + np.arange(-3, 4)) % nfft] = False
    return d[k1] - 20 * np.log10(0.9), d[k2] - (20 * np.log10(0.9) - 100.0), d[far].max()


def ragged_cuts(total, nfft, seed):
    """batch sizes (multiples of 8) from 8 to 3 nfft samples that add up to `total`"""
    rng = np.random.default_rng(seed)
    cuts, left = [], total
    while left:
        b = int(rng.integers(1, 3 * nfft // 8 + 1)) * 8
        if rng.random() < 0.1:
            b = 8
        b = min(b, left)
        cuts.append(b)
        left -= b
    return cuts
