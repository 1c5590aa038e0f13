"""The audio resampler's reference: numpy, DESIGN.md 8 / include/perseus_ddc.h "audio" restated.  `audio_ref` evaluates
the definition in double with exact integer positions, `audio_model32` the same operation order in float32 (alpha one
float32 division; fmaf as one rounding of the exact double product plus the addend).  Never the code under test.

The GPU tolerance.  tests/test_audio_cpu.py::test_float32_model_against_double measures the float32 model against the
double reference on the GPU parity test's own inputs (parity_inputs: 9 x 700 and 1024 x 300 values, uniform in [-1, 1]),
every ratio of RATIOS with every (P, T) of SHAPES and the prototype parity_prototype gives them; worst |model - ref| per
(P, T) over the ratios and both inputs:
    (32, 1) 2.375e-07   (128, 32) 5.858e-07   (128, 64) 8.590e-07   (1024, 8) 2.661e-07
TOL_AUDIO = 7 x the worst of them, the margin the tuner's and the demodulator's tests use.  Never taken from k_audio."""
import math

import numpy as np

RATIOS = ((3072, 625), (128, 625), (1, 1), (3, 1), (1, 3), (16, 1), (1, 16))
SHAPES = ((32, 1), (128, 32), (128, 64), (1024, 8))
MODEL_WORST_AUDIO = 8.590e-07
TOL_AUDIO = 7 * MODEL_WORST_AUDIO


def outputs(L, M, before, n):
    """ceil((before + n) L / M) - ceil(before L / M) in Python integers"""
    return -((-(before + n) * L) // M) - -((-before * L) // M)


def positions(L, M, P, k0, count):
    """outputs k0 .. k0 + count - 1 -> (n_k, q, u mod L) as int64 arrays, from Python-exact integers"""
    d = math.gcd(L, M)
    L, M = L // d, M // d
    k = np.arange(k0, k0 + count, dtype=object)
    v = k * M
    n, r = v // L, v % L
    u = r * P
    return (np.array(n, dtype=np.int64), np.array(u // L, dtype=np.int64), np.array(u % L, dtype=np.int64)), L


def pcm_ref(y, scale=32767.0):
    """float32 y -> int16: s = y * scale in float32, round half to even, saturate, NaN -> 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.asarray(y, np.float32) * np.float32(scale)
        c = np.clip(np.rint(s), np.float32(-32768.0), np.float32(32767.0))
        return np.where(np.isnan(s), np.float32(0.0), c).astype(np.int16)


class AudioRef:
    """The streaming definition: batches of [nrx, n] real values.  f32 False: double.  f32 True: the float32 model."""

    def __init__(self, nrx, L, M, P, T, g, f32=False):
        d = math.gcd(L, M)
        self.L, self.M, self.P, self.T, self.nrx, self.f32 = L // d, M // d, P, T, nrx, f32
        self.ft = np.float32 if f32 else np.float64
        g = np.asarray(g, np.float32).reshape(-1)
        assert g.size == P * T
        self.g = np.concatenate([g, np.zeros(1, np.float32)]).astype(self.ft)
        self.reset()

    def reset(self):
        self.N, self.k = 0, 0
        self.hist = np.zeros((self.nrx, self.T - 1), self.ft)

    def process(self, x):
        ft, T, P = self.ft, self.T, self.P
        x = np.asarray(x, np.float32).reshape(self.nrx, -1).astype(ft)
        n = x.shape[1]
        count = outputs(self.L, self.M, self.N, n)
        xx = np.concatenate([self.hist, x], axis=1)                 # xx[:, T - 1 + i] = x[N + i]
        (nk, q, rem), L = positions(self.L, self.M, P, self.k, count)
        at = nk - self.N + (T - 1)
        acc = np.zeros((self.nrx, count), ft)
        if self.f32:
            alpha = rem.astype(np.float32) / np.float32(L)
        else:
            alpha = rem.astype(np.float64) / float(L)
        if not self.f32 and self.nrx >= 64:
            # many receivers: the same sum as one product with the [inputs, outputs] matrix of the weights
            W = np.zeros((xx.shape[1], count))
            for t in range(T):
                g0, g1 = self.g[t * P + q], self.g[t * P + q + 1]
                W[at - t, np.arange(count)] = g0 + alpha * (g1 - g0)
            acc = xx @ W
        elif not self.f32:
            for t in range(T):
                g0, g1 = self.g[t * P + q], self.g[t * P + q + 1]
                acc += (g0 + alpha * (g1 - g0))[None, :] * xx[:, at - t]
        else:
            # non-finite samples are data like any other (include/perseus_ddc.h, "Non-finite samples"): no warnings
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                for t in range(T):
                    g0, g1 = self.g[t * P + q], self.g[t * P + q + 1]
                    w = (alpha.astype(np.float64) * (g1 - g0).astype(np.float64) + g0.astype(np.float64)).astype(np.float32)
                    acc = (w.astype(np.float64)[None, :] * xx[:, at - t].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
        self.hist = xx[:, xx.shape[1] - (T - 1):]
        self.N += n
        self.k += count
        return acc


def run_cuts(r, x, cuts=None):
    outs, off = [], 0
    for b in cuts or [x.shape[1]]:
        outs.append(r.process(x[:, off:off + b]))
        off += b
    assert off == x.shape[1]
    return np.concatenate(outs, axis=1)


def audio_ref(x, L, M, P, T, g, cuts=None):
    """x [nrx, n] -> double [nrx, ceil(n L / M)], in the given batches (default: one)"""
    x = np.asarray(x)
    return run_cuts(AudioRef(x.shape[0], L, M, P, T, g), x, cuts)


def audio_model32(x, L, M, P, T, g, cuts=None):
    """the float32 model of the same operation order: float32 [nrx, n] -> float32 [nrx, ceil(n L / M)]"""
    x = np.asarray(x, np.float32)
    return run_cuts(AudioRef(x.shape[0], L, M, P, T, g, f32=True), x, cuts)


def kaiser_audio_prototype(P, T, cutoff, beta=9.0):
    """audio_prototype restated: Kaiser-windowed sinc over P T points, `cutoff` cycles per input sample, sum P"""
    n = P * T
    t = (np.arange(n, dtype=np.float64) - (n - 1) / 2.0) / P
    g = np.sinc(2.0 * cutoff * t) * np.kaiser(n, float(beta))
    return (g * (P / g.sum())).astype(np.float32)


def parity_prototype(L, M, P, T):
    return kaiser_audio_prototype(P, T, 0.45 * min(1.0, L / M))


def parity_inputs(nrx):
    """the GPU parity test's series: uniform in [-1, 1], 700 values per receiver (nrx = 1024: 300); 1, 5 and 9 receivers
    are the first rows of one array"""
    if nrx == 1024:
        return np.random.default_rng(1024).uniform(-1.0, 1.0, (1024, 300)).astype(np.float32)
    assert nrx <= 9
    return np.random.default_rng(9).uniform(-1.0, 1.0, (9, 700)).astype(np.float32)[:nrx]
