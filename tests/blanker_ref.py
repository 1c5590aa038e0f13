"""The noise blanker's definition (include/perseus_ddc.h) in numpy float32, vectorised over the receivers and
sequential in m: every product, sum and comparison is one float32 operation in the definition's order, so the device's
outputs are compared with these bit for bit.  Block sums are B successive float32 additions (never np.sum); np.fmin
stands for fminf.  The gate is integer arithmetic on the trigger bits: the distance to the nearest trigger on either side
from running maxima / minima of the triggers' positions."""
import numpy as np

ON = 0x1
BETA, CAP = 0.25, 2.0                            # the tests' smoothing and largest rise per block (exact in float32)
STATUS = np.dtype([("ref", np.float32), ("triggers", np.uint32), ("blanked", np.uint32)])
F32 = np.float32
FAR = 1 << 40


def rx_ok(thr, flags):
    t = F32(thr)
    return not (int(flags) & ~ON) and bool(np.isfinite(t) and t > 0)


class BlankerRef:
    """streaming: process(z) batch by batch, set_rx between batches, read().  After process(): `t` (bool [K, n], the
    batch's triggers), `refs` (float32 [K, n], ref as sample i's trigger test saw it), `dist` (int [K, n], output i's
    distance to the nearest trigger, D + 1 for none)."""

    def __init__(self, rx, block, guard, ramp, beta=BETA, cap=CAP):
        rx = [tuple(r) for r in rx]
        K = len(rx)
        assert 1 <= K <= 1024 and 1 <= block <= 4096 and 0 <= guard <= 128 and 0 <= ramp <= 128
        assert np.isfinite(F32(beta)) and 0 < F32(beta) <= 1 and np.isfinite(F32(cap)) and F32(cap) >= 1
        assert all(rx_ok(*r) for r in rx)
        self.K, self.B, self.W, self.R, self.D = K, int(block), int(guard), int(ramp), int(guard) + int(ramp)
        self.beta, self.cap = F32(beta), F32(cap)
        self.invB, self.invR1 = F32(1.0) / F32(self.B), F32(1.0) / F32(self.R + 1)
        self.thr = np.array([r[0] for r in rx], dtype=F32)
        self.flags = np.array([r[1] for r in rx], dtype=np.int64)
        self.reset()

    def reset(self):
        K, D = self.K, self.D
        self.N = 0
        self.s = np.zeros(K, F32)
        self.ref = np.zeros(K, F32)
        self.triggers = np.zeros(K, np.int64)
        self.blanked = np.zeros(K, np.int64)
        self.hist = np.zeros((K, D), np.complex64)           # the last D inputs
        self.tbits = np.zeros((K, 2 * D), bool)              # the triggers of the last 2 D inputs

    def set_rx(self, j, thr, flags):
        if not 0 <= j < self.K or not rx_ok(thr, flags):
            raise ValueError("blanker_ref: set_rx")
        self.thr[j], self.flags[j] = thr, flags

    def read(self):
        st = np.zeros(self.K, STATUS)
        st["ref"], st["triggers"], st["blanked"] = self.ref, self.triggers % (1 << 32), self.blanked % (1 << 32)
        return st

    def _block_end(self):
        L = self.s * self.invB
        self.s = np.zeros(self.K, F32)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            x = np.fmin(L, self.ref * self.cap)
            d = x - self.ref
            moved = self.ref + (self.beta * d)
            self.ref = np.where(self.ref > 0, moved, L).astype(F32)

    def process(self, z):
        """z complex64 [K, n] -> out complex64 [K, n]: output i is input i - D of the stream"""
        z = np.asarray(z)
        assert z.dtype == np.complex64 and z.ndim == 2 and z.shape[0] == self.K
        K, D, W, n = self.K, self.D, self.W, z.shape[1]
        re, im = np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            p = (re * re) + (im * im)                               # float32 products, one float32 sum
        assert p.dtype == F32
        t = np.zeros((K, n), bool)
        refs = np.zeros((K, n), F32)
        on = (self.flags & ON) != 0
        for i in range(n):
            pi = p[:, i]
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                self.s = self.s + pi
                t[:, i] = on & (self.ref > 0) & (pi > self.ref * self.thr)
            refs[:, i] = self.ref
            self.N += 1
            if self.N % self.B == 0:
                self._block_end()
        self.triggers = self.triggers + t.sum(axis=1)
        # the gate: T's column q is input N0 - 2 D + q, Z's column q input N0 - D + q; output i has its centre at T's
        # column D + i and its source at Z's column i
        T = np.concatenate([self.tbits, t], axis=1)
        Z = np.concatenate([self.hist, z], axis=1)
        pos = np.arange(T.shape[1], dtype=np.int64)
        last = np.maximum.accumulate(np.where(T, pos, -FAR), axis=1)
        nxt = np.minimum.accumulate(np.where(T, pos, FAR)[:, ::-1], axis=1)[:, ::-1]
        pc = D + np.arange(n, dtype=np.int64)
        dist = np.minimum(np.minimum(pc - last[:, pc], nxt[:, pc] - pc), D + 1)
        src = Z[:, :n]
        g = (dist - W).astype(F32) * self.invR1
        zero = np.zeros((K, n), F32)
        out = np.empty((K, n), np.complex64)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            out.real = np.where(dist > D, src.real, np.where(dist <= W, zero, src.real * g))
            out.imag = np.where(dist > D, src.imag, np.where(dist <= W, zero, src.imag * g))
        self.blanked = self.blanked + (dist <= D).sum(axis=1)
        self.tbits = np.ascontiguousarray(T[:, T.shape[1] - 2 * D:])
        self.hist = np.ascontiguousarray(Z[:, Z.shape[1] - D:])
        self.t, self.refs, self.dist = t, refs, dist
        return out


def blanker_ref(z64, rx, **params):
    """one shot -> (out, status, the BlankerRef)"""
    r = BlankerRef(rx, **params)
    out = r.process(z64)
    return out, r.read(), r


def run_cuts(ref, z, cuts):
    """z through ref in batches of the given sizes -> out"""
    outs, off = [], 0
    for b in cuts:
        outs.append(ref.process(z[:, off:off + b]))
        off += b
    assert off == z.shape[1]
    return np.concatenate(outs, axis=1)


def impulse_series(K, n, seed):
    """complex64 [K, n]: complex normal noise (unit variance per component, mean power 2) with seeded bursts per
    receiver: 1 .. 5 consecutive samples of 8 .. 60 times the noise's rms amplitude and random phase, the bursts' starts
    3 .. 700 samples apart.  All values are finite and p = re re + im im is never subnormal."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((K, n, 2), dtype=F32)
    z = np.ascontiguousarray((w[..., 0] + 1j * w[..., 1]).astype(np.complex64))
    for j in range(K):
        starts = np.cumsum(rng.integers(3, 701, size=n // 3 + 1))
        starts = starts[starts < n]
        lens = rng.integers(1, 6, size=starts.size)
        amps = rng.uniform(8.0, 60.0, size=starts.size) * np.sqrt(2.0)
        phases = rng.uniform(0.0, 2.0 * np.pi, size=(starts.size, 5))
        for at, ln, amp, ph in zip(starts, lens, amps, phases):
            seg = z[j, at:at + ln]
            seg[:] = (amp * np.exp(1j * ph[:seg.size])).astype(np.complex64)
    p = z.real * z.real + z.imag * z.imag
    assert z.dtype == np.complex64 and np.isfinite(p).all() and p.min() >= np.finfo(F32).tiny
    return z


THRESHOLDS = (8.0, 12.0, 16.0, 24.0, 40.0, 64.0)


def interleaved_rx(K):
    """ON and OFF receivers interleaved -- every third one is OFF, so the four receivers of a block of the kernel's walk
    hold every mix --, six thresholds between 8 and 64"""
    return [(THRESHOLDS[(j // 3) % 6], 0 if j % 3 == 2 else ON) for j in range(K)]


def param_sets(TT):
    """(B, W, R) of the GPU parity test: D = 8; B = 1 with D = 1; B = 3, which cuts a tile into more than 64 segments and
    leaves a tail in it (no B that divides 256 does both), with D = 2; D = 0; no guard; the largest D; the last one
    completes no block within 3000 samples, so nothing triggers and out is the delayed input"""
    return [(48, 3, 5), (1, 1, 0), (3, 1, 1), (TT, 0, 0), (64, 0, 7), (1000, 128, 128), (4096, 2, 2)]


# the GPU tests' inputs (tests/test_gpu_blanker.py; their preconditions are asserted in tests/test_blanker_cpu.py)
GPU_K, GPU_N, GPU_SEED = 1024, 3000, 21
CUT_SETS = ((48, 3, 5), (1000, 128, 128))


def gpu_cuts(TT, D, n):
    """the batch sizes of the GPU cut test: 0, 1, 2, D - 1, D, 2 D + 1, TT - 1, TT, TT + 1, 3 TT + 5 and the rest"""
    cuts = [0, 1, 2, max(D - 1, 0), D, 2 * D + 1, TT - 1, TT, TT + 1, 3 * TT + 5]
    cuts.append(n - sum(cuts))
    assert cuts[-1] > 0
    return cuts


def params(B, W, R, beta=BETA, cap=CAP):
    return dict(block=B, guard=W, ramp=R, beta=beta, cap=cap)


def bits(x):
    x = np.ascontiguousarray(x)
    if x.dtype == np.complex64:
        return x.view(np.int32)
    return x.view(np.int32) if x.dtype == F32 else x
