"""The mixer's definition (include/perseus_ddc.h) in numpy float32, vectorised over the samples of a batch
and sequential over the receivers, the chunks and the limiter's blocks: every operation is one float32 operation in the
definition's order, so the device's outputs are compared with these bit for bit.  Never the code under test.

fmaf is ONE rounding of the exact a b + c.  The product of two float32 values is exact in double; the double sum of it
and c is not always, and rounding that sum again can land on the wrong side of a float32 tie (about once in 2^29
operations; a test here runs 10^8 of them).  fma() therefore takes the exact error of the double sum (two-sum) and, where
the double sum lies exactly half-way between two float32 values, lets the error decide.  np.fmin and np.fmax stand for
fminf and fmaxf (a NaN operand is dropped).

The sum is stated per sample: the active set, the numbering p of the active receivers and with it the chunk of every
receiver are arrays over the batch's samples, so nothing here knows how the library cuts a batch."""
import numpy as np

F32, F64 = np.float32, np.float64
STATUS = np.dtype([("peak", F32), ("gain", F32), ("min_gain", F32)])
MAX_RX, MAX_BUS, MAX_RAMP, MIN_BLOCK, MAX_BLOCK = 1024, 8, 65536, 8, 4096


def fma(a, b, c):
    """float32 fmaf(a, b, c), broadcasting: one rounding of the exact value"""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        p = a.astype(F64) * b.astype(F64)               # exact
        c64 = c.astype(F64)
        s = p + c64
        r = s.astype(F32)
        bb = s - p
        e = (p - (s - bb)) + (c64 - bb)                 # exact a b + c == s + e
        d = s - r.astype(F64)                           # exact
        fix = np.isfinite(s) & np.isfinite(r) & (e != 0) & (d != 0)
        if fix.any():
            nb = np.nextafter(r, np.where(d > 0, F32(np.inf), F32(-np.inf)).astype(F32))
            tie = fix & np.isfinite(nb) & (np.abs(d) * 2 == np.abs(nb.astype(F64) - r.astype(F64)))
            r = np.where(tie & ((e > 0) == (d > 0)), nb, r).astype(F32)
    return r


def pcm(out, scale):
    """int16 = clamp(rintf(out * scale), -32768, 32767), NaN -> 0"""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        s = np.asarray(out, F32) * F32(scale)
        c = np.clip(np.rint(s), F32(-32768), F32(32767))
    return np.where(np.isnan(s), F32(0), c).astype(np.int16)


def outputs(Lb, before, n):
    """the limiter's outputs of n samples after `before`"""
    w = lambda N: Lb * max(0, N // Lb - 1)
    return w(before + n) - w(before)


class LimiterRef:
    """streaming, all buses at once: process(y [Q, n]) -> out [Q, count]"""

    def __init__(self, Q, block, ceil, rel):
        assert MIN_BLOCK <= block <= MAX_BLOCK and np.isfinite(F32(ceil)) and F32(ceil) > 0 and 0 < F32(rel) <= 1
        self.Q, self.Lb, self.ceil, self.rel = Q, int(block), F32(ceil), F32(rel)
        self.invLb = F32(1.0) / F32(self.Lb)
        self.reset()

    def reset(self):
        self.held = np.zeros((self.Q, 0), F32)
        self.E = np.ones(self.Q, F32)
        self.min_gain = np.ones(self.Q, F32)
        self.gains = []                                 # E[k] of every block written, for the tests' preconditions
        self.clamped = 0                                # outputs the clamp changed

    def process(self, y):
        Lb, Q = self.Lb, self.Q
        v = np.concatenate([self.held, np.asarray(y, F32)], axis=1)
        cb = v.shape[1] // Lb
        wn = max(cb - 1, 0)
        out = np.zeros((Q, wn * Lb), F32)
        if cb:
            P = np.fmax.reduce(np.abs(v[:, :cb * Lb]).reshape(Q, cb, Lb), axis=2, initial=F32(0))
        frac = np.arange(1, Lb + 1).astype(F32) * self.invLb
        with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
            for k in range(wn):
                m = np.fmax(P[:, k], P[:, k + 1])
                t = np.where(m > self.ceil, self.ceil / np.where(m > self.ceil, m, F32(1)), F32(1)).astype(F32)
                Ep = self.E
                E = np.fmin(t, fma(self.rel, F32(1) - Ep, Ep))
                g = fma((E - Ep)[:, None], frac[None, :], Ep[:, None])
                g[:, Lb - 1] = E
                raw = v[:, k * Lb:(k + 1) * Lb] * g
                o = np.fmin(np.fmax(raw, -self.ceil), self.ceil)
                self.clamped += int((np.abs(raw) > self.ceil).sum())
                out[:, k * Lb:(k + 1) * Lb] = o
                self.E = E
                self.min_gain = np.fmin(self.min_gain, E)
                self.gains.append(E.copy())
        self.held = v[:, wn * Lb:].copy()
        return out


class MixerRef:
    """streaming: process(a) batch by batch, set_rx between batches, read(), reset()"""

    def __init__(self, gains, ramp, limit=None, scale=32767.0, chunk=32):
        g = np.array(gains, dtype=F32, ndmin=2)
        K, Q = g.shape
        assert 1 <= K <= MAX_RX and 1 <= Q <= MAX_BUS and 1 <= ramp <= MAX_RAMP and np.isfinite(g).all()
        assert chunk >= 1 and chunk & (chunk - 1) == 0
        self.K, self.Q, self.R, self.C, self.scale = K, Q, int(ramp), int(chunk), F32(scale)
        self.invR = F32(1.0) / F32(self.R)
        self.to = g.copy()
        self.lim = LimiterRef(Q, *limit) if limit is not None else None
        self.reset()

    def reset(self):
        """the targets stay what the last set_rx made them, taken or not"""
        for j, g in getattr(self, "pending", {}).items():
            self.to[j] = g
        self.pending = {}
        self.frm = self.to.copy()
        self.c = np.full(self.K, self.R, np.int64)
        self.N = 0
        self.peak = np.zeros(self.Q, F32)
        if self.lim:
            self.lim.reset()
        # what the tests' preconditions count
        self.ramps_cut = self.midramp_sets = 0
        self.chunk_counts = set()                       # the chunk counts ceil(active / C) seen, per batch as a tuple

    def set_rx(self, j, gains):
        g = np.asarray(gains, F32).reshape(-1)
        if not 0 <= j < self.K or g.shape != (self.Q,) or not np.isfinite(g).all():
            raise ValueError("mixer_ref: set_rx")
        self.pending[int(j)] = g.copy()                 # the later of two wins

    def gain_now(self, j):
        """the gain the last sample processed was given"""
        if self.c[j] == self.R:
            return self.to[j].copy()
        return fma(self.to[j] - self.frm[j], F32(self.c[j]) * self.invR, self.frm[j])

    def read(self, clear=False):
        st = np.zeros(self.Q, STATUS)
        st["peak"] = self.peak
        st["gain"] = self.lim.E if self.lim else F32(1)
        st["min_gain"] = self.lim.min_gain if self.lim else F32(1)
        if clear:
            self.peak = np.zeros(self.Q, F32)
            if self.lim:
                self.lim.min_gain = np.ones(self.Q, F32)
        return st

    def mix(self, a):
        """a float32 [K, n], n > 0 -> y float32 [Q, n]; moves the ramps"""
        K, Q, R, C = self.K, self.Q, self.R, self.C
        n = a.shape[1]
        for j, g in self.pending.items():
            self.midramp_sets += int(self.c[j] < R)
            self.frm[j] = self.gain_now(j)
            self.to[j] = g
            self.c[j] = 0
        self.pending = {}
        ci = np.minimum(self.c[:, None] + np.arange(1, n + 1)[None, :], R)             # [K, n]
        zero = ~self.to.any(axis=1)                                                       # every to[q] is +-0
        active = ~((ci == R) & zero[:, None])
        p = np.cumsum(active, axis=0) - 1
        nact = active.sum(axis=0)
        nch = (nact + C - 1) // C
        self.chunk_counts.add(tuple(sorted(set(int(v) for v in nch))))
        s = np.zeros((max(int(nch.max()), 1), n, Q), F32)
        every = np.arange(n)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            for j in range(K):
                ii = every if active[j].all() else np.flatnonzero(active[j])
                if not ii.size:
                    continue
                cj = ci[j, ii]
                if (cj == R).all():
                    g = self.to[j][None, :]
                else:
                    t = cj.astype(F32) * self.invR
                    g = fma((self.to[j] - self.frm[j])[None, :], t[:, None], self.frm[j][None, :])
                    g = np.where((cj == R)[:, None], self.to[j][None, :], g)
                mm = p[j, ii] // C
                s[mm, ii] = fma(g, a[j, ii][:, None], s[mm, ii])
            y = s[0].copy()
            for m in range(1, s.shape[0]):
                has = m < nch
                y[has] = (y + s[m])[has]
        self.c = np.minimum(self.c + n, R)
        self.ramps_cut += int((self.c < R).sum())
        self.N += n
        return np.ascontiguousarray(y.T)

    def process(self, a):
        """-> (out float32 [Q, count], pcm int16 [count, Q])"""
        a = np.asarray(a)
        assert a.dtype == F32 and a.ndim == 2 and a.shape[0] == self.K
        if a.shape[1] == 0:
            return np.zeros((self.Q, 0), F32), np.zeros((0, self.Q), np.int16)
        y = self.mix(a)
        self.peak = np.fmax(self.peak, np.fmax.reduce(np.abs(y), axis=1, initial=F32(0)))
        out = self.lim.process(y) if self.lim else y
        return out, np.ascontiguousarray(pcm(out, self.scale).T)


def mixer_ref(a, gains, ramp, limit=None, scale=32767.0, chunk=32, changes=()):
    """one shot, the set_rx calls `changes` [(j, gains)] ahead of the batch -> (out, pcm, status, the MixerRef)"""
    r = MixerRef(gains, ramp, limit, scale, chunk)
    for j, g in changes:
        r.set_rx(j, g)
    out, p = r.process(a)
    return out, p, r.read(), r


def run_cuts(ref, a, cuts, before=None):
    """a through ref in batches of the given sizes -> (out, pcm); before(i, ref) is called ahead of batch i"""
    outs, off = [], 0
    for i, b in enumerate(cuts):
        if before:
            before(i, ref)
        outs.append(ref.process(a[:, off:off + b]))
        off += b
    assert off == a.shape[1]
    return np.concatenate([o[0] for o in outs], axis=1), np.concatenate([o[1] for o in outs], axis=0)


# ---- the tests' inputs ----------------------------------------------------------------------------------------------

SERIES_SEED = 31
CEIL, REL = 1.75, 0.5                             # the tests' ceiling and release (exact in float32)
BLOCKS = (8, 48, 1000, 4096)
RAMPS = (1, 37, 4000)


def interleaved_gains(K, Q, seed=5):
    """[K, Q] float32: receiver j is silent for j mod 3 == 2 (all zero, every other one of them -0), else seeded values
    of both signs in +-(0.25 .. 1) / sqrt(the active count), so that a bus of unit-normal series has a deviation of
    about 0.65 whatever K is; one bus of every fifth active receiver is exactly 0 (it feeds the others only)"""
    rng = np.random.default_rng(seed + 1000 * Q + K)
    act = max(1, K - K // 3)
    g = (rng.uniform(0.25, 1.0, (K, Q)) * rng.choice([-1.0, 1.0], (K, Q)) / np.sqrt(act)).astype(F32)
    for j in range(K):
        if j % 3 == 2:
            g[j] = -0.0 if j % 2 else 0.0
        elif j % 5 == 0 and Q > 1:
            g[j, j % Q] = 0.0
    return g


def one_shot_changes(K, Q, gains):
    """the set_rx calls ahead of the one-shot batch: every seventh receiver gets other gains (active ones ramp, silent
    ones come in), every eleventh goes to zero (it is silent from the sample where its ramp ends)"""
    other = interleaved_gains(K + 3, Q, seed=77)[3:]
    ch = []
    for j in range(K):
        if j % 11 == 4:
            ch.append((j, np.zeros(Q, F32)))
        elif j % 7 == 1:
            ch.append((j, other[j] if other[j].any() else gains[(j + 1) % K]))
    return ch


# the set_rx scenario of the GPU test: K receivers, 47 of them active at first
SCN_K, SCN_Q, SCN_R, SCN_CUTS = 70, 2, 400, (700, 1, 999, 1300)


def scenario_changes(gains):
    """{batch index: [(j, gains)]}: ahead of batch 1 (one sample long: the ramp is cut by a batch boundary at c = 1)
    three receivers change; ahead of batch 2 one of them changes again (mid-ramp), one twice (the later wins), sixteen
    active ones go to zero (silent from sample R - 1 of that batch: 47 -> 31 active, across C = 32) and a silent one
    comes in; ahead of batch 3 two of the sixteen come back and a silent one is set to zero again (it stays silent)"""
    K, Q = gains.shape
    rows = interleaved_gains(K + 5, Q, seed=91)[5:]
    other = [next(rows[(k + d) % K] for d in range(K) if rows[(k + d) % K].any()) for k in range(K)]      # no all-zero row among them
    z = np.zeros(Q, F32)
    down = [j for j in range(K) if j % 3 != 2][10:26]
    assert len(down) == 16
    return {1: [(0, other[0]), (4, other[4]), (9, other[9])],
            2: [(4, other[1]), (9, other[3]), (9, other[6])] + [(j, z) for j in down] + [(2, other[7])],
            3: [(down[0], gains[down[0]]), (down[5], other[down[5]]), (5, z)]}


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == F32 else x
