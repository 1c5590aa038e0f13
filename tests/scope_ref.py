"""The scope's reference: numpy in double (include/perseus_ddc.h, "scope").  The reference project holds no spectrum
arithmetic, so this restatement IS the definition; tests/test_scope_cpu.py pins it against closed forms.  Never the code
under test.

Tolerance.  The device's transform differs from any host library's in radix order and contraction, so the GPU tests
compare with the double reference within a bound that comes from an INDEPENDENT float32 model (scipy.fft on complex64,
float32 powers, float32 sequential line sums) on the very inputs the GPU tests use.  Metric: max_k |line - ref| / max_k
ref per line, the worst line.  Measured (tests/test_scope_cpu.py::test_float32_model_against_double re-measures them):
    256 / 128 / 4   1.92e-7     512 / 384 / 3    2.17e-7     256 / 16 / 1     2.75e-7
    1024 / 1024 / 1 2.87e-7     2048 / 512 / 2   2.81e-7     4096 / 1024 / 2  2.59e-7     1024 / 512 / 2  2.51e-7
MODEL_WORST is the worst of them, rounded up; TOL_SCOPE = TOL_FACTOR x MODEL_WORST = 2.4e-6 -- both errors are
O(eps log N), the factor covers the different operation order --, below the panorama's 1e-5.
For the weak-tone test the bound is taken relative to the weak bin's own reference value instead, over WEAK_CASES tone
placements per size (the rounding noise a strong bin-centred tone leaves in a far bin depends on the two bins).  The
model's worst there is WEAK_MODEL_WORST[nfft], 2.70e-4 at 256, 3.39e-4 at 512, 1.50e-4 at 1024, 3.50e-5 at 2048 and
8.33e-5 at 4096, rounded up (re-measured by test_weak_tone_model), and the same factor holds:
TOL_WEAK[nfft] = 8 x that.  In dB this is 10 log10(1 + TOL_WEAK) <= 0.02 dB on the weak bin and nothing to speak of on
the strong one; rounding the two amplitudes to float32 moves the reference's own distance by up to 0.002 dB: DB_MARGIN = 0.05."""
import numpy as np

F32 = np.float32
TOL_FACTOR = 8
MODEL_WORST = 3.0e-7
TOL_SCOPE = TOL_FACTOR * MODEL_WORST
WEAK_MODEL_WORST = {256: 3.0e-4, 512: 3.5e-4, 1024: 1.6e-4, 2048: 3.6e-5, 4096: 8.5e-5}
TOL_WEAK = {k: TOL_FACTOR * v for k, v in WEAK_MODEL_WORST.items()}
DB_MARGIN = 0.05

NSRC = 64
# (nfft, hop, avg, slots) of the parity test; CUT_SIZES are those of the bit-exact tests: every FramePlan, 512 the one
# 8 x 8 x 8 plan, 2048 and 4096 the ones whose block is 2 and 4 waves
SIZES = [(256, 128, 4, 1024), (512, 384, 3, 1024), (256, 16, 1, 1024), (1024, 1024, 1, 1024), (2048, 512, 2, 16),
         (4096, 1024, 2, 16)]
CUT_SIZES = [(256, 128, 4), (1024, 512, 2), (512, 384, 3), (2048, 512, 2), (4096, 1024, 2)]


def hann(n):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)).astype(F32)


def nseg_of(length, nfft, hop):
    return max(0, (length - nfft) // hop + 1)


def nlines_of(length, nfft, hop, avg):
    return nseg_of(length, nfft, hop) // avg


def gpu_len(nfft, hop, avg):
    """6 lines and, where a line has more than one segment, half a line more, then a third of a hop"""
    nseg = 6 * avg + avg // 2
    return (nseg - 1) * hop + nfft + hop // 3 + 1


def gpu_series(nfft, hop, avg, nsrc=NSRC, seed=77):
    """The GPU tests' input, complex64 [nsrc, n]: complex noise of sigma 0.1 per component plus two tones per row, one
    of amplitude 0.7 and one 80 dB below it, at frequencies that differ from row to row (none on a bin centre)."""
    n = gpu_len(nfft, hop, avg)
    rng = np.random.default_rng(seed + nfft + hop)
    z = 0.1 * (rng.standard_normal((nsrc, n)) + 1j * rng.standard_normal((nsrc, n)))
    t = np.arange(n)
    r = np.arange(nsrc)[:, None]
    z += 0.7 * np.exp(2j * np.pi * (((5 + 3 * r) % nfft + 0.3) / nfft) * t)
    z += 0.7e-4 * np.exp(-2j * np.pi * (((11 + 5 * r) % nfft + 0.45) / nfft) * t)
    return z.astype(np.complex64)


def slot_rows(nslots, nsrc=NSRC):
    """slots over the rows with repeats, every 13th off"""
    j = np.arange(nslots)
    rows = (7 * j + 3) % nsrc
    rows[j % 13 == 5] = -1
    return rows.astype(np.int64)


def segments_view(x, nfft, hop):
    n = nseg_of(x.shape[-1], nfft, hop)
    st = x.strides
    return np.lib.stride_tricks.as_strided(x, shape=x.shape[:-1] + (n, nfft), strides=st[:-1] + (hop * st[-1], st[-1]),
                                           writeable=False)


def scope_ref(z, nfft, hop, avg, window, first_segment=0, nsegments=None):
    """z complex [rows, n] -> float64 [rows, lines, nfft]: windowed segments, np.fft.fft in double, re^2 + im^2, summed
    over avg segments per line.  first_segment / nsegments: only those segments (a multiple of avg)."""
    z = np.ascontiguousarray(np.asarray(z, np.complex128))
    w = np.asarray(window, np.float64)
    segs = segments_view(z, nfft, hop)
    segs = segs[:, first_segment:segs.shape[1] if nsegments is None else first_segment + nsegments]
    L = segs.shape[1] // avg
    out = np.zeros((z.shape[0], L, nfft))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):     # non-finite samples are data: no warnings
        for l in range(L):
            X = np.fft.fft(segs[:, l * avg:(l + 1) * avg] * w, axis=-1)
            out[:, l] = (X.real ** 2 + X.imag ** 2).sum(axis=1)
    return out


def scope_model_f32(z, nfft, hop, avg, window):
    """The INDEPENDENT float32 model: scipy.fft on complex64, float32 powers, float32 sequential line sums."""
    import scipy.fft
    z = np.ascontiguousarray(np.asarray(z, np.complex64))
    w = np.asarray(window, F32)
    segs = segments_view(z, nfft, hop)
    L = segs.shape[1] // avg
    out = np.zeros((z.shape[0], L, nfft), F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):     # non-finite samples are data: no warnings
        for l in range(L):
            for i in range(avg):
                X = scipy.fft.fft(segs[:, l * avg + i] * w, axis=-1)
                assert X.dtype == np.complex64
                p = (X.real * X.real + X.imag * X.imag).astype(F32)
                out[:, l] = p if i == 0 else out[:, l] + p
    return out


def slot_lines(row_lines, rows):
    """lines per source row -> lines per slot; an off slot's are zeros"""
    rows = np.asarray(rows)
    out = row_lines[np.maximum(rows, 0)].copy()
    out[rows < 0] = 0
    return out


def err(lines, ref):
    """max_k |line - ref| / max_k ref per line, the worst line; lines whose reference is all zero are left out (the
    tests ask those for exact zeros)"""
    lines, ref = np.asarray(lines, np.float64), np.asarray(ref, np.float64)
    top = ref.max(axis=-1)
    d = np.abs(lines - ref).max(axis=-1)
    ok = top > 0
    return float((d[ok] / top[ok]).max()) if ok.any() else 0.0


def db(lines, avg, window):
    w = np.asarray(window, np.float64)
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(np.asarray(lines, np.float64) / (avg * w.sum() ** 2))


class ScopeRef:
    """The streaming definition: process() batch by batch, set_slot between them.  Per slot it keeps the series the
    definition speaks of -- the watched row's values, zeros before a retarget -- and makes the lines that complete."""

    def __init__(self, nsrc, rows, nfft, hop, avg, window):
        self.nsrc, self.rows = nsrc, [int(r) for r in rows]
        self.nfft, self.hop, self.avg, self.window = nfft, hop, avg, np.asarray(window, np.float64)
        if any(r < -1 or r >= nsrc for r in self.rows):
            raise ValueError("row")
        self.series = np.zeros((len(self.rows), 0), np.complex128)

    def set_slot(self, j, row):
        if not (0 <= j < len(self.rows)) or not (-1 <= row < self.nsrc):
            raise ValueError("slot or row")
        if self.rows[j] != row:
            self.rows[j] = row
            self.series[j] = 0

    def process(self, z):
        z = np.asarray(z, np.complex128)
        before = self.series.shape[1]
        new = np.zeros((len(self.rows), z.shape[1]), np.complex128)
        for j, r in enumerate(self.rows):
            if r >= 0:
                new[j] = z[r]
        self.series = np.concatenate([self.series, new], axis=1)
        l0 = nlines_of(before, self.nfft, self.hop, self.avg)
        l1 = nlines_of(self.series.shape[1], self.nfft, self.hop, self.avg)
        return scope_ref(self.series, self.nfft, self.hop, self.avg, self.window, l0 * self.avg, (l1 - l0) * self.avg)


def run_cuts(obj, z, cuts):
    """obj.process over z cut into batches -> the lines, concatenated along the line axis"""
    out, at = [], 0
    for c in cuts:
        out.append(np.asarray(obj.process(z[:, at:at + c])))
        at += c
    assert at == z.shape[1]
    return np.concatenate(out, axis=1)


def gpu_cuts(nfft, hop, avg, n):
    """The cut list of the bit-exact tests: 0, 1, hop - 1, hop, hop + 1, nfft - 1, nfft and avg hop, then 7, 0 and the
    rest; its preconditions are asserted by tests/test_scope_cpu.py"""
    cuts = [0, 1, hop - 1, hop, hop + 1, nfft - 1, nfft, avg * hop, 7, 0]
    cuts.append(n - sum(cuts))
    return cuts


RAGGED_SEED = {2048: 17, 4096: 17}


def ragged_seed(nfft):
    """the seed of the bit-exact tests' ragged list: 11, or where the series is too few transforms long for that one to
    have more than 12 batches, the first seed that gives as many (with a 0 and a 1 among them)"""
    return RAGGED_SEED.get(nfft, 11)


def ragged_cuts(n, nfft, seed):
    """seeded batch sizes from 0 to 3 nfft / 2 samples, small ones favoured, that add up to n"""
    rng = np.random.default_rng(seed)
    cuts, left = [], n
    while left:
        b = int(rng.integers(0, 3 * nfft // 2 + 1))
        if rng.random() < 0.3:
            b = int(rng.integers(0, 4))
        b = min(b, left)
        cuts.append(b)
        left -= b
    return cuts


def tone_series(nfft, n, tones, nsrc=1):
    """sum of A exp(2 pi i k t / nfft) over (A, k) in tones, no noise, complex64 [nsrc, n] (every row the same)"""
    t = np.arange(n)
    x = np.zeros(n, complex)
    for a, k in tones:
        x += a * np.exp(2j * np.pi * ((k * t) % nfft) / nfft)
    return np.repeat(x.astype(np.complex64)[None], nsrc, axis=0)


WEAK_CASES = 8
WEAK_LINES = 3


def weak_tones(nfft, seed=5):
    """WEAK_CASES pairs (strong bin, weak bin), at least 8 bins apart, the first pair fixed"""
    rng = np.random.default_rng(seed + nfft)
    pairs = [(nfft // 8 + 3, nfft // 2 + 9)]
    while len(pairs) < WEAK_CASES:
        ks = int(rng.integers(0, nfft))
        pairs.append((ks, (ks + int(rng.integers(8, nfft - 8))) % nfft))
    return pairs


def weak_series(nfft, hop, avg):
    """row r: two bin-centred tones, amplitude 0.7 on weak_tones' strong bin and 0.7e-4 on its weak bin, no noise;
    WEAK_LINES lines' worth.  -> complex64 [WEAK_CASES, n]"""
    n = (WEAK_LINES * avg - 1) * hop + nfft
    return np.concatenate([tone_series(nfft, n, [(0.7, ks), (0.7e-4, k)]) for ks, k in weak_tones(nfft)], axis=0)


def set_slot_plan(nfft, hop, avg):
    """The set_slot test: [(samples fed so far, [(slot, row), ...])], every point in the middle of a line with samples
    carried.  Slot 2 is retargeted and later brought back, slot 3 is switched off and on again, slot 5 (off in
    slot_rows) is switched on, slot 4 is given the row it has."""
    rows = slot_rows(8)
    assert rows[5] == -1 and min(rows[2], rows[3], rows[4]) >= 0
    at1 = nfft + avg * hop + hop // 2
    at2 = at1 + avg * hop + 3
    at3 = at2 + (3 if (nfft, hop, avg) == (512, 384, 3) else 2) * hop + 1          # (there two hops on would end a line)
    return [(at1, [(2, int(rows[2]) + 1), (3, -1), (4, int(rows[4]))]),
            (at2, [(3, int(rows[3])), (5, 9)]),
            (at3, [(2, int(rows[2]))])]


TOUCHED = (2, 3, 5)


def run_plan(obj, z, plan, cuts_between):
    """z through obj.process with the plan's set_slot calls at their sample counts; cuts_between(a, b) -> the batch
    sizes from sample a to sample b.  -> the lines, concatenated"""
    out, at = [], 0
    for stop, calls in list(plan) + [(z.shape[1], [])]:
        for c in cuts_between(at, stop):
            out.append(np.asarray(obj.process(z[:, at:at + c])))
            at += c
        assert at == stop
        for j, row in calls:
            obj.set_slot(j, row)
    return np.concatenate(out, axis=1)
