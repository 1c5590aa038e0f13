"""What the non-finite tests (tests/test_nonfinite_cpu.py, tests/test_gpu_nonfinite.py) share: the poison values, where
they are planted, and the two comparisons.  A plain module: no fixtures, nothing of the code under test."""
import numpy as np

F32 = np.float32
QNAN_BITS = 0x7FC00000
NEVER_BITS = (0xFFFFFFFF, QNAN_BITS)             # cells nothing may read: both words are NaNs, the first a negative one


def f32_of(word):
    return np.array([word], np.uint32).view(F32)[0]


QNAN = f32_of(QNAN_BITS)
# in data: the quiet NaN and the two infinities.  Signalling NaNs are left out on purpose: neither C nor the header
# pins fminf of one.
POISON = {"nan": QNAN, "+inf": F32(np.inf), "-inf": F32(-np.inf)}
# for the bit-exact stages two more: a finite value whose square overflows, and one whose square is zero in float32
POISON_EXACT = dict(POISON, huge=F32(1e25), tiny=F32(2.0 ** -80))


FLOATS = {np.dtype(np.float32): (F32, np.uint32), np.dtype(np.complex64): (F32, np.uint32), np.dtype(np.float64): (np.float64, np.uint64)}


def parts(x):
    """a float32 / complex64 / float64 array as its real numbers (complex: re, im interleaved along the last axis)"""
    x = np.ascontiguousarray(x)
    return x.view(FLOATS[x.dtype][0])


def words(x):
    """the uint32 words of a float32 / complex64 array (complex: re, im interleaved along the last axis), the uint64
    words of a float64 one (the equaliser's states); integer arrays as they are"""
    x = np.ascontiguousarray(x)
    return x.view(FLOATS[x.dtype][1]) if x.dtype in FLOATS else x


def never_read(shape, dtype):
    """an array of `shape` whose every 32-bit word is 0xFFFFFFFF or 0x7FC00000, alternating (int16 / uint8 arrays get the
    bytes of that pattern): the fill of padding, spare rows and output buffers"""
    dtype = np.dtype(dtype)
    nbytes = int(np.prod(shape)) * dtype.itemsize
    w = np.empty((nbytes + 3) // 4, np.uint32)
    w[0::2], w[1::2] = NEVER_BITS
    return w.view(np.uint8)[:nbytes].view(dtype).reshape(shape).copy()


def plant(x, rows, cols, value, part="both"):
    """a copy of x (float32 or complex64 [K, n]) with `value` at x[r, c] for every r in rows and c in cols; complex:
    in the real part, the imaginary part or both"""
    y = np.array(x, copy=True)
    rows, cols = np.atleast_1d(rows), np.atleast_1d(cols)
    assert y.ndim == 2 and rows.size and cols.size and 0 <= rows.min() and rows.max() < y.shape[0]
    assert 0 <= cols.min() and cols.max() < y.shape[1]
    for r in rows:
        if y.dtype == np.complex64:
            v = y[r].view(F32).reshape(-1, 2)
            if part in ("re", "both"):
                v[cols, 0] = value
            if part in ("im", "both"):
                v[cols, 1] = value
        else:
            assert y.dtype == F32
            y[r, cols] = value
    return y


def placements(TT, H, n, far=None):
    """the standard columns for a stage whose kernel walks tiles of TT and whose window / history is H long: 0, H - 1,
    TT - 1, TT, 2 TT + 3 and n - 1, in ascending order without repeats.  With cuts_for() the column TT - 1 is the last
    sample of a batch, TT the only sample of a batch of 1 and n - 1 the last sample the object sees.  far: the column
    to take for 2 TT + 3, where a stage's tiles count outputs and not inputs (TT is then the input of the second tile's
    first output, far that of output 2 TT + 3)."""
    far = 2 * TT + 3 if far is None else far
    assert TT < far < n - 1
    return sorted({0, max(H - 1, 0), TT - 1, TT, far, n - 1} & set(range(n)))


def cuts_for(TT, n, far=None):
    """the batch sizes that go with placements(): 1 | TT - 1 | 1 | far - TT | 0 | the rest (far = 2 TT + 3 unless
    given) -- column 0 and column TT are batches of 1, TT - 1, far and n - 1 each the last sample of a batch"""
    far = 2 * TT + 3 if far is None else far
    cuts = [1, TT - 1, 1, far - TT, 0, n - far - 1]
    assert min(cuts[1], cuts[3], cuts[5]) > 0 and sum(cuts) == n
    return cuts


def poisoned_rows(K, G=16):
    """rows 0 and K - 1 and the first and last row of the full group of G in the middle; with K = 2 G + 3 every clean
    row shares a block of 2, 4 or 16 receivers with a poisoned one, in this order or the reversed one"""
    assert K >= 2 * G + 1
    return [0, G, 2 * G - 1, K - 1]


def same_or_both_nan(got, want, what=""):
    """NaN exactly where `want` has NaN; every other value equal by its words, infinities and signed zeros included.  For
    poisoned rows only: the host's and the device's NaNs may differ in sign and payload.  `want` must hold values that
    are no NaN, or the comparison would say nothing."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype not in FLOATS:
        assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4].tolist())
        return
    g, w = parts(got), parts(want)
    gn, wn = np.isnan(g), np.isnan(w)
    assert not wn.all(), (what, "nothing but NaN to compare with")
    assert np.array_equal(gn, wn), (what, "NaN positions", np.argwhere(gn != wn)[:4].tolist())
    gw, ww = words(g), words(w)
    bad = (gw != ww) & ~wn
    assert not bad.any(), (what, "bits", np.argwhere(bad)[:4].tolist())


def clean_rows_identical(got, clean, rows, what=""):
    """plain equality of the words on `rows` -- after asserting that clean[rows] holds nothing that is not finite, so
    that no NaN-tolerant comparison is needed, or used, there"""
    got, clean = np.ascontiguousarray(got), np.ascontiguousarray(clean)
    assert got.shape == clean.shape and got.dtype == clean.dtype, (what, got.shape, clean.shape)
    rows = np.asarray(rows)
    c = clean[rows]
    if c.dtype in FLOATS:
        assert np.isfinite(parts(c)).all(), (what, "the clean run is not finite on these rows")
    gw, cw = words(got[rows]), words(c)
    assert np.array_equal(gw, cw), (what, np.argwhere(gw != cw)[:4].tolist())


# ---- ragged outputs: records of which the first counts[j] of row j are written ---------------------------------------

def gather(buf, counts):
    """a record buffer [K, capacity, ...] and its counts [K] -> one array per row, the records that were written"""
    counts = np.asarray(counts)
    assert counts.shape == (buf.shape[0],) and (counts >= 0).all() and (counts <= buf.shape[1]).all(), (counts.tolist(), buf.shape)
    return [buf[j, :counts[j]].copy() for j in range(buf.shape[0])]


def dense(rows, width):
    """per-row record lists (each [count_j, ...], one dtype and record shape) as one array [K, width, ...], zeros behind
    a row's records: rows that hold the same records give the same array, so the comparisons above apply.  With the
    rows' counts beside it nothing is lost: a record of zeros is told from no record"""
    out = np.zeros((len(rows), width) + tuple(rows[0].shape[1:]), rows[0].dtype)
    for j, r in enumerate(rows):
        assert r.shape[0] <= width and r.shape[1:] == out.shape[2:] and r.dtype == out.dtype, (j, r.shape, out.shape)
        out[j, :r.shape[0]] = r
    return out


def record_words(chars):
    """per-row arrays of 16-byte records (a reference's CHAR arrays) as int32 [count_j, 4], the device's layout"""
    return [np.ascontiguousarray(c).view(np.int32).reshape(-1, 4) for c in chars]
