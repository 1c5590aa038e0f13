"""The scope without a GPU: the host arithmetic and the argument checks of the C ABI, the reference's own properties
(tests/scope_ref.py), the float32 model the GPU tolerances rest on, and the preconditions the GPU tests' inputs have to
meet."""
import ctypes as C

import numpy as np
import pytest

import scope_ref as SR

ALL_SIZES = [s[:3] for s in SR.SIZES] + [s for s in SR.CUT_SIZES if s not in [t[:3] for t in SR.SIZES]]


def cut_lists(nfft, hop, avg):
    """the batch cuts the GPU tests use at this size: one batch everywhere; at CUT_SIZES also the list, the list reversed
    and a seeded ragged one"""
    n = SR.gpu_len(nfft, hop, avg)
    if (nfft, hop, avg) not in SR.CUT_SIZES:
        return n, [[n]]
    cuts = SR.gpu_cuts(nfft, hop, avg, n)
    return n, [[n], cuts, cuts[::-1], SR.ragged_cuts(n, nfft, SR.ragged_seed(nfft))]


def test_reference_against_closed_forms():
    """A tone of amplitude a on a bin centre under the periodic Hann window: (a N / 2)^2 in its bin, (a N / 4)^2 in the
    two neighbours, nothing elsewhere, times avg; and Parseval: sum_k p[k] = N sum_n |x[n] w[n]|^2 per segment."""
    nfft, hop, avg, a, k0 = 256, 64, 3, 0.25, 37
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(nfft) / nfft)     # in double: the closed form is the unrounded window's
    n = (2 * avg - 1) * hop + nfft
    t = np.arange(n)
    x = (a * np.exp(2j * np.pi * k0 * t / nfft))[None]
    lines = SR.scope_ref(x, nfft, hop, avg, w)
    assert lines.shape == (1, 2, nfft)
    want = np.zeros(nfft)
    want[k0], want[k0 - 1], want[k0 + 1] = (a * nfft / 2) ** 2, (a * nfft / 4) ** 2, (a * nfft / 4) ** 2
    assert np.max(np.abs(lines - avg * want)) <= 1e-9 * avg * want.max()
    assert np.max(np.abs(SR.db(lines, avg, w)[0, :, k0] - 20 * np.log10(a))) < 1e-9
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))
    lines = SR.scope_ref(x, nfft, hop, avg, w)
    for l in range(2):
        e = sum((np.abs(x[:, s * hop:s * hop + nfft] * w) ** 2).sum(axis=1) for s in range(l * avg, (l + 1) * avg))
        assert np.allclose(lines[:, l].sum(axis=1), nfft * e, rtol=1e-12)


@pytest.mark.parametrize("size", ALL_SIZES)
def test_scope_lines_against_brute_force(pkg, size):
    """pddc_scope_lines for every (hop, avg, cut) of the GPU tests: line l is complete once sample
    (l avg + avg - 1) hop + nfft - 1 is in the stream"""
    nfft, hop, avg = size
    n, lists = cut_lists(nfft, hop, avg)

    def brute(length):
        l = 0
        while (l * avg + avg - 1) * hop + nfft <= length:
            l += 1
        return l

    for cuts in lists:
        at = 0
        for c in cuts:
            assert pkg.scope_lines(nfft, hop, avg, at, c) == brute(at + c) - brute(at), (cuts, at, c)
            at += c
        assert at == n
    assert brute(n) == 6 == SR.nlines_of(n, nfft, hop, avg)
    for bad in ((128, 64, 1), (8192, 4096, 1), (300, 150, 1), (256, 15, 1), (256, 257, 1), (256, 128, 0), (256, 128, 4097)):
        assert pkg.scope_lines(*bad, 0, 1 << 20) == 0, bad
    assert pkg.scope_lines(4096, 256, 4096, 0, 1 << 24) == ((((1 << 24) - 4096) // 256 + 1) // 4096)
    assert pkg.scope_block_items(128) == 0 and all(pkg.scope_block_items(n) >= 1 for n in (256, 512, 1024, 2048, 4096))
    assert pkg.PDDC_SCOPE_CENTERED == 0x1


@pytest.mark.parametrize("size", SR.CUT_SIZES)
def test_reference_streaming_equals_one_shot(size):
    nfft, hop, avg = size
    n, lists = cut_lists(nfft, hop, avg)
    z = SR.gpu_series(nfft, hop, avg, nsrc=5)
    w = SR.hann(nfft)
    rows = [0, 4, -1, 4, 2, 1, 3]
    want = SR.slot_lines(SR.scope_ref(z, nfft, hop, avg, w), rows)
    assert want.shape == (7, 6, nfft) and not want[2].any() and np.array_equal(want[1], want[3])
    for cuts in lists:
        got = SR.run_cuts(SR.ScopeRef(5, rows, nfft, hop, avg, w), z, cuts)
        assert np.array_equal(got, want), cuts


def test_reference_set_slot_counts_the_new_row_as_zeros_before_the_change():
    nfft, hop, avg = 256, 128, 4
    z = SR.gpu_series(nfft, hop, avg, nsrc=5)
    n, w, cut = z.shape[1], SR.hann(nfft), 1000
    r = SR.ScopeRef(5, [0, 1, -1], nfft, hop, avg, w)
    a = r.process(z[:, :cut])
    r.set_slot(0, 3)
    r.set_slot(1, 1)                                   # the row it has: nothing changes
    r.set_slot(2, 4)                                   # off -> on
    for bad in ((3, 0), (-1, 0), (0, 5), (0, -2)):
        with pytest.raises(ValueError):
            r.set_slot(*bad)
    got = np.concatenate([a, r.process(z[:, cut:])], axis=1)
    zz = z.copy()
    zz[:, :cut] = 0
    plain, zeroed = SR.scope_ref(z, nfft, hop, avg, w), SR.scope_ref(zz, nfft, hop, avg, w)
    la = a.shape[1]
    assert 0 < la < got.shape[1] == 6
    assert np.array_equal(got[0, :la], plain[0, :la]) and np.array_equal(got[0, la:], zeroed[3, la:])
    assert np.array_equal(got[1], plain[1])
    assert not got[2, :la].any() and np.array_equal(got[2, la:], zeroed[4, la:])
    assert not np.array_equal(zeroed[3, la], plain[3, la])         # the change fell into line la


@pytest.mark.parametrize("size", SR.CUT_SIZES)
def test_gpu_inputs_preconditions(size):
    """What tests/test_gpu_scope.py relies on: every cut list adds up to the series and contains 0, 1, hop - 1, hop,
    hop + 1, nfft - 1, nfft and avg hop; the series ends inside a line (a partial sum is left behind) and inside a
    segment; every set_slot point lies in the middle of a line, with samples carried, and the points are in order; the
    slot map has repeats, off slots and every row."""
    nfft, hop, avg = size
    n, lists = cut_lists(nfft, hop, avg)
    for cuts in lists[1:3]:
        assert sum(cuts) == n and min(cuts) >= 0
        assert {0, 1, hop - 1, hop, hop + 1, nfft - 1, nfft, avg * hop} <= set(cuts)
    assert sum(lists[3]) == n and 0 in lists[3] and 1 in lists[3] and len(lists[3]) > 12
    nseg = SR.nseg_of(n, nfft, hop)
    assert nseg % avg != 0 and n > (nseg - 1) * hop + nfft
    last = 0
    for at, calls in SR.set_slot_plan(nfft, hop, avg):
        s = SR.nseg_of(at, nfft, hop)
        assert last < at < n and s % avg != 0 and at - s * hop > 0
        last = at
    rows = SR.slot_rows(1024)
    assert set(rows.tolist()) == set(range(-1, SR.NSRC)) and (rows < 0).sum() > 50
    assert not np.isnan(SR.gpu_series(nfft, hop, avg, nsrc=2)).any()


def test_float32_model_against_double():
    """The independent float32 model on the very inputs of the GPU tests, re-measured: MODEL_WORST quotes its worst,
    TOL_SCOPE is TOL_FACTOR times that and stays below the panorama's 1e-5."""
    worst = 0.0
    for nfft, hop, avg in ALL_SIZES:
        z, w = SR.gpu_series(nfft, hop, avg), SR.hann(nfft)
        e = SR.err(SR.scope_model_f32(z, nfft, hop, avg, w), SR.scope_ref(z, nfft, hop, avg, w))
        print(f"float32 model {nfft} / {hop} / {avg}: {e:.2e}")
        worst = max(worst, e)
    assert SR.MODEL_WORST / 2 < worst <= SR.MODEL_WORST
    assert SR.TOL_SCOPE == SR.TOL_FACTOR * SR.MODEL_WORST <= 1e-5 and SR.TOL_FACTOR == 8


@pytest.mark.parametrize("size", SR.CUT_SIZES)
def test_weak_tone_model(size):
    """The weak-tone bound: the model's error on the weak bin, relative to the bin's own reference value, over the tone
    placements the GPU test uses; the reference itself puts the weak bin 80 dB below the strong one."""
    nfft, hop, avg = size
    z, w = SR.weak_series(nfft, hop, avg), SR.hann(nfft)
    ref, mod = SR.scope_ref(z, nfft, hop, avg, w), SR.scope_model_f32(z, nfft, hop, avg, w)
    assert ref.shape == (SR.WEAK_CASES, SR.WEAK_LINES, nfft)
    worst, d = 0.0, SR.db(ref, avg, w)
    for r, (ks, k) in enumerate(SR.weak_tones(nfft)):
        assert min((ks - k) % nfft, (k - ks) % nfft) >= 8
        worst = max(worst, float((np.abs(mod[r, :, k] - ref[r, :, k]) / ref[r, :, k]).max()))
        assert np.max(np.abs(d[r, :, ks] - d[r, :, k] - 80.0)) < 0.002
        assert np.max(np.abs(d[r, :, ks] - 20 * np.log10(0.7))) < 1e-4
    print(f"float32 model, weak bin, nfft {nfft}: {worst:.2e}")
    assert SR.WEAK_MODEL_WORST[nfft] / 2 < worst <= SR.WEAK_MODEL_WORST[nfft]
    assert 10 * np.log10(1 + SR.TOL_WEAK[nfft]) + 0.002 < SR.DB_MARGIN


def test_argument_errors_without_a_device(pkg):
    L = pkg.ddc_lib()
    hann = SR.hann

    def create(nsrc=8, rows=(0, 7, -1, 3), nslots=None, nfft=256, hop=128, avg=4, window=None, flags=0, null_rows=False,
               null_window=False):
        r = (C.c_int * max(len(rows), 1))(*rows)
        w = np.ascontiguousarray(hann(nfft if nfft in (256, 512, 1024, 2048, 4096) else 256) if window is None else window,
                                 dtype=np.float32)
        h = C.c_void_p()
        rc = L.pddc_scope_create(C.byref(h), 0, nsrc, len(rows) if nslots is None else nslots, None if null_rows else r, nfft,
                                 hop, avg, None if null_window else w.ctypes.data_as(C.POINTER(C.c_float)), flags)
        if rc == 0:
            L.pddc_scope_destroy(h)
        return rc

    nanw, infw = hann(256).copy(), hann(256).copy()
    nanw[200], infw[0] = np.nan, -np.inf
    bad = [dict(nsrc=0), dict(nsrc=1025), dict(nsrc=-3), dict(nslots=0), dict(rows=[0] * 1025), dict(null_rows=True),
           dict(null_window=True), dict(nfft=128, hop=64), dict(nfft=8192, hop=4096), dict(nfft=300, hop=150), dict(nfft=0, hop=0),
           dict(hop=15), dict(hop=257), dict(hop=0), dict(hop=-128), dict(nfft=4096, hop=255), dict(avg=0), dict(avg=-1),
           dict(avg=4097), dict(flags=2), dict(flags=0x80000001), dict(rows=(0, 8)), dict(rows=(-2, 0)), dict(window=nanw),
           dict(window=infw)]
    for kw in bad:
        assert create(**kw) == pkg.PDDC_EINVAL, kw
    w = hann(256)
    r = (C.c_int * 1)(0)
    assert L.pddc_scope_create(None, 0, 1, 1, r, 256, 128, 1, w.ctypes.data_as(C.POINTER(C.c_float)), 0) == pkg.PDDC_EINVAL
    import torch
    if not torch.cuda.is_available():
        # every limit from the inside
        assert create() == pkg.PDDC_ENODEV
        assert create(nsrc=1024, rows=[1023] * 1024, nfft=4096, hop=4096, avg=4096, flags=1) == pkg.PDDC_ENODEV
        assert create(nsrc=1, rows=[-1], nfft=256, hop=16, avg=1) == pkg.PDDC_ENODEV
        with pytest.raises(pkg.PddcError) as e:
            pkg.Scope(4, [0, 1], 256)
        assert e.value.code == pkg.PDDC_ENODEV
    for kw in (dict(nfft=128), dict(nfft=256, hop=8), dict(nfft=256, avg=0), dict(nfft=256, avg=1 << 40),
               dict(nfft=256, window=nanw), dict(nfft=256, window=hann(512))):
        with pytest.raises(pkg.PddcError) as e:
            pkg.Scope(4, [0, 1], **kw)
        assert e.value.code == pkg.PDDC_EINVAL, kw
    for rows in ([0, 4], [-2], [1 << 40], []):
        with pytest.raises(pkg.PddcError) as e:
            pkg.Scope(4, rows, 256)
        assert e.value.code == pkg.PDDC_EINVAL, rows
    n = C.c_size_t(5)
    assert L.pddc_scope_process(None, None, 8, 8, None, 8, C.byref(n), None) == pkg.PDDC_EINVAL and n.value == 5
    assert L.pddc_scope_set_slot(None, 0, 0) == pkg.PDDC_EINVAL
    assert L.pddc_scope_reset(None) == pkg.PDDC_EINVAL
    assert L.pddc_scope_next_lines(None, 1 << 20) == 0
    assert L.pddc_scope_destroy(None) == 0
