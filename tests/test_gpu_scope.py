"""The scope on the device (pddc_scope_*, k_scope) against tests/scope_ref.py: within TOL_SCOPE of the double reference
(where the tolerance comes from: scope_ref.py), and bit for bit against itself under every change that must not matter."""
import ctypes as C
import types

import numpy as np
import pytest

import scope_ref as SR
import tuner_ref as TR

pytestmark = pytest.mark.gpu


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


_cache = {}


def inputs(size, dev):
    """(z on the host, z on the device, window, the double reference per source row), made once per size"""
    import torch
    if size not in _cache:
        nfft, hop, avg = size
        z, w = SR.gpu_series(nfft, hop, avg), SR.hann(nfft)
        _cache[size] = (z, torch.from_numpy(z).to(dev), w, SR.scope_ref(z, nfft, hop, avg, w))
    return _cache[size]


def run(pkg, zd, rows, size, cuts=None, **kw):
    """a new Scope over zd cut into batches -> the lines on the host, float32 [nslots, lines, nfft]"""
    nfft, hop, avg = size
    s = pkg.Scope(zd.shape[0], rows, nfft, hop, avg, **kw)
    got, at = [], 0
    for c in cuts or [zd.shape[1]]:
        assert s.next_lines(c) == pkg.scope_lines(nfft, hop, avg, at, c)
        got.append(s.process(zd[:, at:at + c]).cpu().numpy())
        assert got[-1].shape == (len(rows), pkg.scope_lines(nfft, hop, avg, at, c), nfft)
        at += c
    assert at == zd.shape[1]
    s.close()
    return np.concatenate(got, axis=1)


@pytest.mark.parametrize("size", SR.SIZES, ids=lambda s: "-".join(map(str, s)))
def test_against_the_reference(pkg, dev, size):
    """64 source rows, the slots mapped over them with repeats and off slots, one batch of 6 lines and a partial one:
    the line count is scope_lines', every line is within TOL_SCOPE of the double reference, an off slot's lines are
    zeros, and centered=True gives the same bits rotated by nfft/2."""
    nfft, hop, avg, nslots = size
    z, zd, w, ref_rows = inputs(size[:3], dev)
    rows = SR.slot_rows(nslots)
    got = run(pkg, zd, rows, size[:3])
    want = SR.slot_lines(ref_rows, rows)
    assert got.shape == want.shape == (nslots, 6, nfft)
    e = SR.err(got, want)
    print(f"scope {nfft} / {hop} / {avg}, {nslots} slots: err {e:.2e} (TOL_SCOPE {SR.TOL_SCOPE:.1e})")
    assert (rows < 0).any() and not got[rows < 0].any()
    assert e <= SR.TOL_SCOPE
    cen = run(pkg, zd, rows, size[:3], centered=True)
    assert np.array_equal(bits(cen), bits(np.roll(got, nfft // 2, axis=-1)))


@pytest.mark.parametrize("size", SR.CUT_SIZES, ids=lambda s: "-".join(map(str, s)))
def test_cut_and_company(pkg, dev, size):
    """Bit for bit: one batch against the cut list (0, 1, hop - 1, hop, hop + 1, nfft - 1, nfft, avg hop, ...), the list
    reversed and a seeded ragged list; 1024 slots (256 at 2048 and 4096, the plans of 2 and 4 waves per transform)
    against 7, 5 and 1 (counts on either side of the kernel's items per block); the slot order reversed; a slot alone
    against itself among them all; two slots on one row."""
    nfft, hop, avg = size
    z, zd, w, _ = inputs(size, dev)
    n = z.shape[1]
    rows = SR.slot_rows(256 if nfft >= 2048 else 1024)
    base = bits(run(pkg, zd, rows, size))
    cuts = SR.gpu_cuts(nfft, hop, avg, n)
    for name, c in (("cuts", cuts), ("reversed", cuts[::-1]), ("ragged", SR.ragged_cuts(n, nfft, SR.ragged_seed(nfft)))):
        assert np.array_equal(bits(run(pkg, zd, rows, size, c)), base), name
    g = pkg.scope_block_items(nfft)
    assert g == 1 or (7 % g and 5 % g)                 # blocks whose items belong to two line units
    for k in (7, 5, 1):
        assert np.array_equal(bits(run(pkg, zd, rows[:k], size)), base[:k]), k
    assert np.array_equal(bits(run(pkg, zd, rows[::-1], size, cuts)), base[::-1])
    assert rows[37] >= 0 and np.array_equal(bits(run(pkg, zd, rows[37:38], size, cuts[::-1])), base[37:38])
    assert rows[37] == rows[37 + 64] and np.array_equal(base[37], base[37 + 64]) and base[37].any()


@pytest.mark.parametrize("size", SR.CUT_SIZES, ids=lambda s: "-".join(map(str, s)))
def test_weak_tone(pkg, dev, size):
    """Two bin-centred tones of amplitude 0.7 and 0.7e-4, no noise, Hann window, WEAK_CASES placements: the weak bin is
    within TOL_WEAK of its own reference value, and in dB (scope_db) it stands 80 dB below the strong one within
    DB_MARGIN."""
    import torch
    nfft, hop, avg = size
    z, w = SR.weak_series(nfft, hop, avg), SR.hann(nfft)
    ref = SR.scope_ref(z, nfft, hop, avg, w)
    s = pkg.Scope(SR.WEAK_CASES, range(SR.WEAK_CASES), nfft, hop, avg, window=w)
    lines = s.process(torch.from_numpy(z).to(dev))
    got, d = lines.cpu().numpy(), pkg.scope_db(lines, avg, w)
    s.close()
    assert got.shape == ref.shape == (SR.WEAK_CASES, SR.WEAK_LINES, nfft)
    worst, worst_db = 0.0, 0.0
    for r, (ks, k) in enumerate(SR.weak_tones(nfft)):
        worst = max(worst, float((np.abs(got[r, :, k] - ref[r, :, k]) / ref[r, :, k]).max()))
        worst_db = max(worst_db, float(np.abs(d[r, :, ks] - d[r, :, k] - 80.0).max()))
        assert np.max(np.abs(d[r, :, ks] - 20 * np.log10(0.7))) < 0.001
    print(f"weak tone, nfft {nfft}: weak bin off by {worst:.2e} of itself (TOL_WEAK {SR.TOL_WEAK[nfft]:.1e}), "
          f"distance off 80 dB by {worst_db:.4f} dB")
    assert worst <= SR.TOL_WEAK[nfft]
    assert worst_db <= SR.DB_MARGIN


def test_repeatability(pkg, dev):
    """The plans of 2 and 4 waves per transform (2048, 4096) and one of a single wave (1024) as the control, 64 slots, the
    gpu_series input in gpu_cuts' batches: a fresh object, ten runs after reset() and another fresh object give the same
    bits in every line."""
    for size in ((2048, 512, 2), (4096, 1024, 2), (1024, 512, 2)):
        nfft, hop, avg = size
        z, zd, w, _ = inputs(size, dev)
        cuts = SR.gpu_cuts(nfft, hop, avg, z.shape[1])
        rows = SR.slot_rows(64)

        def once(s):
            return bits(SR.run_cuts(types.SimpleNamespace(process=lambda b: s.process(b).cpu().numpy()), zd, cuts))

        s = pkg.Scope(SR.NSRC, rows, nfft, hop, avg)
        first = once(s)
        assert first.shape == (64, 6, nfft) and first[rows >= 0].any()
        for i in range(10):
            s.reset()
            assert np.array_equal(once(s), first), (size, i)
        s.close()
        fresh = pkg.Scope(SR.NSRC, rows, nfft, hop, avg)
        assert np.array_equal(once(fresh), first), size
        fresh.close()


def test_strides_and_canaries(pkg, dev):
    """z is the view Tuner.process returns (stride = capacity > n), lines have line_stride above the lines due: the
    slack on both sides keeps its canary, and the values are within TOL_SCOPE of the reference on a host copy of the view."""
    import torch
    M, hop, T, K, S = 1024, 512, 64, 13, 1200
    nfft, shop, avg = 256, 128, 2
    gen = torch.Generator(device="cpu").manual_seed(5)
    rows = torch.view_as_complex(torch.randn((S, M, 2), generator=gen, dtype=torch.float32)).to(dev)
    g = types.SimpleNamespace(nchan=M, hop=hop, device=0, first=0, count=M)
    t = pkg.Tuner(g, TR.receiver_set(M, K), pkg.tuner_lowpass(T, 1), 1)
    cap = t.next_outputs(S) + 37
    zbuf = torch.full((K, cap), 3.0 - 4.0j, dtype=torch.complex64, device=dev)
    zv = t.process(rows, out=zbuf)
    n = zv.shape[1]
    assert zv.stride(0) == cap > n > 4 * nfft
    slots = [0, 12, -1, 5, 5, 7, 1]
    s = pkg.Scope(K, slots, nfft, shop, avg)
    due = s.next_lines(n)
    assert due == SR.nlines_of(n, nfft, shop, avg) >= 3
    canary = 7.25
    obuf = torch.full((len(slots), due + 3, nfft), canary, dtype=torch.float32, device=dev)
    out = s.process(zv, out=obuf)
    assert out.data_ptr() == obuf.data_ptr() and out.shape == (len(slots), due, nfft) and out.stride(0) == (due + 3) * nfft
    zh = zv.cpu().numpy()
    want = SR.slot_lines(SR.scope_ref(zh, nfft, shop, avg, SR.hann(nfft)), slots)
    e = SR.err(out.cpu().numpy(), want)
    print(f"strided: err {e:.2e}")
    assert e <= SR.TOL_SCOPE and not out[2].any()
    assert bool((obuf[:, due:] == canary).all()) and bool((zbuf[:, n:] == 3.0 - 4.0j).all())
    s.close()
    t.close()


class OnDevice:
    """a Scope as SR.run_plan drives the reference; with `bad`, refused set_slot calls in front of every good one"""

    def __init__(self, pkg, scope, bad=()):
        self.pkg, self.s, self.bad = pkg, scope, bad

    def process(self, z):
        return self.s.process(z).cpu().numpy()

    def set_slot(self, j, row):
        for b in self.bad:
            with pytest.raises(self.pkg.PddcError) as e:
                self.s.set_slot(*b)
            assert e.value.code == self.pkg.PDDC_EINVAL
        self.s.set_slot(j, row)


@pytest.mark.parametrize("size", SR.CUT_SIZES, ids=lambda s: "-".join(map(str, s)))
def test_set_slot_between_batches(pkg, dev, size):
    """Retarget, switch off and switch on again in mid-line (SR.set_slot_plan): the touched slots are within TOL_SCOPE of
    the streaming reference, with exact zeros where it has zeros; every slot is bit-equal to a second device run with
    the same calls at the same sample counts under a different cut; untouched slots are bit-equal to a run without the
    calls; bad calls are refused and change nothing."""
    nfft, hop, avg = size
    z, zd, w, _ = inputs(size, dev)
    n, nslots = z.shape[1], 64
    rows, plan = SR.slot_rows(nslots), SR.set_slot_plan(nfft, hop, avg)
    want = SR.run_plan(SR.ScopeRef(SR.NSRC, rows[:8], nfft, hop, avg, w), z, plan, lambda a, b: [b - a])
    bad = ((nslots, 0), (-1, 0), (0, SR.NSRC), (0, -2))
    a = SR.run_plan(OnDevice(pkg, pkg.Scope(SR.NSRC, rows, nfft, hop, avg), bad), zd, plan, lambda a, b: [b - a])
    rng = np.random.default_rng(4)

    def fine(a, b):
        c = [0, 1] + [int(v) for v in rng.integers(0, hop // 2 + 1, 3)]
        return c + [b - a - sum(c)]

    b = SR.run_plan(OnDevice(pkg, pkg.Scope(SR.NSRC, rows, nfft, hop, avg)), zd, plan, fine)
    plain = run(pkg, zd, rows, size)
    assert a.shape == b.shape == plain.shape == (nslots, 6, nfft)
    assert np.array_equal(bits(a), bits(b))
    untouched = [j for j in range(nslots) if j not in SR.TOUCHED]
    assert np.array_equal(bits(a[untouched]), bits(plain[untouched]))
    for j in SR.TOUCHED:
        e = SR.err(a[j], want[j])
        print(f"set_slot {nfft} / {hop} / {avg}: slot {j} err {e:.2e}")
        assert e <= SR.TOL_SCOPE
        zero = ~want[j].any(axis=-1)
        assert not a[j][zero].any()
        assert not np.array_equal(bits(a[j]), bits(plain[j]))
    assert (~want[3].any(axis=-1)).any() and (~want[5].any(axis=-1)).any()


def refused_calls_change_nothing(pkg, dev, size):
    """Refused calls -- a stride below n, a line stride below the lines due, misaligned z and lines, NULL z, NULL lines
    with lines due, lines overlapping z -- between good batches: the result equals that of an object that never saw them.
    NULL lines when none are due is accepted.  n = 0 and n < nfft on a fresh object work; reset starts the series again."""
    import torch
    nfft, hop, avg = size
    z, zd, w, _ = inputs(size, dev)
    n, L = z.shape[1], pkg.ddc_lib()
    rows = SR.slot_rows(16)
    base = bits(run(pkg, zd, rows, size))
    cuts = [0, nfft - 1, avg * hop + 5, 1]
    cuts.append(n - sum(cuts))
    s = pkg.Scope(SR.NSRC, rows, nfft, hop, avg)
    st = torch.cuda.current_stream(0).cuda_stream
    big = torch.zeros((16, 8, nfft), dtype=torch.float32, device=dev)
    got, at = [], 0
    for c in cuts:
        m = 2 * avg * hop + nfft                       # a batch that has lines due wherever it starts
        due = s.next_lines(m)
        assert due >= 1 and at + m <= n
        zp, cnt = zd[:, at:].data_ptr(), C.c_size_t(77)
        refused = [((zp, m, m - 1, big.data_ptr(), 8), pkg.PDDC_ECAPACITY),
                   ((zp, m, n, big.data_ptr(), due - 1), pkg.PDDC_ECAPACITY),
                   ((zp + 4, m, n, big.data_ptr(), 8), pkg.PDDC_EINVAL),
                   ((zp, m, n, big.data_ptr() + 4, 8), pkg.PDDC_EINVAL),
                   ((zp, m, n, big.data_ptr() + 8, 8), pkg.PDDC_EINVAL),
                   ((None, m, n, big.data_ptr(), 8), pkg.PDDC_EINVAL),
                   ((zp, m, n, None, 8), pkg.PDDC_EINVAL),
                   ((zp, m, n, zd.data_ptr(), 8), pkg.PDDC_EINVAL)]
        for (p, mm, zs, lp, ls), code in refused:
            assert L.pddc_scope_process(s._h, p, mm, zs, lp, ls, C.byref(cnt), st) == code, (p, mm, zs, lp, ls)
            assert cnt.value == 77 and s.next_lines(m) == due
        if s.next_lines(c) == 0:
            assert L.pddc_scope_process(s._h, zd[:, at:].data_ptr() if c else None, c, n, None, 0, C.byref(cnt), st) == 0
            assert cnt.value == 0
            got.append(np.zeros((16, 0, nfft), np.float32))
        else:
            got.append(s.process(zd[:, at:at + c]).cpu().numpy())
        at += c
    assert np.array_equal(bits(np.concatenate(got, axis=1)), base)
    assert not big.any()
    # reset, then a fresh object's first steps: n = 0, n < nfft, the rest
    s.reset()
    assert s.next_lines(n) == 6
    again = [s.process(zd[:, a:b]).cpu().numpy() for a, b in ((0, 0), (0, nfft - 1), (nfft - 1, n))]
    assert again[0].shape == again[1].shape == (16, 0, nfft)
    assert np.array_equal(bits(again[2]), base)
    s.close()


def test_a_refused_process_changes_nothing(pkg, dev):
    """refused_calls_change_nothing at the smallest plan"""
    refused_calls_change_nothing(pkg, dev, SR.CUT_SIZES[0])


def test_a_refused_process_changes_nothing_at_the_largest_plan(pkg, dev):
    """refused_calls_change_nothing at 4096 / 1024 / 2: the longest carried record and partial line, across refused calls
    and reset()"""
    assert (4096, 1024, 2) in SR.CUT_SIZES
    refused_calls_change_nothing(pkg, dev, (4096, 1024, 2))


def test_end_to_end(pkg, dev):
    """2^21 samples of noise plus a carrier, packed by the package's pack24, through Channelizer (1024, hop 512) -> Tuner
    (T = 64, R = 4: 39062.5 S/s) -> Scope (nfft 256, hop 128, avg 2: 152.6 Hz per bin) on one stream.  Two slots watch
    two receivers tuned 1 kHz apart: the carrier's peak sits in the bin each tuning word predicts, the two differ by the
    predicted count, and the lines are within TOL_SCOPE of the reference on a host copy of the tuner's own output."""
    import torch
    M, hop, T, R, ns, fs = 1024, 512, 64, 4, 1 << 21, 80.0e6
    nfft, shop, avg = 256, 128, 2
    fc = 300 * fs / M + 3000.0
    L = pkg.ddc_lib()
    words = [int(L.pddc_nco_freg(fc - 2100.0, fs)), int(L.pddc_nco_freg(fc - 1100.0, fs))]
    gen = torch.Generator(device="cpu").manual_seed(41)
    sig = (0.05 * torch.randn((ns, 2), generator=gen, dtype=torch.float32)).to(dev)
    ph = (2.0 * np.pi * fc / fs) * torch.arange(ns, dtype=torch.float64, device=dev)
    sig[:, 0] += (0.2 * torch.cos(ph)).float()
    sig[:, 1] += (0.2 * torch.sin(ph)).float()
    packed = pkg.pack24_f32(sig)
    ch = pkg.Channelizer(M, pkg.tuner_prototype(M, 4), hop)
    tu = pkg.Tuner(ch, words, pkg.tuner_lowpass(T, R), R)
    sc = pkg.Scope(2, [0, 1], nfft, shop, avg)
    zv = tu.process(ch.process(packed))
    lines = sc.process(zv)
    torch.cuda.synchronize()
    n = zv.shape[1]
    got = lines.cpu().numpy()
    assert got.shape == (2, SR.nlines_of(n, nfft, shop, avg), nfft) and got.shape[1] >= 3 and zv.stride(0) >= n
    want = SR.scope_ref(zv.cpu().numpy(), nfft, shop, avg, SR.hann(nfft))
    e = SR.err(got, want)
    binw = fs / (hop * R) / nfft
    offs = [(fc - wd * fs / 2.0 ** 32) / binw for wd in words]
    pred = [int(np.rint(o)) % nfft for o in offs]
    peak = [sorted(set(got[j].argmax(axis=-1).tolist())) for j in range(2)]
    print(f"end to end: {n} values per receiver, err {e:.2e}, carrier at bins {offs[0]:.2f} and {offs[1]:.2f}, peaks {peak}")
    assert all(abs(o - np.rint(o)) < 0.3 for o in offs) and pred == [14, 7]
    assert peak == [[pred[0]], [pred[1]]] and peak[0][0] - peak[1][0] == pred[0] - pred[1]
    assert e <= SR.TOL_SCOPE
    for o in (sc, tu, ch):
        o.close()
