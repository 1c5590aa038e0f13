"""Adapt (pddc_adapt_*, k_adapt) on the GPU against the numpy float32 reference (tests/adapt_ref.py) fed the very float32
arrays uploaded.  Every comparison is by int32 views and exact equality: there are no tolerances.  The inputs'
preconditions (denormal products and weights, every mode in every lane group, finite outputs) are asserted in
tests/test_adapt_cpu.py."""
import ctypes as C
import types

import numpy as np
import pytest

import adapt_ref as AR
import demod_ref as DR
import tuner_ref as TR

pytestmark = pytest.mark.gpu
K0, N0 = AR.K0, AR.N0
FEW = 37


def run(pkg, x, rx, T, D, cuts=None, before=None):
    """all of x (torch [K, n]) through a fresh Adapt in the given batches -> numpy (out, weights); before(i, s) is called
    ahead of batch i"""
    import torch
    s = pkg.Adapt(rx, T, D, eps=AR.EPS)
    outs, off = [], 0
    for i, b in enumerate(cuts or [x.shape[1]]):
        if before:
            before(i, s)
        o = s.process(x[:, off:off + b])
        assert o.shape == (len(rx), b)
        outs.append(o)
        off += b
    assert off == x.shape[1]
    w = s.read_weights()
    s.close()
    return torch.cat(outs, dim=1).cpu().numpy(), w


def same(got, want, what=""):
    for name, g, w in zip(("out", "weights"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        assert np.array_equal(AR.bits(g), AR.bits(w)), (what, name, np.argwhere(AR.bits(g) != AR.bits(w))[:4].tolist())


def rows_of(r, sl):
    return tuple(v[sl] for v in r)


@pytest.fixture(scope="module")
def series(dev):
    """the input, its upload, and the reference at the first (T, D) for all K0 receivers: computed once, never changed"""
    import torch
    x, rx = AR.gpu_series(), AR.interleaved_rx(K0)
    T, D = AR.GPU_SETS[0]
    out, w, _ = AR.adapt_ref(x, rx, T, D)
    assert np.isfinite(out).all()
    return types.SimpleNamespace(x=x, rx=rx, xd=torch.from_numpy(x).to(dev), want=(out, w))


@pytest.mark.parametrize("T,D", AR.GPU_SETS)
def test_bits_against_the_reference(pkg, dev, series, T, D):
    """K = 1024 at (T, D) = (64, 1) and K = 37 at (16, 1), (32, 7), (128, 256), (64, 255), n = 3000; modes, steps and leaks
    interleaved receiver by receiver, a row of zeros, a row that goes silent after 1000 samples, two rows small enough
    for denormal products and weights: out and read_weights() equal adapt_ref's."""
    if (T, D) == AR.GPU_SETS[0]:
        same(run(pkg, series.xd, series.rx, T, D), series.want, (T, D))
        return
    x, rx = series.x[:FEW], series.rx[:FEW]
    got = run(pkg, series.xd[:FEW].contiguous(), rx, T, D)
    same(got, AR.adapt_ref(x, rx, T, D)[:2], (T, D))
    assert not AR.bits(got[0][AR.ZERO_ROW]).any() and not AR.bits(got[1][AR.ZERO_ROW]).any()


@pytest.mark.parametrize("T,D", [(64, 1), (128, 256), (16, 1)])
def test_bits_against_the_cut_and_the_company(pkg, dev, series, T, D):
    """One batch against batches of 0, 1, 2, D, D + T - 1, TT - 1, TT, TT + 1, 3 TT + 5 and the rest for K = 1024; the
    receiver order reversed (with the cuts reversed); K = 7 and K = 1 slices against the same rows among the 1024."""
    TT = pkg.adapt_tile_outputs()
    cuts = [0, 1, 2, D, D + T - 1, TT - 1, TT, TT + 1, 3 * TT + 5]
    cuts.append(N0 - sum(cuts))
    assert cuts[-1] > 0
    x, rx = series.xd, series.rx
    one = run(pkg, x, rx, T, D)
    if (T, D) == AR.GPU_SETS[0]:
        same(one, series.want, "one batch")
    same(run(pkg, x, rx, T, D, cuts), one, "cut")
    rev = run(pkg, x.flip(0).contiguous(), rx[::-1], T, D, cuts[::-1])
    same(rev, rows_of(one, slice(None, None, -1)), "reversed")
    few = run(pkg, x[500:507].contiguous(), rx[500:507], T, D, cuts)
    same(few, rows_of(one, slice(500, 507)), "K 7")
    for j in (0, 1, 2, 3, AR.TINY_ROW, 63, 64, 1023):
        alone = run(pkg, x[j:j + 1].contiguous(), rx[j:j + 1], T, D, cuts)
        same(alone, rows_of(one, slice(j, j + 1)), f"alone {j}")


def test_strides_and_in_place(pkg, dev):
    """The input is the view Demod.process returns behind a small Tuner, in a buffer of capacity > n (row stride > n); out
    with capacity > n, the padding keeps its fill value; out is a gives the bits of out of place."""
    import torch
    M, hop, T, Rd, K, S = 1024, 512, 64, 4, 13, 1200
    gen = torch.Generator(device="cpu").manual_seed(5)
    rows = torch.view_as_complex(torch.randn((S, M, 2), generator=gen, dtype=torch.float32)).to(dev)
    g = types.SimpleNamespace(nchan=M, hop=hop, device=0, first=0, count=M)
    t = pkg.Tuner(g, TR.receiver_set(M, K), pkg.tuner_lowpass(T, Rd), Rd)
    z = t.process(rows)
    n = z.shape[1]
    d = pkg.Demod([(pkg.PDDC_DEMOD_AM, 0, pkg.PDDC_DEMOD_DCBLOCK)] * K)
    abuf = torch.full((K, n + 5), 3.0, dtype=torch.float32, device=dev)
    av = d.process(z, out=abuf)
    assert av.data_ptr() == abuf.data_ptr() and av.stride(0) == n + 5 > n > 256
    rx = AR.interleaved_rx(K)
    for Ta, Da in ((32, 7), (128, 256)):
        xin = av.cpu().numpy()
        want = AR.adapt_ref(xin, rx, Ta, Da)[:2]
        assert any(not np.array_equal(want[0][j], xin[j]) for j in range(K))
        s = pkg.Adapt(rx, Ta, Da, eps=AR.EPS)
        obuf = torch.full((K, n + 11), 7.0, dtype=torch.float32, device=dev)
        out = s.process(av, out=obuf)
        assert out.data_ptr() == obuf.data_ptr() and out.shape == (K, n)
        same((out.cpu().numpy(), s.read_weights()), want, "strided")
        assert bool((obuf[:, n:] == 7.0).all()) and bool((abuf[:, n:] == 3.0).all())
        assert np.array_equal(AR.bits(av.cpu().numpy()), AR.bits(xin))
        s.reset()
        keep = abuf.clone()
        out2 = s.process(av, out=av)                           # in place
        assert out2.data_ptr() == abuf.data_ptr()
        same((out2.cpu().numpy(), s.read_weights()), want, "in place")
        assert bool((abuf[:, n:] == 3.0).all())
        abuf.copy_(keep)
        s.close()
    d.close()
    t.close()


def test_set_rx_between_batches(pkg, dev, series):
    """Mode, step and leak changes and restarts on some receivers against the streaming reference, bit for bit; the
    receivers that were not touched have the bits of a run without the changes; a bad call is refused and changes
    nothing."""
    K, T, D = 12, 32, 7
    cuts = [700, 1, 999, 1300]
    rows = slice(100, 100 + K)
    rx = series.rx[rows]
    x = series.xd[rows].contiguous()
    R = AR.RESTART
    changes = {1: [(2, AR.OFF, 0.5, 0.0, 0), (3, AR.NR, 1.25, 2.0 ** -8, 0), (4, rx[4][0], rx[4][1], rx[4][2], R)],
               2: [(2, AR.NOTCH, 0.5, 0.0, 0), (7, AR.NOTCH, 0.125, 0.0, R), (7, AR.NR, 0.125, 0.0, 0)],   # the restart stays asked for
               3: [(0, AR.NR, 0.75, 2.0 ** -4, 0), (3, AR.OFF, 1.25, 2.0 ** -8, R), (9, AR.NOTCH, 1.0, 0.5, 0)]}
    nan, inf = float("nan"), float("inf")
    bad = ((1, 3, 0.5, 0.0, 0), (1, 1, 0.0, 0.0, 0), (1, 1, 2.0, 0.0, 0), (1, 1, nan, 0.0, 0), (1, 1, inf, 0.0, 0),
           (1, 1, 0.5, 1.0, 0), (1, 1, 0.5, -0.25, 0), (1, 1, 0.5, nan, 0), (1, 1, 0.5, 0.0, 2), (K, 1, 0.5, 0.0, 0),
           (-1, 1, 0.5, 0.0, 0))

    def before(i, s):
        for c in changes.get(i, ()):
            s.set_rx(*c)
        for b in bad:
            with pytest.raises(pkg.PddcError) as e:
                s.set_rx(*b)
            assert e.value.code == pkg.PDDC_EINVAL

    got = run(pkg, x, rx, T, D, cuts, before)
    clean = run(pkg, x, rx, T, D, cuts)
    touched = {c[0] for cs in changes.values() for c in cs}
    assert 1 not in touched
    for j in range(K):
        if j not in touched:
            same(rows_of(got, slice(j, j + 1)), rows_of(clean, slice(j, j + 1)), f"untouched {j}")
    ref = AR.AdaptRef(rx, T, D)
    outs, off = [], 0
    for i, b in enumerate(cuts):
        for c in changes.get(i, ()):
            ref.set_rx(*c)
        outs.append(ref.process(series.x[rows, off:off + b]))
        off += b
    same(got, (np.concatenate(outs, axis=1), ref.weights), "set_rx")
    assert all(not np.array_equal(got[0][j], clean[0][j]) for j in touched)


def test_a_refused_process_changes_nothing(pkg, dev, series):
    """process calls refused for capacity (each stride), for a misaligned or missing pointer and for a partial overlap of
    out with a, between the batches: the next correct call's bits are those of an object that never saw them.  reset
    starts the series again with the first run's bits."""
    import torch
    K, T, D = 9, 16, 1
    cuts = [700, 300, 2000]
    rows = slice(300, 300 + K)
    rx = series.rx[rows]
    x = series.xd[rows].contiguous()
    clean = run(pkg, x, rx, T, D, cuts)
    L = pkg.ddc_lib()
    EINVAL, ECAP = pkg.PDDC_EINVAL, pkg.PDDC_ECAPACITY

    def disturb(i, s):
        b = cuts[i]
        with pytest.raises(pkg.PddcError) as e:
            s.process(x[:, :b], out=torch.empty((K, b - 1), dtype=torch.float32, device=dev))
        assert e.value.code == ECAP
        o = torch.empty((K, b), dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream().cuda_stream

        def call(ap=x.data_ptr(), n=b, as_=N0, op=o.data_ptr(), os_=b):
            return L.pddc_adapt_process(s._h, ap, n, as_, op, os_, stream)

        assert call(as_=b - 1) == ECAP and call(os_=b - 1) == ECAP
        assert call(ap=x.data_ptr() + 2) == EINVAL and call(op=o.data_ptr() + 1) == EINVAL
        assert call(ap=None) == EINVAL and call(op=None) == EINVAL
        assert call(op=x.data_ptr() + 4, os_=N0) == EINVAL                                       # out over a, shifted
        assert call(op=x.data_ptr(), os_=N0 - 1) == EINVAL                                       # out is a, another stride
        assert call(op=x.data_ptr() + 4 * (N0 * (K - 1) + b - 1), os_=b) == EINVAL               # out's first value is a's last
        assert call(ap=None, n=0, as_=0, op=None, os_=0) == pkg.PDDC_OK
        assert L.pddc_adapt_read_weights(s._h, None, stream) == EINVAL

    got = run(pkg, x, rx, T, D, cuts, disturb)
    same(got, clean, "refused")
    s = pkg.Adapt(rx, T, D, eps=AR.EPS)                         # reset starts the series again
    assert not AR.bits(s.read_weights()).any()
    first = s.process(x).clone()
    w1 = s.read_weights()
    s.reset()
    assert not AR.bits(s.read_weights()).any()
    second = s.process(x)
    same((first.cpu().numpy(), w1), clean, "first")
    same((second.cpu().numpy(), s.read_weights()), clean, "after reset")
    s.close()


def test_end_to_end(pkg, O, dev):
    """2^19 samples with two tones in one channel's upper sideband -- a strong one 700 Hz and a weak one 1900 Hz above the
    (absent) carrier -- and a little noise, packed by the package's pack24, through Channelizer (1024, hop 512) -> Tuner
    (T = 64, R = 4) -> Demod SSB on one stream; an Adapt (T = 16, D = 1) with one receiver in NOTCH and one in NR on the
    same series.  The outputs and weights equal adapt_ref on the downloaded audio.  What each output keeps of the two
    tones over the second half is compared with the reference's own figures: the very same numbers, and the directions the
    reference shows -- the notch takes more off the strong tone than off the weak one, and more off either than the noise
    reduction does (both tones are predictable: on the CPU references of the chain the notch kept 0.007 of the strong
    and 0.23 of the weak tone, the noise reduction 0.99 and 1.2)."""
    import torch
    c = DR.CHAIN
    ns, strong, weak, noise = 1 << 19, 0.45, 0.03, 0.003
    f_strong, f_weak = 700.0, 1900.0
    n = np.arange(ns, dtype=np.int64)
    t = n.astype(np.float64) / DR.FS
    ph = 2.0 * np.pi * ((DR.CARRIER_WORD * n) & DR.MASK).astype(np.float64) / 2.0 ** 32
    rng = np.random.default_rng(78)
    xs = strong * np.exp(1j * (ph + 2.0 * np.pi * f_strong * t)) + weak * np.exp(1j * (ph + 2.0 * np.pi * f_weak * t))
    xs = xs + noise * (rng.standard_normal(ns) + 1j * rng.standard_normal(ns))
    sig = np.stack([xs.real, xs.imag], axis=1).astype(np.float32)
    packed = pkg.pack24_f32(torch.from_numpy(sig).to(dev))
    assert np.array_equal(packed.cpu().numpy(), O.pack24_f32(sig))
    word, bfo = pkg.demod_ssb_words(DR.FS, DR.OUT_RATE, DR.CARRIER_HZ, DR.SSB_BAND[0], DR.SSB_BAND[1], True)
    w, h = pkg.tuner_prototype(c["nchan"], c["proto_taps"]), pkg.tuner_lowpass(c["ntaps"], c["decim"])
    ch = pkg.Channelizer(c["nchan"], w, c["hop"])
    tu = pkg.Tuner(ch, [word] * 2, h, c["decim"])
    d = pkg.Demod([(pkg.PDDC_DEMOD_SSB, bfo, 0)] * 2)
    rx = [(pkg.PDDC_ADAPT_NOTCH, 0.5, 2.0 ** -10), (pkg.PDDC_ADAPT_NR, 0.5, 2.0 ** -10)]
    T, D = 16, 1
    s = pkg.Adapt(rx, T, D, eps=AR.EPS)
    a = d.process(tu.process(ch.process(packed.clone())))
    out = s.process(a)
    an, on = a.cpu().numpy(), out.cpu().numpy()
    assert an.shape == on.shape == (2, 239) and np.array_equal(AR.bits(an[0]), AR.bits(an[1]))
    want = AR.adapt_ref(an, rx, T, D)[:2]
    same((on, s.read_weights()), want, "chain")
    lo = 120
    fs, fw = f_strong / DR.OUT_RATE, f_weak / DR.OUT_RATE

    def kept(v):
        """what v keeps of the strong and of the weak tone, relative to the input"""
        return (AR.tone_part(v, fs, lo)[0] / AR.tone_part(an[0], fs, lo)[0], AR.tone_part(v, fw, lo)[0] / AR.tone_part(an[0], fw, lo)[0])

    got_notch, got_nr, ref_notch, ref_nr = kept(on[0]), kept(on[1]), kept(want[0][0]), kept(want[0][1])
    print(f"kept of (strong, weak): notch {got_notch[0]:.4f} {got_notch[1]:.4f} (reference {ref_notch[0]:.4f} {ref_notch[1]:.4f}), "
          f"nr {got_nr[0]:.4f} {got_nr[1]:.4f} (reference {ref_nr[0]:.4f} {ref_nr[1]:.4f})")
    assert got_notch == ref_notch and got_nr == ref_nr
    # the directions, the reference's own: whatever it shows, the device shows
    for f in (lambda k_notch, k_nr: k_notch[0] < k_notch[1], lambda k_notch, k_nr: k_notch[0] < k_nr[0],
              lambda k_notch, k_nr: k_notch[1] < k_nr[1]):
        assert f(got_notch, got_nr) == f(ref_notch, ref_nr)
    # and on this input the reference does show them (a fact of the reference alone)
    assert ref_notch[0] < ref_notch[1] and ref_notch[0] < ref_nr[0] and ref_notch[1] < ref_nr[1]
    for obj in (s, d, tu, ch):
        obj.close()
