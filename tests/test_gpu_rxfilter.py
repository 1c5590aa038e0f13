"""RxFilter (pddc_rxfilter_*, k_rxfilter) on the GPU against the numpy reference in double (tests/rxfilter_ref.py).
Tolerance: rxfilter_ref.TOL_RXFILTER, 7 x the float32 model's worst case on the parity test's very inputs
(tests/test_rxfilter_cpu.py), never taken from k_rxfilter."""
import numpy as np
import pytest

import demod_ref as DR
import rxfilter_ref as RR

pytestmark = pytest.mark.gpu


def run(pkg, z, bank, sel, cuts=None, before=None, out_pad=0):
    """all of z (torch complex64 [nrx, n], any row stride) through a fresh RxFilter in the given batches -> complex64
    [nrx, n]; before(i, f) is called ahead of batch i; out_pad > 0: every batch is written into a view of a tensor whose
    rows lie that many values further apart"""
    import torch
    f = pkg.RxFilter(bank, sel)
    outs, off = [], 0
    for i, b in enumerate(cuts or [z.shape[1]]):
        if before:
            before(i, f)
        out = torch.zeros((z.shape[0], b + out_pad), dtype=torch.complex64, device=z.device) if out_pad else None
        o = f.process(z[:, off:off + b], out=out)
        assert o.shape == (z.shape[0], b) and o.dtype == torch.complex64
        if out_pad:
            assert o.stride(0) == b + out_pad
        outs.append(o)
        off += b
    assert off == z.shape[1]
    torch.cuda.synchronize()
    f.close()
    return torch.cat(outs, dim=1)


def bits(t):
    import torch
    return torch.view_as_real(t.contiguous()).contiguous().view(torch.int32)


def err(out, ref):
    return float(np.max(np.abs(out.cpu().numpy().astype(np.complex128) - ref))) if ref.size else 0.0


_REFS = {}


def parity_ref(nrx, B, T):
    """the double reference of the parity case, computed once"""
    if (nrx, B, T) not in _REFS:
        _REFS[(nrx, B, T)] = RR.rxfilter_ref(RR.parity_inputs(nrx), RR.parity_bank(B, T), RR.select(nrx, B))
    return _REFS[(nrx, B, T)]


@pytest.mark.parametrize("nrx", [1, 5, 9, 1024])
def test_parity(pkg, dev, nrx):
    """(B, T) of (1, 1), (3, 2), (4, 64), (64, 255), (5, 256), receiver j on filter (7 j + 3) mod B: 700 inputs per receiver
    (nrx = 1024: 300), re and im uniform in [-1, 1], one batch; |out - rxfilter_ref| <= TOL_RXFILTER."""
    import torch
    z = RR.parity_inputs(nrx)
    zd = torch.from_numpy(z).to(dev)
    worst = 0.0
    for B, T in RR.SHAPES:
        out = run(pkg, zd, RR.parity_bank(B, T), RR.select(nrx, B))
        ref = parity_ref(nrx, B, T)
        assert tuple(out.shape) == ref.shape == z.shape
        e = err(out, ref)
        worst = max(worst, e)
        print(f"nrx {nrx} B {B} T {T}: err {e:.2e} (bar {RR.TOL_RXFILTER:.2e})")
        assert e <= RR.TOL_RXFILTER, (nrx, B, T, e)
    print(f"nrx {nrx}: worst {worst:.2e}")


@pytest.mark.parametrize("T,cuts", [(64, RR.CUTS), (256, [0, 1, 100, 2, 150, 0, 254, 3, 190])])
def test_bits_against_the_cut_and_the_company(pkg, dev, T, cuts):
    """9 receivers, 700 inputs.  One batch against cuts with batches of 0, 1 and fewer than T - 1 inputs, so that the carried
    record spans several batches (T = 64: 0, 1, 2, 30, 0, 31, 255, 256, 125; T = 256: five batches in a row stay below
    255), and against 40 batches of one input followed by 660: equal int32 views.  Receiver j's bits are the same alone,
    as index 0 or 6 of seven receivers with other filters around it, and with input and output rows n or n + 13 apart."""
    import torch
    assert sum(cuts) == 700
    B = 4
    bank, sel = RR.parity_bank(B, T), RR.select(9, B)
    z = torch.from_numpy(RR.parity_inputs(9)).to(dev)
    one = run(pkg, z, bank, sel)
    assert torch.isfinite(torch.view_as_real(one)).all()
    assert err(one, parity_ref(9, B, T) if T == 64 else RR.rxfilter_ref(RR.parity_inputs(9), bank, sel)) <= RR.TOL_RXFILTER
    assert torch.equal(bits(run(pkg, z, bank, sel, cuts)), bits(one))
    assert torch.equal(bits(run(pkg, z, bank, sel, [1] * 40 + [660])), bits(one))
    for j in (2, 8):
        alone = run(pkg, z[j:j + 1], bank, [sel[j]], cuts)
        assert torch.equal(bits(alone[0]), bits(one[j])), j
        others = [k for k in range(9) if k != j][:6]
        for at in (0, 6):
            rows = others[:at] + [j] + others[at:]
            company = [(sel[j] + 1 + i) % B for i in range(6)]         # filters other than j's among them
            fs = company[:at] + [sel[j]] + company[at:]
            seven = run(pkg, z[rows].contiguous(), bank, fs, cuts)
            assert torch.equal(bits(seven[at]), bits(one[j])), (j, at)
    wide = torch.zeros((9, 713), dtype=torch.complex64, device=dev)
    wide[:, :700] = z
    view = wide[:, :700]
    assert view.stride(0) == 713
    assert torch.equal(bits(run(pkg, view, bank, sel, cuts, out_pad=13)), bits(one))
    assert torch.equal(bits(run(pkg, view, bank, sel)), bits(one))
    assert torch.equal(bits(run(pkg, z, bank, sel, out_pad=13)), bits(one))


@pytest.mark.parametrize("T", [256, 1])
def test_tile_seams(pkg, dev, T):
    """Batches of TT - 1, TT, TT + 1 and 2 TT + 1 outputs, 5 receivers (a ragged last group): against the reference, and
    the bits of the same series cut in two at TT - 1 and at TT."""
    import torch
    TT = pkg.rxfilter_tile_outputs()
    B = 3
    bank, sel = RR.parity_bank(B, T), RR.select(5, B)
    zfull = np.random.default_rng(TT).uniform(-1.0, 1.0, (5, 2 * TT + 1, 2)).astype(np.float32).view(np.complex64)[..., 0]
    ref = RR.rxfilter_ref(zfull, bank, sel)                            # causal: a prefix's outputs are the prefix of these
    for n in (TT - 1, TT, TT + 1, 2 * TT + 1):
        zd = torch.from_numpy(np.ascontiguousarray(zfull[:, :n])).to(dev)
        one = run(pkg, zd, bank, sel)
        e = err(one, ref[:, :n])
        print(f"T {T}: {n} outputs, err {e:.2e}")
        assert e <= RR.TOL_RXFILTER, (T, n, e)
        if n == 2 * TT + 1:
            for cut in (TT - 1, TT):
                assert torch.equal(bits(run(pkg, zd, bank, sel, [cut, n - cut])), bits(one)), (T, cut)


def test_filter_change(pkg, dev):
    """Three batches; set_rx of receivers 1 and 3 between the first and the second, receiver 1 set back between the second
    and the third.  Per segment the outputs are bit-equal to those of an object that had that segment's filters from
    the start and was fed the same inputs (what is carried is inputs); the whole is within TOL_RXFILTER of the double
    reference given the same changes, and bit-equal under another cut with the same change points."""
    import torch
    B, T = 4, 64
    bank = RR.parity_bank(B, T)
    z = RR.parity_inputs(5)
    zd = torch.from_numpy(z).to(dev)
    sel0, sel1, sel2 = [0, 1, 2, 3, 0], [0, 3, 2, 0, 0], [0, 1, 2, 0, 0]
    a, b = 200, 450                                                    # the change points

    def changes(at_a, at_b):
        def before(i, f):
            if i == at_a:
                f.set_rx(1, 3)
                f.set_rx(3, 0)
            if i == at_b:
                f.set_rx(1, 1)
        return before

    got = run(pkg, zd, bank, sel0, [a, b - a, 700 - b], before=changes(1, 2))
    for s, (lo, hi) in zip((sel0, sel1, sel2), ((0, a), (a, b), (b, 700))):
        steady = run(pkg, zd, bank, s)
        assert torch.equal(bits(got[:, lo:hi]), bits(steady[:, lo:hi])), (lo, hi)
    ref = RR.run_cuts(RR.RxFilterRef(bank, sel0), z, [a, b - a, 700 - b], before=changes(1, 2))
    e = err(got, ref)
    print(f"filter change: err {e:.2e}")
    assert e <= RR.TOL_RXFILTER
    assert not np.array_equal(ref[1, a:b], RR.rxfilter_ref(z, bank, sel0)[1, a:b])
    other = run(pkg, zd, bank, sel0, [1, a - 1, 0, 100, b - a - 100, 30, 700 - b - 30], before=changes(2, 5))
    assert torch.equal(bits(other), bits(got))


def test_pass_through(pkg, dev):
    """a bank row [1, 0, ..., 0] returns its input: equal values (-0 comes out as +0)"""
    import torch
    T = 64
    bank = RR.parity_bank(2, T).copy()
    bank[1] = 0.0
    bank[1, 0] = 1.0
    z = RR.parity_inputs(5).copy()
    z[2, 10] = complex(-0.0, 0.0)
    z[2, 11] = complex(0.0, -0.0)
    zd = torch.from_numpy(z).to(dev)
    out = run(pkg, zd, bank, [1, 0, 1, 1, 0], [100, 600])
    assert torch.equal(out[[0, 2, 3]], zd[[0, 2, 3]])
    assert not torch.equal(out[1], zd[1])


def test_guard(pkg, dev):
    """z and out are views of wider tensors that hold NaN beyond n: the outputs are finite and right, the columns >= n of
    `out` are untouched."""
    import torch
    B, T, n = 4, 64, 700
    bank, sel = RR.parity_bank(B, T), RR.select(9, B)
    nan = complex(float("nan"), float("nan"))
    zw = torch.full((9, n + 40), nan, dtype=torch.complex64, device=dev)
    zw[:, :n] = torch.from_numpy(RR.parity_inputs(9)).to(dev)
    ow = torch.full((9, n + 29), nan, dtype=torch.complex64, device=dev)
    f = pkg.RxFilter(bank, sel)
    o = f.process(zw[:, :n], out=ow)
    torch.cuda.synchronize()
    f.close()
    assert o.data_ptr() == ow.data_ptr() and o.shape == (9, n)
    assert err(o, parity_ref(9, B, T)) <= RR.TOL_RXFILTER
    assert torch.isnan(torch.view_as_real(ow[:, n:])).all()


def test_a_refused_call_changes_nothing_and_reset(pkg, dev):
    """PDDC_ECAPACITY for a short `out` or a stride below n, PDDC_EINVAL for overlapping input and output, for NULL or
    misaligned pointers and for a bad set_rx, between the batches: the next good batch gives the bits of an undisturbed
    run.  n = 0 is valid.  After reset the outputs repeat those after create."""
    import torch
    B, T = 4, 64
    bank, sel = RR.parity_bank(B, T), RR.select(9, B)
    nrx, n = 9, 700
    cuts = [300, 150, 250]
    z = torch.from_numpy(RR.parity_inputs(9)).to(dev)
    clean = run(pkg, z, bank, sel, cuts)
    lib = pkg.ddc_lib()

    def disturb(i, f):
        b = cuts[i]
        with pytest.raises(pkg.PddcError) as e:
            f.process(z[:, :b], out=torch.empty((nrx, b - 1), dtype=torch.complex64, device=dev))
        assert e.value.code == pkg.PDDC_ECAPACITY
        buf = torch.zeros((nrx, 2 * n), dtype=torch.complex64, device=dev)
        buf[:, :n] = z
        for shift in (0, 1, b - 1):                                   # in place, and one row's output over its input's tail
            with pytest.raises(pkg.PddcError) as e:
                f.process(buf[:, :b], out=buf[:, shift:])
            assert e.value.code == pkg.PDDC_EINVAL
        for rx, flt in ((-1, 0), (nrx, 0), (0, -1), (0, B)):
            with pytest.raises(pkg.PddcError) as e:
                f.set_rx(rx, flt)
            assert e.value.code == pkg.PDDC_EINVAL
        o = torch.empty((nrx, b), dtype=torch.complex64, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        call = lambda *args: lib.pddc_rxfilter_process(f._h, *args, st)
        assert call(z.data_ptr(), b, b - 1, o.data_ptr(), b) == pkg.PDDC_ECAPACITY
        assert call(z.data_ptr(), b, n, o.data_ptr(), b - 1) == pkg.PDDC_ECAPACITY
        assert call(z.data_ptr() + 4, b, n, o.data_ptr(), b) == pkg.PDDC_EINVAL
        assert call(z.data_ptr(), b, n, o.data_ptr() + 4, b) == pkg.PDDC_EINVAL
        assert call(None, b, n, o.data_ptr(), b) == pkg.PDDC_EINVAL
        assert call(z.data_ptr(), b, n, None, b) == pkg.PDDC_EINVAL
        assert call(None, 0, 0, None, 0) == pkg.PDDC_OK
        assert torch.equal(f.process(z[:, :0]), z[:, :0])

    got = run(pkg, z, bank, sel, cuts, before=disturb)
    assert torch.equal(bits(got), bits(clean))
    f = pkg.RxFilter(bank, sel)
    first = [f.process(z[:, :300]), f.process(z[:, 300:])]
    f.reset()
    again = f.process(z)
    torch.cuda.synchronize()
    assert torch.equal(bits(torch.cat(first, dim=1)), bits(again)) and torch.equal(bits(again), bits(clean))
    f.close()


def tone_levels(y, freqs, skip):
    """least-squares amplitudes of complex exponentials of the given frequencies (cycles per value) in y[skip:]"""
    m = np.arange(skip, y.size)
    A = np.stack([np.exp(2j * np.pi * f * m) for f in freqs], axis=1)
    c, *_ = np.linalg.lstsq(A, y[skip:], rcond=None)
    return np.abs(c)


def test_behind_the_tuner(pkg, O, dev):
    """Channelizer (M = 1024, hop 512, 2^17 samples: 249 rows) -> Tuner (T = 64, R = 1) with two receivers on one word ->
    RxFilter with a wide (half width 0.25 of the tuner's output rate) and a narrow (0.08) filter of 65 taps from
    rxfilter_bank.  The packed input holds two 24-bit tones, 0.02 and 0.11 cycles per tuner output above the word: the
    first inside both pass-bands, the second inside the wide one only.  The device's RxFilter output is within
    TOL_RXFILTER of RxFilterRef applied to a host copy of the device's own tuner output; the outer tone's level in the
    narrow receiver relative to the wide one lies within 1 dB of what the reference gives (and both tones pass the wide
    one, the outer one, on the narrow filter's skirt, comes out about 39 dB down: at least 20).  Then Demod (AM) reads the RxFilter view, whose rows lie
    further apart than n, without a copy."""
    import torch
    M, hop, Tt, ns, Tf = 1024, 512, 64, 1 << 17, 65
    word = 300 << 22
    f1, f2 = 0.02, 0.11
    n = np.arange(ns, dtype=np.int64)
    ph = ((word * n) & 0xFFFFFFFF).astype(np.float64) / 2.0 ** 32
    x = 0.3 * np.exp(2j * np.pi * (ph + f1 / hop * n)) + 0.3 * np.exp(2j * np.pi * (ph + f2 / hop * n))
    i = np.clip(np.rint(x.real * 8388607.0), -8388608, 8388607).astype(np.int64)
    q = np.clip(np.rint(x.imag * 8388607.0), -8388608, 8388607).astype(np.int64)
    packed = torch.from_numpy(O.pack24(i, q).reshape(-1)).to(dev)
    bank = pkg.rxfilter_bank(1.0, [0.25, 0.08], Tf)
    ch = pkg.Channelizer(M, pkg.tuner_prototype(M, 4), hop)
    tu = pkg.Tuner(ch, [word, word], pkg.tuner_lowpass(Tt, 1), 1)
    rf = pkg.RxFilter(bank, [0, 1])
    de = pkg.Demod([(DR.AM, 0, 0), (DR.AM, 0, 0)])
    rows = ch.process(packed)
    assert rows.shape[0] == 249
    z = tu.process(rows)
    nz = z.shape[1]
    assert nz == 249 - (Tt - 1)
    buf = torch.zeros((2, nz + 7), dtype=torch.complex64, device=dev)
    y = rf.process(z, out=buf)
    assert y.stride(0) == nz + 7 and y.data_ptr() == buf.data_ptr()
    a = de.process(y)
    torch.cuda.synchronize()
    zh = z.cpu().numpy()
    ref = RR.rxfilter_ref(zh, bank, [0, 1])
    e = err(y, ref)
    yh = y.cpu().numpy().astype(np.complex128)
    lv, lr = [tone_levels(v, (f1, f2), Tf - 1) for v in yh], [tone_levels(v, (f1, f2), Tf - 1) for v in ref]
    got_db, ref_db = 20 * np.log10(lv[1][1] / lv[0][1]), 20 * np.log10(lr[1][1] / lr[0][1])
    print(f"behind the tuner: {nz} values, err {e:.2e}; wide {lv[0]}, narrow {lv[1]}; outer tone narrow / wide "
          f"{got_db:.2f} dB (reference {ref_db:.2f} dB)")
    assert float(np.max(np.abs(zh))) <= 1.0 and e <= RR.TOL_RXFILTER
    assert abs(got_db - ref_db) <= 1.0
    assert ref_db <= -20.0 and np.all(lr[0] > 0.25) and lr[1][0] > 0.25
    # AM of the view: sqrt(re^2 + im^2) of the device's own values, to the demodulator's own tolerance
    am = np.abs(yh)
    assert a.shape == (2, nz) and float(np.max(np.abs(a.cpu().numpy().astype(np.float64) - am))) <= DR.TOL_DEMOD[DR.AM]
    for o in (de, rf, tu, ch):
        o.close()
