"""Channelizer (pddc_channelizer_*, Channelizer) on the GPU against the numpy reference in double
(tests/channelizer_ref.py)."""
import time

import numpy as np
import pytest

import channelizer_ref as CR
import spectrum_ref as R

TOL = CR.TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lcg19(O):
    packed = O.lcg_bytes(6 << 19, 12345)
    return packed, R.to_complex(O, packed)


def synth(pkg, dev, ns, seed=12345):
    import torch
    d = torch.empty(6 * ns, dtype=torch.uint8, device=dev)
    pkg.check(pkg.ddc_lib().pddc_synth_lcg(d.data_ptr(), 6 * ns, seed, 0, torch.cuda.current_stream().cuda_stream))
    return d


def run(pkg, d, nchan, hop, w, cuts=None, first=0, count=None, ranges=None):
    """the whole of d through a fresh Channelizer in the given batches -> torch complex64 [rows, count] on the device
    (ranges: {batch index: (first, count)} applied before that batch; the rows then come back as a list per batch)"""
    import torch
    ch = pkg.Channelizer(nchan, w, hop, first, count)
    outs, off = [], 0
    for i, b in enumerate(cuts or [d.numel() // 6]):
        if ranges and i in ranges:
            ch.set_range(*ranges[i])
        want = ch.next_rows(b)
        y = ch.process(d[6 * off:6 * (off + b)].data_ptr(), b)
        assert y.shape == (want, ch.count)
        outs.append(y)
        off += b
    torch.cuda.synchronize()
    ch.close()
    return outs if ranges else torch.cat(outs, dim=0)


def bits(t):
    import torch
    return torch.view_as_real(t).contiguous().view(torch.int32)


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("nchan", CR.SIZES)
def test_parity(pkg, O, dev, lcg19, nchan, half):
    """e = max |y - ref| / max |ref| over all rows and channels <= TOL against the double reference, for every taps per
    branch P (P M <= 16384), the Kaiser prototype of channelizer_prototype and a seeded random one, 2^19 LCG samples, in
    one batch and in ragged batches down to 8 samples -- and the two bit-identical.
    Where TOL = 1.32e-6 comes from: the independent float32 model (complex64, float32 fold, scipy.fft; the same samples) is
    1.38e-7 .. 1.89e-7 away from the double reference in this metric, worst at M = 1024, P = 8, D = M with the random
    prototype (tests/test_channelizer_cpu.py::test_float32_model_against_double re-measures it); TOL is 7 x that worst
    case, the room for another factorisation and another order of the fold.  k_channelize measured 1.3e-7 .. 1.8e-7 here (2.0e-7 over 2^26 samples, test_full_size)."""
    import torch
    packed, x = lcg19
    d = torch.from_numpy(packed).to(dev)
    hop = nchan // 2 if half else nchan
    for P in CR.TAPS:
        if P * nchan > CR.MAX_PROTO:
            continue
        for name, w in (("kaiser", pkg.channelizer_prototype(nchan, P)), ("random", CR.random_prototype(nchan, P))):
            ref = CR.channelizer_ref(x, nchan, hop, w)
            y1 = run(pkg, d, nchan, hop, w)
            y2 = run(pkg, d, nchan, hop, w, cuts=R.ragged_cuts(packed.size // 6, nchan, 7 + nchan + P))
            e = CR.err(y1.cpu().numpy(), ref)
            same = y1.shape == y2.shape and torch.equal(bits(y1), bits(y2))
            print(f"M {nchan} D {hop} P {P} {name}: rows {y1.shape[0]} err {e:.2e} ragged identical {same}")
            assert y1.shape == ref.shape
            assert e <= TOL, (P, name, e)
            assert same, (P, name)


@pytest.mark.parametrize("combo", CR.combos(), ids=lambda c: "-".join(map(str, c)))
def test_weak_channel(pkg, O, dev, combo):
    """A tone of 0.7 on one channel's centre and one 80 dB below it on another's, 24-bit, the Kaiser prototype, 41 rows in
    one batch, the eight placements of channelizer_ref.weak_channels: in every row the weak channel is within
    TOL_WEAK_CHAN of its own reference value and the strong one within TOL of its own; the whole matrix is within TOL in
    test_parity's metric (which bounds the far channels); ragged batches give the bits of the one batch; and the list
    form over [weak, strong, a far channel] gives the bits of those columns.
    TOL_WEAK_CHAN = 7 x the independent float32 model's worst on these inputs, 2.67e-4 at M = 4096, P = 1
    (tests/test_channelizer_cpu.py::test_weak_channel_model re-measures it)."""
    import torch
    M, P, D = combo
    w = CR.kaiser_prototype(M, P)
    worst = dict(weak=0.0, strong=0.0, matrix=0.0)
    for r, (ks, kw) in enumerate(CR.weak_channels(M)):
        packed = CR.weak_packed(O, M, P, D, ks, kw)
        ref = CR.channelizer_ref(R.to_complex(O, packed), M, D, w)
        d = torch.from_numpy(packed).to(dev)
        y1 = run(pkg, d, M, D, w)
        y = y1.cpu().numpy()
        assert y.shape == ref.shape == (CR.WEAK_ROWS, M)
        figs = dict(weak=CR.weak_err(y, ref, kw), strong=CR.weak_err(y, ref, ks), matrix=CR.err(y, ref))
        worst = {k: max(v, figs[k]) for k, v in worst.items()}
        assert figs["weak"] <= CR.TOL_WEAK_CHAN, (ks, kw, figs)
        assert figs["strong"] <= TOL and figs["matrix"] <= TOL, (ks, kw, figs)
        y2 = run(pkg, d, M, D, w, cuts=R.ragged_cuts(packed.size // 6, M, 7 + M + P + r))
        assert y1.shape == y2.shape and torch.equal(bits(y1), bits(y2)), (ks, kw)
        cols = [kw, ks, CR.far_channel(M, ks, kw)]
        ch = pkg.Channelizer(M, w, D)
        ch.set_channels(cols)
        yl = ch.process(d)
        torch.cuda.synchronize()
        ch.close()
        assert yl.shape == (CR.WEAK_ROWS, 3) and torch.equal(bits(yl), bits(y1[:, cols])), (ks, kw)
    print(f"weak channel, M {M} P {P} D {D}: weak channel off by {worst['weak']:.2e} of itself (TOL_WEAK_CHAN "
          f"{CR.TOL_WEAK_CHAN:.2e}), strong {worst['strong']:.2e}, matrix {worst['matrix']:.2e} (TOL {TOL:.2e})")


def test_batches_shorter_than_the_prototype(pkg, dev, lcg19):
    import torch
    packed, x = lcg19
    M, P = 2048, 4
    w = pkg.channelizer_prototype(M, P)
    d = torch.from_numpy(packed).to(dev)
    ch = pkg.Channelizer(M, w, M // 2)
    assert ch.next_rows(P * M - 8) == 0 and ch.process(d.data_ptr(), P * M - 8).shape == (0, M)
    y = ch.process(d[6 * (P * M - 8):].data_ptr(), 8)
    torch.cuda.synchronize()
    assert y.shape == (1, M) and CR.err(y.cpu().numpy(), CR.channelizer_ref(x[:P * M], M, M // 2, w)) <= TOL
    # refused calls queue nothing and move nothing
    with pytest.raises(pkg.PddcError) as e:
        ch.process(d.data_ptr(), 12)
    assert e.value.code == pkg.PDDC_EINVAL
    with pytest.raises(pkg.PddcError) as e:
        ch.process(d.data_ptr() + 8, 8 * M)
    assert e.value.code == pkg.PDDC_EINVAL
    small = torch.empty((1, M), dtype=torch.complex64, device=dev)
    with pytest.raises(pkg.PddcError) as e:
        ch.process(d[6 * P * M:].data_ptr(), 4 * M, out=small)
    assert e.value.code == pkg.PDDC_ECAPACITY
    out = torch.empty((8, M), dtype=torch.complex64, device=dev)
    y = ch.process(d[6 * P * M:].data_ptr(), 4 * M, out=out)
    torch.cuda.synchronize()
    assert y.shape == (8, M) and y.data_ptr() == out.data_ptr()
    ref = CR.channelizer_ref(x[:(P + 4) * M], M, M // 2, w)
    assert ref.shape[0] == 9 and CR.err(y.cpu().numpy(), ref[1:]) <= TOL
    ch.close()


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("nchan", CR.SIZES)
def test_range(pkg, dev, lcg19, nchan, half):
    """A channel range gives the corresponding columns of the full-range output bit for bit (including a range that
    wraps and a single channel); set_range between batches takes effect at the next row and loses none."""
    import torch
    packed, _ = lcg19
    d = torch.from_numpy(packed).to(dev)
    M, hop = nchan, nchan // 2 if half else nchan
    w = pkg.channelizer_prototype(M, 4)
    full = run(pkg, d, M, hop, w)
    cols = lambda f, c: (f + torch.arange(c, device=dev)) % M
    for f, c in ((0, M), (M - 8, 16), (5, 1), (M // 2 - 100, 200)):
        y = run(pkg, d, M, hop, w, first=f, count=c)
        assert y.shape == (full.shape[0], c)
        assert torch.equal(bits(y), bits(full[:, cols(f, c)])), (f, c)
    ns = packed.size // 6
    cuts = [ns // 4 + 8, ns // 4 - 8, 8 * 5, ns // 2 - 8 * 5]
    rng = {1: (M - 8, 16), 2: (5, 1), 3: (M // 2 - 100, 200)}
    outs = run(pkg, d, M, hop, w, cuts=cuts, ranges=rng)
    row = 0
    for i, y in enumerate(outs):
        f, c = rng.get(i, (0, M))
        assert torch.equal(bits(y), bits(full[row:row + y.shape[0], cols(f, c)])), i
        row += y.shape[0]
    assert row == full.shape[0]


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("nchan", CR.SIZES)
def test_parity_in_the_walk(pkg, O, dev, tune, nchan, half):
    """2^24 LCG samples, P = 4 (M = 4096: the largest window), thousands of rows, several per block's run: every value
    against the double reference <= TOL; and the same stream with other run lengths (tunable chan_run: 1 row per block,
    7, and one block for everything up to 5000 rows) bit-identical."""
    import torch
    ns = 1 << 24
    d = synth(pkg, dev, ns)
    hop = nchan // 2 if half else nchan
    w = CR.random_prototype(nchan, 4)
    y = run(pkg, d, nchan, hop, w)
    x = R.to_complex(O, d.cpu().numpy())
    ref = CR.channelizer_ref(x, nchan, hop, w)
    e = CR.err(y.cpu().numpy(), ref)
    print(f"walk M {nchan} D {hop}: rows {y.shape[0]} err {e:.2e}")
    assert y.shape == ref.shape and y.shape[0] >= 4093 and e <= TOL
    del x, ref
    for r in (1, 7, 5000):
        tune("chan_run", r)
        y2 = run(pkg, d, nchan, hop, w)
        assert torch.equal(bits(y), bits(y2)), r


def test_repeatability(pkg, dev):
    """The same batches after reset(), 20 times, and on a fresh object: identical bits."""
    import torch
    ns = 1 << 22
    d = synth(pkg, dev, ns, 777)
    cuts = [ns - 40 * 4096 - 8 * 5, 8 * 5, 4096 * 39, 4096]
    assert sum(cuts) == ns

    def once(ch):
        off, outs = 0, []
        for b in cuts:
            outs.append(ch.process(d[6 * off:].data_ptr(), b))
            off += b
        torch.cuda.synchronize()
        return torch.cat(outs, dim=0)

    for M, hop, P in ((4096, 2048, 4), (1024, 1024, 8)):
        w = pkg.channelizer_prototype(M, P)
        ch = pkg.Channelizer(M, w, hop)
        y0 = once(ch)
        assert y0.shape[0] == (ns - P * M) // hop + 1
        for _ in range(20):
            ch.reset()
            assert torch.equal(bits(once(ch)), bits(y0))
        ch.close()
        fresh = pkg.Channelizer(M, w, hop)
        assert torch.equal(bits(once(fresh)), bits(y0))
        fresh.close()


def ref_rows_in_chunks(O, d, ns, M, hop, w, cols, rows_per_chunk=2048):
    """the reference of a long device stream, row chunk by row chunk with the L - D overlap, columns `cols`"""
    L = w.size
    nrows = CR.nrows_of(ns, L, hop)
    out = np.empty((nrows, len(cols)), np.complex128)
    for a in range(0, nrows, rows_per_chunk):
        b = min(a + rows_per_chunk, nrows)
        lo, hi = a * hop, (b - 1) * hop + L
        x = R.to_complex(O, d[6 * lo:6 * hi].cpu().numpy())
        out[a:b] = CR.channelizer_ref(x, M, hop, w, row0=a)[:, cols]
    return out


def test_full_size(pkg, O, dev):
    """One 2^28-sample batch, M = 4096, D = M, P = 4, a range of 256 channels (the full matrix would be 2 GiB to compare
    on the host): 65 533 rows, every value against the reference computed in chunks with their L - D overlap; plus the
    full range on 2^26 samples.  <= TOL."""
    import torch
    M, P = 4096, 4
    w = pkg.channelizer_prototype(M, P)
    ns = 1 << 28
    d = synth(pkg, dev, ns)
    first, count = 4000, 256
    y = run(pkg, d, M, M, w, first=first, count=count)
    t0 = time.time()
    cols = (first + np.arange(count)) % M
    ref = ref_rows_in_chunks(O, d, ns, M, M, w, cols)
    e1 = CR.err(y.cpu().numpy(), ref)
    print(f"full size 2^28, {count} channels: rows {y.shape[0]} err {e1:.2e}, reference took {time.time() - t0:.0f} s")
    assert y.shape == ref.shape == (65533, count) and e1 <= TOL
    del y, ref
    ns = 1 << 26
    y = run(pkg, d[:6 * ns], M, M, w)
    ref = ref_rows_in_chunks(O, d, ns, M, M, w, np.arange(M))
    scale = np.max(np.abs(ref))
    e2 = 0.0
    for a in range(0, ref.shape[0], 2048):
        e2 = max(e2, float(np.max(np.abs(y[a:a + 2048].cpu().numpy().astype(np.complex128) - ref[a:a + 2048])) / scale))
    print(f"full size 2^26, all channels: rows {y.shape[0]} err {e2:.2e}")
    assert tuple(y.shape) == ref.shape == (16381, M) and e2 <= TOL


def test_bank_panorama_and_channelizer_on_one_batch(pkg, dev, taps):
    """One d_packed and one stream: a Bank of four 48-tap members, a Spectrum and a Channelizer -- each bit-identical
    to its run alone."""
    import torch
    ns = 1 << 22
    d = synth(pkg, dev, ns, 4242)
    st = torch.cuda.current_stream().cuda_stream
    t48 = taps("d8_127")[:48].copy()
    fregs = [0x12345678, 0x3456789A, 0x9ABCDEF0, 0xDEADBEEF]
    w = pkg.channelizer_prototype(2048, 4)

    def rounds(with_bank, with_spec, with_chan):
        pipes = [pkg.Pipeline([(8, t48)], device=0, mix=True) for _ in fregs]
        for p, f in zip(pipes, fregs):
            p.set_freg(f)
        bank = pkg.Bank(pipes)
        sp = pkg.Spectrum(4096, 2048, None, peak=True) if with_spec else None
        ch = pkg.Channelizer(2048, w, 1024) if with_chan else None
        outs = [torch.zeros((ns // 8 + 16, 2), dtype=torch.float32, device=dev) for _ in fregs]
        res, rows = [], []
        for rnd in range(2):
            if with_bank:
                n, nb = bank.process_ptr(d.data_ptr(), ns, [o.data_ptr() for o in outs], [o.shape[0] for o in outs], st)
                assert nb == 4
                res += [o[:k].clone() for o, k in zip(outs, n)]
            if sp:
                sp.process(d)
            if ch:
                rows.append(ch.process(d))
        spec = sp.read() if sp else None
        torch.cuda.synchronize()
        bank.close()
        for p in pipes:
            p.close()
        if sp:
            sp.close()
        if ch:
            ch.close()
        return res, spec, rows

    all_b, all_s, all_c = rounds(True, True, True)
    alone_b, _, _ = rounds(True, False, False)
    _, alone_s, _ = rounds(False, True, False)
    _, _, alone_c = rounds(False, False, True)
    assert len(all_b) == len(alone_b) == 8
    for a, b in zip(all_b, alone_b):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert all_s[2] == alone_s[2] > 0
    assert torch.equal(all_s[0].view(torch.int32), alone_s[0].view(torch.int32))
    assert torch.equal(all_s[1].view(torch.int32), alone_s[1].view(torch.int32))
    assert len(all_c) == len(alone_c) == 2 and all_c[0].shape[0] > 4000
    for a, b in zip(all_c, alone_c):
        assert torch.equal(bits(a), bits(b))


@pytest.mark.perf
@pytest.mark.parametrize("lg", [24, 28])
def test_channelizer_time_against_the_host_path(pkg, dev, perf_record, lg):
    """k_channelize against what a host had before it: pddc_unpack24_f32 into a float buffer, overlapping frames
    (as_strided) times w, the sum over the P taps of a branch, torch.fft.fft -- same box, same process, D = M, P = 4,
    full range, median of 15 by events after a 1 s settle.  The kernel must be faster at every point.  Recorded without
    an assertion: pddc_unpack24_f32 alone on the same bytes (6 B read + 8 B written per sample: the same traffic),
    Spectrum.process with N = M (the same loads and transform, no stores), D = M/2, and a range of 256 channels."""
    import torch
    ns = 1 << lg
    d = synth(pkg, dev, ns)

    def timed(fn, reps=15):
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    for M in (1024, 4096):
        P = 4
        L = P * M
        wn = pkg.channelizer_prototype(M, P)
        w = torch.from_numpy(wn).to(dev)
        rows = (ns - L) // M + 1
        # (a repeated batch continues the stream: from the second on it completes L/D - 1 more rows than the first)
        out = torch.empty((rows + 8, M), dtype=torch.complex64, device=dev)
        out2 = torch.empty((2 * rows + 16, M), dtype=torch.complex64, device=dev)
        ch = pkg.Channelizer(M, wn, M)
        chr_ = pkg.Channelizer(M, wn, M, first=M // 2 - 128, count=256)
        chh = pkg.Channelizer(M, wn, M // 2)
        sp = pkg.Spectrum(M, M, None)

        def host_path():
            x = torch.view_as_complex(pkg.unpack24_f32(d))
            fr = x.as_strided((rows, L), (M, 1))
            u = (fr * w).view(rows, P, M).sum(dim=1)
            return torch.fft.fft(u, dim=1)

        def new(c, o):
            c.process(d, out=o)

        host_path()
        new(ch, out)
        torch.cuda.synchronize()
        time.sleep(1.0)                      # freshly allocated buffers are slow at first
        t_host = timed(host_path)
        t_new = timed(lambda: new(ch, out))
        t_rng = timed(lambda: new(chr_, out))
        t_half = timed(lambda: new(chh, out2))
        t_unp = timed(lambda: pkg.unpack24_f32(d))
        t_spec = timed(lambda: sp.process(d))
        for c in (ch, chr_, chh, sp):
            c.close()
        del out, out2
        torch.cuda.empty_cache()
        perf_record(f"channelizer_2p{lg}_m{M}_ms", round(t_new, 4), unit="ms", host_path_ms=round(t_host, 4),
                    ratio=round(t_host / t_new, 2), range256_ms=round(t_rng, 4),
                    half_hop_ms=round(t_half, 4), unpack24_ms=round(t_unp, 4),
                    spectrum_ms=round(t_spec, 4))
        assert t_new < t_host, (lg, M, t_new, t_host)
