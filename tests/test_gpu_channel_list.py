"""The channel list on the GPU: Channelizer.set_channels writes rows of the listed channels only, Tuner.set_channels reads
them in place (include/perseus_ddc.h).  The yardstick is the range mode of the same objects, bit for bit -- a value's bits
may not depend on the list, its order, the mode, the batch cut or the run length -- and tests/channelizer_ref.py for
parity.  Input: the on-device LCG stream.  The channelizer cases take 2^15 samples at M = 1024 (2^16 at 2048, 2^17 at
4096): about 57 rows at P = 4 and hop M/2.  The tuner cases take four times that (249 rows): with fewer rows than T = 64
there would be no output to compare."""
import ctypes as C

import numpy as np
import pytest

import channelizer_ref as CR
import spectrum_ref as R
import tuner_ref as TR

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00001


def synth(pkg, dev, ns, seed=12345):
    import torch
    d = torch.empty(6 * ns, dtype=torch.uint8, device=dev)
    pkg.check(pkg.ddc_lib().pddc_synth_lcg(d.data_ptr(), 6 * ns, seed, 0, torch.cuda.current_stream().cuda_stream))
    return d


def bits(t):
    import torch
    return torch.view_as_real(t.contiguous()).contiguous().view(torch.int32)


def nsamples_of(M):
    return {1024: 1 << 15, 2048: 1 << 16, 4096: 1 << 17}[M]


def lists_of(M, seed):
    rng = np.random.default_rng(seed)
    return [[M - 1], [int(v) for v in rng.permutation(M)[:7]], [int(v) for v in rng.permutation(M)[:1024]]]


def columns(full, channels, dev):
    import torch
    return full[:, torch.tensor(list(channels), dtype=torch.long, device=dev)]


def full_range(pkg, d, M, hop, w):
    import torch
    ch = pkg.Channelizer(M, w, hop)
    y = ch.process(d)
    torch.cuda.synchronize()
    ch.close()
    return y


@pytest.mark.parametrize("M,P,hop", [(1024, 1, 1024), (1024, 4, 512), (2048, 2, 2048), (4096, 4, 2048), (1024, 8, 512)])
def test_same_bits_as_range_mode(pkg, dev, M, P, hop):
    """list_out == full_out[:, channels], bit for bit, for n = 1 (channel M - 1), n = 7 and n = 1024, random and unsorted
    (M = 1024: a permutation of all channels).  (4096, 4, 2048) is the instance at the LDS limit (159 616 B): it must
    launch."""
    import torch
    d = synth(pkg, dev, nsamples_of(M))
    w = pkg.tuner_prototype(M, P)
    full = full_range(pkg, d, M, hop, w)
    assert full.shape == (CR.nrows_of(nsamples_of(M), P * M, hop), M) and full.shape[0] > 20
    for channels in lists_of(M, 100 + M + P):
        ch = pkg.Channelizer(M, w, hop)
        ch.set_channels(channels)
        assert ch.count == len(channels) and list(ch.channels) == channels
        assert ch.next_rows(nsamples_of(M)) == full.shape[0]
        y = ch.process(d)
        torch.cuda.synchronize()
        assert y.shape == (full.shape[0], len(channels))
        assert torch.equal(bits(y), bits(columns(full, channels, dev))), (M, P, hop, len(channels))
        ch.close()


@pytest.mark.parametrize("M,P,hop,n", [(1024, 4, 512, 7), (4096, 4, 2048, 1024), (2048, 2, 2048, 1)])
def test_nothing_else_is_written(pkg, dev, M, P, hop, n):
    """64 guard values behind rows * n, prefilled with a NaN pattern, are intact; a capacity one row short is
    PDDC_ECAPACITY with nothing written and no state moved: the next call gives the same rows."""
    import torch
    ns = nsamples_of(M)
    d = synth(pkg, dev, ns)
    w = pkg.tuner_prototype(M, P)
    channels = [int(v) for v in np.random.default_rng(n + M).permutation(M)[:n]]
    full = full_range(pkg, d, M, hop, w)
    rows = full.shape[0]
    ch = pkg.Channelizer(M, w, hop)
    ch.set_channels(channels)
    buf = torch.full((rows * n + 64,), NAN_BITS, dtype=torch.int32, device=dev).repeat_interleave(2).view(torch.float32)
    assert buf.numel() == 2 * (rows * n + 64)
    nr = C.c_size_t(99)
    st = torch.cuda.current_stream().cuda_stream
    rc = pkg.ddc_lib().pddc_channelizer_process(ch._h, d.data_ptr(), ns, buf.data_ptr(), rows - 1, C.byref(nr), st)
    torch.cuda.synchronize()
    assert rc == pkg.PDDC_ECAPACITY
    assert bool((buf.view(torch.int32) == NAN_BITS).all())
    assert ch.next_rows(ns) == rows
    rc = pkg.ddc_lib().pddc_channelizer_process(ch._h, d.data_ptr(), ns, buf.data_ptr(), rows, C.byref(nr), st)
    torch.cuda.synchronize()
    assert rc == 0 and nr.value == rows
    got = torch.view_as_complex(buf.view(-1, 2))
    assert torch.equal(bits(got[:rows * n].view(rows, n)), bits(columns(full, channels, dev)))
    assert bool((buf.view(torch.int32)[2 * rows * n:] == NAN_BITS).all())
    ch.close()


@pytest.mark.parametrize("chan_run", [1, 7, 0])
def test_cuts_runs_and_mode_changes(pkg, dev, tune, chan_run):
    """One stream in ragged batches (multiples of 8; the first gives one row, the third is shorter than L and gives
    none), the list changed before each, then range mode, then a list again -- all calls back to back on one stream,
    no synchronisation in between.  Every batch equals the matching rows and columns of an uncut full-range run."""
    import torch
    M, P, hop = 1024, 4, 512
    ns = nsamples_of(M)
    d = synth(pkg, dev, ns)
    w = pkg.tuner_prototype(M, P)
    full = full_range(pkg, d, M, hop, w)
    rng = np.random.default_rng(77)
    la, lb, lc, ld = ([int(v) for v in rng.permutation(M)[:n]] for n in (7, 1024, 3, 33))
    cuts = [P * M + 24, 8000, 40, 5608, 7200]
    cuts.append(ns - sum(cuts))
    modes = [("list", la), ("list", lb), ("list", lc), ("range", (1000, 100)), ("list", ld), (None, None)]
    assert all(c % 8 == 0 and c > 0 for c in cuts) and cuts[2] < P * M
    tune("chan_run", chan_run)
    ch = pkg.Channelizer(M, w, hop)
    outs, cols, off = [], [], 0
    cur = list(range(M))
    for b, (mode, arg) in zip(cuts, modes):
        if mode == "list":
            ch.set_channels(arg)
            cur = arg
        elif mode == "range":
            ch.set_range(*arg)
            assert ch.channels is None
            cur = [(arg[0] + i) % M for i in range(arg[1])]
        want = ch.next_rows(b)
        y = ch.process(d[6 * off:6 * (off + b)].data_ptr(), b)
        assert y.shape == (want, len(cur))
        outs.append(y)
        cols.append(cur)
        off += b
    torch.cuda.synchronize()
    ch.close()
    counts = [y.shape[0] for y in outs]
    assert counts[0] == 1 and counts[2] == 0 and sum(counts) == full.shape[0]          # the rows go on without a gap
    row = 0
    for i, (y, c) in enumerate(zip(outs, cols)):
        assert torch.equal(bits(y), bits(columns(full[row:row + y.shape[0]], c, dev))), (chan_run, i)
        row += y.shape[0]


@pytest.mark.parametrize("M", [1024, 4096])
def test_parity_on_the_listed_columns(pkg, O, dev, M):
    """list mode against the double reference on the listed columns, within channelizer_ref.TOL (the error is taken
    relative to the largest reference value among the LISTED columns: no wider than the range mode's bar)."""
    import torch
    P, hop = 4, M // 2
    d = synth(pkg, dev, nsamples_of(M))
    x = R.to_complex(O, d.cpu().numpy())
    w = pkg.channelizer_prototype(M, P)
    channels = [int(v) for v in np.random.default_rng(M).permutation(M)[:1024]]
    ch = pkg.Channelizer(M, w, hop)
    ch.set_channels(channels)
    y = ch.process(d)
    torch.cuda.synchronize()
    ch.close()
    ref = CR.channelizer_ref(x, M, hop, w)[:, channels]
    e = CR.err(y.cpu().numpy(), ref)
    print(f"list parity M {M}: rows {y.shape[0]} err {e:.2e}")
    assert y.shape == ref.shape and e <= CR.TOL


@pytest.mark.parametrize("listed", [False, True])
def test_refused_lists_change_nothing(pkg, dev, listed):
    """a duplicate entry, an entry = M, n = 0 and n = 1025: PDDC_EINVAL, and the next process() is what it would have been"""
    import torch
    M, P, hop = 1024, 4, 512
    d = synth(pkg, dev, nsamples_of(M))
    w = pkg.tuner_prototype(M, P)
    full = full_range(pkg, d, M, hop, w)
    good = [5, 1023, 0, 77, 512, 300, 301]
    ch = pkg.Channelizer(M, w, hop, 900, 200)
    if listed:
        ch.set_channels(good)
    for bad in ([3, 9, 3], [1, M], [-1], [], list(range(1025)), list(range(1023)) + [5, 5]):
        with pytest.raises(pkg.PddcError) as e:
            ch.set_channels(bad)
        assert e.value.code == pkg.PDDC_EINVAL
    assert pkg.ddc_lib().pddc_channelizer_set_channels(ch._h, None, 3) == pkg.PDDC_EINVAL
    cols = good if listed else [(900 + i) % M for i in range(200)]
    assert ch.count == len(cols) and (list(ch.channels) == good if listed else ch.channels is None)
    y = ch.process(d)
    torch.cuda.synchronize()
    assert torch.equal(bits(y), bits(columns(full, cols, dev)))
    ch.close()


def tuner_words(M, K):
    b = M.bit_length() - 1
    if K == 1:
        return [TR.receiver_set(M, 40)[30]]
    if K == 7:                                      # receivers 2 and 5 share channel 300, off centre on either side
        return [(300 << (32 - b)) + 999, 0x12345678, (300 << (32 - b)) - 4000, TR.MASK - 5, (M - 1) << (32 - b),
                (300 << (32 - b)) + 999, 0x9ABCDEF0]
    return TR.receiver_set(M, K)


def tune_in_batches(pkg, ch, rows, words, h, decim, cuts):
    import torch
    t = pkg.Tuner(ch, words, h, decim)
    outs, off = [], 0
    for b in cuts:
        want = t.next_outputs(b)
        o = t.process(rows[off:off + b])
        assert o.shape == (len(words), want)
        outs.append(o)
        off += b
    assert off == rows.shape[0]
    torch.cuda.synchronize()
    t.close()
    return torch.cat(outs, dim=1)


@pytest.mark.parametrize("T,decim", [(64, 4), (3, 64)])
@pytest.mark.parametrize("M", [1024, 4096])
def test_tuner_in_list_mode_gives_range_mode_bits(pkg, dev, M, T, decim):
    """Channelizer(list) -> Tuner(list), the list from tuner_channel_list and the same list reversed, in ragged row
    batches (0 and 1 row among them), against Channelizer(full) -> Tuner(full) in one batch: the same bits.  K = 1,
    K = 7 with two receivers on one channel, K = 1024."""
    import torch
    hop, P = M // 2, 4
    ns = 4 * nsamples_of(M)
    d = synth(pkg, dev, ns)
    w, h = pkg.tuner_prototype(M, P), TR.random_lowpass(T)
    chf = pkg.Channelizer(M, w, hop)
    rows_full = chf.process(d)
    S = rows_full.shape[0]
    assert TR.noutputs_of(S, T, decim) >= 3
    cuts = [0, 1, decim - 1, T, 0, 7, 1, 2 * T + 1]
    cuts.append(S - sum(cuts))
    assert cuts[-1] > 0
    for K in (1, 7, 1024):
        words = tuner_words(M, K)
        want = tune_in_batches(pkg, chf, rows_full, words, h, decim, [S])
        assert want.shape == (K, TR.noutputs_of(S, T, decim))
        chans = pkg.tuner_channel_list(M, words)
        assert chans.size == len({TR.channel_of(M, f)[0] for f in words}) <= K
        for order in (chans, chans[::-1]):
            chl = pkg.Channelizer(M, w, hop)
            chl.set_channels(order)
            rows = chl.process(d)
            assert rows.shape == (S, chans.size)
            got = tune_in_batches(pkg, chl, rows, words, h, decim, cuts)
            assert torch.equal(bits(got), bits(want)), (M, T, decim, K)
            chl.close()
    chf.close()


def test_retune_across_a_list_change(pkg, dev):
    """Between two batches: the union list on both objects, set_freq, the shrunk list on both -- against the range-mode
    chain retuned at the same row, bit for bit.  Before that, set_freq to the unlisted channel and a list that misses a
    receiver's channel are refused (PDDC_EINVAL) and leave no trace in the outputs."""
    import torch
    M, P, hop, T, decim = 1024, 4, 512, 64, 4
    ns = 4 * nsamples_of(M)
    d = synth(pkg, dev, ns)
    w, h = pkg.tuner_prototype(M, P), pkg.tuner_lowpass(T, decim)
    words = [(10 << 22) + 5000, (11 << 22) - 77, (500 << 22) + (1 << 21) - 1, (500 << 22) - 123456, (1023 << 22) + 9]
    new1 = (700 << 22) - 31337                      # receiver 1 moves from channel 11 to 700
    cut = 8 * 9000
    parts = (d[:6 * cut], d[6 * cut:])

    chf = pkg.Channelizer(M, w, hop)
    tf = pkg.Tuner(chf, words, h, decim)
    a = tf.process(chf.process(parts[0]))
    tf.set_freq(1, new1)
    b = tf.process(chf.process(parts[1]))
    torch.cuda.synchronize()
    want = torch.cat([a, b], dim=1)
    tf.close()
    chf.close()
    assert a.shape[1] > 10 and b.shape[1] > 10

    l0 = pkg.tuner_channel_list(M, words)
    assert l0.tolist() == [10, 11, 500, 1023]
    chl = pkg.Channelizer(M, w, hop)
    chl.set_channels(l0)
    tl = pkg.Tuner(chl, words, h, decim)
    assert tl.count == 4 and tl.channels.tolist() == l0.tolist()
    a = tl.process(chl.process(parts[0]))
    with pytest.raises(pkg.PddcError) as e:
        tl.set_freq(1, new1)                         # channel 700 is not listed
    assert e.value.code == pkg.PDDC_EINVAL
    with pytest.raises(pkg.PddcError) as e:
        tl.set_channels([10, 500, 1023, 700])        # receiver 1 still sits on channel 11
    assert e.value.code == pkg.PDDC_EINVAL and tl.channels.tolist() == l0.tolist()
    union = l0.tolist() + [700]
    chl.set_channels(union)
    tl.set_channels(union)
    tl.set_freq(1, new1)
    shrunk = pkg.tuner_channel_list(M, [words[0], new1] + words[2:])
    assert shrunk.tolist() == [10, 500, 700, 1023]
    chl.set_channels(shrunk)
    tl.set_channels(shrunk)
    rows = chl.process(parts[1])
    assert rows.shape[1] == 4
    b = tl.process(rows)
    torch.cuda.synchronize()
    got = torch.cat([a, b], dim=1)
    assert got.shape == want.shape and torch.equal(bits(got), bits(want))
    # back to range mode on both: the stream goes on
    chl.set_range(0, M)
    tl.set_range(0, M)
    assert tl.channels is None and chl.process(parts[0][:6 * 8 * hop]).shape[1] == M
    tl.close()
    chl.close()
