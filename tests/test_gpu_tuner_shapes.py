"""k_tune / k_tune_carry in every regime of their control flow, against the numpy reference in double (tests/tuner_ref.py):
both group sizes, runs of several tiles with a move of 0, 1 and up to 4088 values between tiles, the full 64 KiB of LDS in
the 32-receiver form, a channel range that wraps through channel 0 with many receivers per column, and phase words
after s D passed 2^31 and 2^32.  Whether a case is in its regime is read from Tuner.schedule (the numbers process()
launches from), never restated here.  Tolerance: tuner_ref.TOL_TUNER_SHAPES, 7 x the float32 model's worst case on these
inputs (tests/test_tuner_cpu.py::test_float32_model_on_the_shape_cases), never taken from k_tune."""
import types

import numpy as np
import pytest

import tuner_ref as TR

pytestmark = pytest.mark.gpu

M, HOP, FIRST, COUNT, S = TR.SHAPES_GRID


def grid(nchan, hop, first=0, count=None):
    """what Tuner reads of a Channelizer, for tests that feed it rows of their own"""
    return types.SimpleNamespace(nchan=nchan, hop=hop, device=0, first=first, count=nchan if count is None else count)


def bits(t):
    import torch
    return torch.view_as_real(t.contiguous()).contiguous().view(torch.int32)


def same_bits(a, b):
    import torch
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def play(pkg, g, words, h, decim, batches, before=None, rows_before=0):
    """a fresh Tuner fed the batches (tensors [n, count]) in order -> complex64 [K, outputs].  before: {batch index:
    function of the tuner}, called before that batch.  next_outputs and the shape of every batch are checked against
    the window arithmetic."""
    import torch
    t = pkg.Tuner(g, words, h, decim)
    outs, off = [], rows_before
    for i, b in enumerate(batches):
        if before and i in before:
            before[i](t)
        n = b.shape[0]
        want = TR.noutputs_of(off + n, h.size, decim) - TR.noutputs_of(off, h.size, decim)
        assert t.next_outputs(n) == want, (i, off, n)
        o = t.process(b)
        assert o.shape == (len(words), want), (i, off, n)
        outs.append(o)
        off += n
    torch.cuda.synchronize()
    t.close()
    return torch.cat(outs, dim=1)


def split(rows, cuts):
    """rows cut into batches of the given lengths, then the rest"""
    out, off = [], 0
    for c in cuts:
        out.append(rows[off:off + c])
        off += c
    assert off <= rows.shape[0], "the cuts are longer than the rows: pick new shapes or more rows"
    out.append(rows[off:])
    return out


def schedule_of(pkg, g, words, h, decim, nrows):
    t = pkg.Tuner(g, words, h, decim)
    sch = t.schedule(nrows)
    t.close()
    return sch


@pytest.fixture(scope="module")
def rows64():
    return TR.gaussian_rows(S, COUNT)


@pytest.fixture(scope="module")
def words():
    return TR.receiver_set_in(M, FIRST, COUNT, 1024)


@pytest.fixture(scope="module")
def zref(rows64, words):
    """the double reference's z of all 1024 receivers, made once for every parity case and left unchanged"""
    res = [TR.channel_of(M, f)[1] for f in words]
    y = rows64[:, TR.columns_of(M, FIRST, words)].astype(np.complex128)
    z = TR.mix(y, res, [0] * len(words), HOP)
    z.setflags(write=False)
    return z


def assert_regime(T, decim, sch, nout):
    """the case is where it is there for; if the run rule or the tile rule ever changes, choose new shapes"""
    why = f"(T, R) = ({T}, {decim}) left its regime, schedule {sch}: choose new shapes or rows for this case"
    assert sch["group"] == (32 if T <= 128 else 8), why
    assert sch["run"] % sch["tile"] == 0 and sch["run"] >= 2 * sch["tile"] and nout > sch["tile"], why
    if (T, decim) in ((128, 64), (64, 64)):
        assert sch["tile"] < 8 and sch["tile"] * decim - decim + T == 256, why          # 256 rows x 32 x 8 B = 64 KiB
    if (T, decim) in ((128, 1), (512, 1)):
        assert (T - decim) * sch["group"] >= 4064, why


@pytest.mark.parametrize("T,decim", TR.CASES_TR_SHAPES)
def test_parity_in_every_tile_regime(pkg, dev, rows64, words, zref, T, decim):
    """8300 seeded Gaussian rows of the 64 channels from 1004 on (the range wraps through channel 0, column 20), hop
    512; the 1024 receivers of receiver_set_in (9 .. 24 on each column), then the first 33 and the first 9 (one past a
    block of 32 and of 8); Kaiser and random h; one batch: max |out - ref| / max |ref| <= TOL_TUNER_SHAPES = 1.10e-5
    (7 x the float32 model's worst case on these inputs, 1.574e-6).  Before the run Tuner.schedule must say that the
    case is in its regime: group 32 up to T = 128 and 8 above, a run of at least two tiles with more than a tile of
    outputs, for (128, 64) and (64, 64) tiles of 256 rows (the full 64 KiB), for (128, 1) and (512, 1) a move of at
    least 4064 values.  Every case prints its schedule and its error (lines that start with `shapes:`)."""
    import torch
    rows = torch.from_numpy(rows64).to(dev)
    g = grid(M, HOP, FIRST, COUNT)
    nout = TR.noutputs_of(S, T, decim)
    for name, h in (("kaiser", pkg.tuner_lowpass(T, decim)), ("random", TR.random_lowpass(T))):
        ref = TR.fir_decim_mm(zref, h, decim).T
        assert ref.shape == (1024, nout)
        for K in (1024, 33, 9):
            sch = schedule_of(pkg, g, words[:K], h, decim, S)
            if K == 1024:
                assert_regime(T, decim, sch, nout)
            out = play(pkg, g, words[:K], h, decim, [rows])
            e = TR.err(out.cpu().numpy(), ref[:K])
            print(f"shapes: parity T {T} R {decim} {name} K {K}: outputs {out.shape[1]} schedule {sch} err {e:.2e}")
            assert out.shape == ref[:K].shape
            assert e <= TR.TOL_TUNER_SHAPES, (T, decim, name, K, e)


@pytest.mark.parametrize("T,decim", TR.CASES_TR_SHAPES)
def test_bits_do_not_depend_on_cut_company_or_range(pkg, dev, rows64, words, T, decim):
    """The one-batch result of 1024 receivers (random h) against, bit for bit: ragged batches of 0, 1, R - 1, T,
    tile R - 1, tile R, tile R + 1, run R + 3 rows and the rest (tile and run from Tuner.schedule); receivers 0, 31, 32,
    511 and 1023 alone and seven together; the reversed receiver order; the same words behind the full range (the rows
    scattered into a zero [S, 1024] matrix); a set_range from the full range to the wrapped 64 between two batches (a
    refused set_range that leaves a receiver out before and after it changes nothing); and list mode from the second
    batch on, the 64 channels listed in descending order and the columns permuted to match."""
    import torch
    rows = torch.from_numpy(rows64).to(dev)
    g = grid(M, HOP, FIRST, COUNT)
    h = TR.random_lowpass(T)
    sch = schedule_of(pkg, g, words, h, decim, S)
    assert_regime(T, decim, sch, TR.noutputs_of(S, T, decim))
    tile, run = sch["tile"], sch["run"]
    one = play(pkg, g, words, h, decim, [rows])
    assert one.shape == (1024, TR.noutputs_of(S, T, decim))
    assert words[15] == words[16] and same_bits(one[15], one[16])

    cuts = [0, 1, decim - 1, T, tile * decim - 1, tile * decim, tile * decim + 1, run * decim + 3]
    assert same_bits(play(pkg, g, words, h, decim, split(rows, cuts)), one)

    for j in (0, 31, 32, 511, 1023):
        assert same_bits(play(pkg, g, words[j:j + 1], h, decim, split(rows, cuts[::-1]))[0], one[j]), j
    seven = [0, 31, 32, 511, 1023, 5, 640]
    assert same_bits(play(pkg, g, [words[j] for j in seven], h, decim, [rows]), one[seven])
    assert same_bits(play(pkg, g, words[::-1], h, decim, [rows]), one.flip(0))

    full = torch.zeros((S, M), dtype=torch.complex64, device=dev)
    full[:, [(FIRST + i) % M for i in range(COUNT)]] = rows
    gf = grid(M, HOP)
    assert same_bits(play(pkg, gf, words, h, decim, [full]), one)

    cut = tile * decim + 7
    outside = (FIRST + 1) % M                        # leaves the receivers of channel 1004 out

    def narrow(t):
        with pytest.raises(pkg.PddcError) as e:
            t.set_range(outside, COUNT)
        assert e.value.code == pkg.PDDC_EINVAL and (t.first, t.count) == (0, M)
        t.set_range(FIRST, COUNT)
        with pytest.raises(pkg.PddcError) as e:
            t.set_range(outside, COUNT)
        assert e.value.code == pkg.PDDC_EINVAL and (t.first, t.count) == (FIRST, COUNT)

    assert same_bits(play(pkg, gf, words, h, decim, [full[:cut], rows[cut:]], before={1: narrow}), one)

    listed = [(FIRST + COUNT - 1 - i) % M for i in range(COUNT)]
    flipped = rows[cut:].flip(1).contiguous()
    got = play(pkg, g, words, h, decim, [rows[:cut], flipped], before={1: lambda t: t.set_channels(listed)})
    assert same_bits(got, one)


@pytest.mark.parametrize("hop", [4096, 2048])
def test_phase_past_2_31_and_2_32(pkg, dev, hop):
    """M = 4096, the wrapped range 4094, 4095, 0, 1, 16 receivers of receiver_set_in, w + 4096 seeded Gaussian rows,
    w = 2^32 / hop the row at which s D wraps and v = w / 2 the row at which it passes 2^31; (T, R) in (64, 4), (128, 1),
    (512, 64).  (a) One batch, Kaiser and random h: the outputs whose windows lie in the 4096 rows from v - 2048 and
    from w - 2048 against tuner_ref_range(row0) in double <= TOL_TUNER_SHAPES.  (b) Batches cut at w - 1, w, w + 1 and
    at v - 1, v, v + 1 give the one batch's bits over the whole stream, every batch with the exact output count.
    (c) Retunes at s0 = v, w - 1, w, w + 1 (at w the host's (s0 D) mod 2^32 is 0), each to another channel of the range,
    receiver 0 at all four: the device against TunerRef(row0) started with the phi that the rule
    phi' = phi + (F - F') (s0 D) mod 2^32 gives in exact integers, every segment behind a retune <= TOL_TUNER_SHAPES;
    the receivers that were not retuned keep the bits of the run without retunes."""
    import torch
    Mc, first, count = TR.DEEP_GRID
    w = (1 << 32) // hop
    v = w // 2
    Sd, win = w + 4096, 4096
    rows64 = TR.gaussian_rows(Sd, count)
    rows = torch.from_numpy(rows64).to(dev)
    g = grid(Mc, hop, first, count)
    words = TR.receiver_set_in(Mc, first, count, 16)
    sh = 20
    chans = [(first + i) % Mc for i in range(count)]
    for T, decim in TR.CASES_DEEP:
        n_all, n_win = TR.noutputs_of(Sd, T, decim), TR.noutputs_of(win, T, decim)
        one = None
        for name, h in (("random", TR.random_lowpass(T)), ("kaiser", pkg.tuner_lowpass(T, decim))):
            one = play(pkg, g, words, h, decim, [rows])
            assert one.shape == (16, n_all)
            for row0 in (v - 2048, w - 2048):
                assert row0 % decim == 0
                ref = TR.tuner_ref_range(rows64[row0:row0 + win], Mc, hop, first, words, h, decim, row0=row0)
                got = one[:, row0 // decim:row0 // decim + n_win].cpu().numpy()
                e = TR.err(got, ref)
                print(f"shapes: deep hop {hop} T {T} R {decim} {name} rows {row0} ..: outputs {n_win} err {e:.2e}")
                assert got.shape == ref.shape and e <= TR.TOL_TUNER_SHAPES, (hop, T, decim, name, row0, e)
        # from here on h is the Kaiser low-pass and `one` its one-batch result
        for c in (w, v):
            assert same_bits(play(pkg, g, words, h, decim, split(rows, [c - 1, 1, 1])), one), (T, decim, c)

        # retunes: receiver 0 at every s0, receivers 1, 2, 3 once each; always to another channel of the range
        def other(f, step, r):
            k = TR.channel_of(Mc, f)[0]
            return ((chans[(chans.index(k) + step) % count] << sh) + r) & TR.MASK

        plan, cur = [], list(words)
        for i, (s0, j, r) in enumerate(((v, None, 12345), (w - 1, 1, -(1 << 19)), (w, 2, (1 << 19) - 1), (w + 1, 3, -1))):
            todo = [(0, other(cur[0], 1 + i % 3, (12345, -54321, 99, 5 - (1 << 19))[i]))]
            todo += [(j, other(cur[j], 2, r))] if j is not None else []
            for jj, f in todo:
                assert TR.channel_of(Mc, f)[0] != TR.channel_of(Mc, cur[jj])[0] and TR.channel_of(Mc, f)[0] in chans
                cur[jj] = f
            plan.append((s0, todo))
        batches = split(rows, [v, w - 1 - v, 1, 1])
        retune = lambda todo: (lambda t: [t.set_freq(jj, f) for jj, f in todo])
        dev_out = play(pkg, g, words, h, decim, batches, before={i + 1: retune(todo) for i, (_, todo) in enumerate(plan)})
        assert dev_out.shape == one.shape
        assert same_bits(dev_out[4:], one[4:])
        assert not same_bits(dev_out[:4], one[:4])
        for row0 in (v - 2048, w - 2048):
            # the words and phi in force at row0, by the rule in exact integers
            wds, phi = list(words), [0] * 16
            for s0, todo in plan:
                if s0 < row0:
                    for jj, f in todo:
                        phi[jj] = (phi[jj] + (wds[jj] - f) * ((s0 * hop) % (1 << 32))) % (1 << 32)
                        wds[jj] = f
            ref = TR.TunerRef(Mc, hop, wds, h, decim, row0=row0, phi=phi)
            inside = [(s0, todo) for s0, todo in plan if row0 <= s0 < row0 + win]
            assert inside and (row0 < v or phi[0] != 0)
            outs, at = [], row0
            for s0, todo in inside + [(row0 + win, [])]:
                outs.append(ref.process(rows64[at:s0].astype(np.complex128), first))
                for jj, f in todo:
                    ref.set_freq(jj, f)
                at = s0
            want = np.concatenate(outs, axis=1)
            got = dev_out[:, row0 // decim:row0 // decim + n_win].cpu().numpy()
            assert got.shape == want.shape
            m = np.arange(n_win) * decim + row0
            for s0 in [row0] + [s for s, _ in inside]:
                seg = m >= s0
                if seg.any():
                    e = TR.err(got[:, seg], want[:, seg])
                    print(f"shapes: deep retunes hop {hop} T {T} R {decim} rows {row0} .. from {s0}: "
                          f"outputs {int(seg.sum())} err {e:.2e}")
                    assert e <= TR.TOL_TUNER_SHAPES, (hop, T, decim, row0, s0, e)
        del one, dev_out


@pytest.mark.parametrize("K", [1, 33, 1024])
def test_schedule_reports_what_process_launches(pkg, dev, rows64, words, K):
    """Tuner.schedule between the batches of a ragged run, (T, R) = (5, 4), (128, 1), (512, 63): blocks = ceil(outputs /
    run), run a multiple of the tile, group and tile those of the shape, carried = rows so far + nrows - R x outputs so
    far; with no outputs {group, tile, 0, 0, carried}; asking changes nothing: the run's bits are those of a run that
    never asked.  On a closed handle it is refused with PDDC_EINVAL."""
    import torch
    rows = torch.from_numpy(rows64).to(dev)
    g = grid(M, HOP, FIRST, COUNT)
    for T, decim in ((5, 4), (128, 1), (512, 63)):
        h = TR.random_lowpass(T)
        cuts = [3, 0, T, 1, 3000, decim - 1, 2000]
        batches = split(rows, cuts)
        quiet = play(pkg, g, words[:K], h, decim, batches)
        t = pkg.Tuner(g, words[:K], h, decim)
        outs, off, done = [], 0, 0
        for b in batches:
            n = b.shape[0]
            for _ in range(2):                       # asking twice gives the same answer
                sch = t.schedule(n)
            nout = t.next_outputs(n)
            assert sch["group"] == (32 if T <= 128 else 8) and sch["tile"] >= 1
            assert sch["carried"] == off + n - decim * (done + nout) and 0 <= sch["carried"] < T
            if nout:
                assert sch["run"] % sch["tile"] == 0 and sch["run"] > 0
                assert sch["blocks"] == -(-nout // sch["run"])
            else:
                assert (sch["run"], sch["blocks"]) == (0, 0)
            t.schedule(7 * n + 1)                    # another size: still nothing moves
            outs.append(t.process(b))
            off, done = off + n, done + nout
        torch.cuda.synchronize()
        print(f"shapes: schedule T {T} R {decim} K {K}: last batch {sch}")
        assert same_bits(torch.cat(outs, dim=1), quiet)
        t.close()
        with pytest.raises(pkg.PddcError) as e:
            t.schedule(100)
        assert e.value.code == pkg.PDDC_EINVAL
