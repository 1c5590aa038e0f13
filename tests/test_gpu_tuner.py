"""Tuner (pddc_tuner_*, Tuner) on the GPU against the numpy reference in double (tests/tuner_ref.py on
tests/channelizer_ref.py).  Tolerances: tuner_ref.TOL_TUNER / TOL_CHAIN, 7 x the float32 models' worst cases
(tests/test_tuner_cpu.py::test_float32_models_against_double), never taken from k_tune."""
import time
import types

import numpy as np
import pytest

import channelizer_ref as CR
import spectrum_ref as R
import tuner_ref as TR

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


def grid(M, hop, first=0, count=None):
    """what Tuner reads of a Channelizer, for the tests that feed it rows of their own"""
    return types.SimpleNamespace(nchan=M, hop=hop, device=0, first=first, count=M if count is None else count)


def run(pkg, rows, g, words, h, decim, cuts=None):
    """all of rows (torch complex64 [S, count]) through a fresh Tuner in the given batches -> complex64 [K, outputs]"""
    import torch
    t = pkg.Tuner(g, words, h, decim)
    outs, off = [], 0
    for b in cuts or [rows.shape[0]]:
        want = t.next_outputs(b)
        o = t.process(rows[off:off + b])
        assert o.shape == (len(words), want)
        outs.append(o)
        off += b
    assert off == rows.shape[0]
    torch.cuda.synchronize()
    t.close()
    return torch.cat(outs, dim=1)


def bits(t):
    import torch
    return torch.view_as_real(t.contiguous()).contiguous().view(torch.int32)


def random_rows(dev, nrows, count, seed=99):
    import torch
    gen = torch.Generator(device="cpu").manual_seed(seed)
    r = torch.randn((nrows, count, 2), generator=gen, dtype=torch.float32)
    return torch.view_as_complex(r).to(dev)


def lowpasses(pkg, T, decim):
    return (("kaiser", pkg.tuner_lowpass(T, decim)), ("random", TR.random_lowpass(T)))


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("nchan", [1024, 4096])
def test_parity_tuner_alone(pkg, dev, lcg19, nchan, half):
    """The double reference's rows rounded to complex64 and uploaded; K = 1024 receivers (every boundary residue on
    channels 0, 1, M/2, M - 1, the word that wraps to channel 0, two identical words, the rest seeded random), K = 1 and
    K = 7; (T, R) in (1, 1), (64, 4), (512, 64), Kaiser and random h: max |out - ref| / max |ref| <= TOL_TUNER = 5.92e-6
    (7 x the float32 model's worst case, 8.46e-7 at T = 512).  Cases whose T exceeds the rows of 2^19 samples give no
    output in the reference either and are skipped inside, as in the CPU measurement.
    k_tune measured 5.6e-8 .. 8.4e-7 here (profiles/r11/tuner_tests_figures.txt)."""
    import torch
    _, x = lcg19
    M, hop = nchan, nchan // 2 if half else nchan
    y64 = CR.channelizer_ref(x, M, hop, TR.kaiser_prototype_wide(M, 4)).astype(np.complex64)
    rows = torch.from_numpy(y64).to(dev)
    yd = y64.astype(np.complex128)
    words = TR.receiver_set(M, 1024)
    done = 0
    for T, decim in TR.CASES_TR:
        if TR.noutputs_of(y64.shape[0], T, decim) == 0:
            continue
        for name, h in lowpasses(pkg, T, decim):
            for K in (1024, 1, 7):
                wk = words[:K] if K > 1 else words[30:31]
                ref = TR.tuner_ref(yd, M, hop, wk, h, decim)
                out = run(pkg, rows, grid(M, hop), wk, h, decim)
                e = TR.err(out.cpu().numpy(), ref)
                print(f"M {M} D {hop} T {T} R {decim} {name} K {K}: outputs {out.shape[1]} err {e:.2e}")
                assert out.shape == ref.shape
                assert e <= TR.TOL_TUNER, (T, decim, name, K, e)
                done += 1
    assert done >= 12


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("nchan", [1024, 4096])
def test_parity_end_to_end(pkg, dev, lcg19, nchan, half):
    """packed bytes -> Channelizer -> Tuner on one stream against tuner_ref on channelizer_ref, all in double:
    <= TOL_CHAIN = 6.20e-6 (7 x the model chain's worst case, 8.86e-7)."""
    import torch
    packed, x = lcg19
    M, hop = nchan, nchan // 2 if half else nchan
    w = pkg.tuner_prototype(M, 4)
    d = torch.from_numpy(packed).to(dev)
    y = CR.channelizer_ref(x, M, hop, w)
    words = TR.receiver_set(M, 1024)
    for T, decim in TR.CASES_TR:
        if TR.noutputs_of(y.shape[0], T, decim) == 0:
            continue
        for name, h in lowpasses(pkg, T, decim):
            ch = pkg.Channelizer(M, w, hop)
            t = pkg.Tuner(ch, words, h, decim)
            out = t.process(ch.process(d))
            torch.cuda.synchronize()
            ref = TR.tuner_ref(y, M, hop, words, h, decim)
            e = TR.err(out.cpu().numpy(), ref)
            print(f"chain M {M} D {hop} T {T} R {decim} {name}: outputs {out.shape[1]} err {e:.2e}")
            assert out.shape == ref.shape and e <= TR.TOL_CHAIN, (T, decim, name, e)
            t.close()
            ch.close()


def ref_rows_in_chunks(O, d, ns, M, hop, w, cols, rows_per_chunk=2048):
    """the channelizer reference of a long device stream, row chunk by row chunk with the L - D overlap, columns `cols`"""
    L = w.size
    nrows = CR.nrows_of(ns, L, hop)
    out = np.empty((nrows, len(cols)), np.complex128)
    for a in range(0, nrows, rows_per_chunk):
        b = min(a + rows_per_chunk, nrows)
        x = R.to_complex(O, d[6 * a * hop:6 * ((b - 1) * hop + L)].cpu().numpy())
        out[a:b] = CR.channelizer_ref(x, M, hop, w, row0=a)[:, cols]
    return out


def test_end_to_end_full_size(pkg, O, dev):
    """2^26 LCG samples, M = 4096, hop 2048, K = 256, T = 64, R = 4, the stream in three batches: every output against
    the reference (computed for the 256 columns only) <= TOL_CHAIN."""
    import torch
    M, hop, T, decim, ns = 4096, 2048, 64, 4, 1 << 26
    w = pkg.tuner_prototype(M, 4)
    h = pkg.tuner_lowpass(T, decim)
    words = TR.receiver_set(M, 256)
    d = synth(pkg, dev, ns)
    ch = pkg.Channelizer(M, w, hop)
    t = pkg.Tuner(ch, words, h, decim)
    outs, off = [], 0
    for b in (ns // 2 + 8, 8 * 1000, ns // 2 - 8 - 8 * 1000):
        outs.append(t.process(ch.process(d[6 * off:6 * (off + b)])))
        off += b
    torch.cuda.synchronize()
    out = torch.cat(outs, dim=1).cpu().numpy()
    t0 = time.time()
    kr = [TR.channel_of(M, f) for f in words]
    ycols = ref_rows_in_chunks(O, d, ns, M, hop, w, np.array([k for k, _ in kr]))
    ref = TR.fir_decim(TR.mix(ycols, [r for _, r in kr], [0] * len(words), hop), h, decim).T
    e = TR.err(out, ref)
    print(f"full size 2^26, K 256: rows {ycols.shape[0]} outputs {out.shape[1]} err {e:.2e}, reference took {time.time() - t0:.0f} s")
    assert out.shape == ref.shape == (256, (ycols.shape[0] - T) // decim + 1) and e <= TR.TOL_CHAIN
    t.close()
    ch.close()


@pytest.mark.parametrize("T,decim", TR.CASES_TR + ((3, 64),))
def test_ragged_batches_and_company_give_the_same_bits(pkg, dev, T, decim):
    """6000 seeded rows of 1024 channels, hop 512.  Ragged row batches (0, 1, R - 1, T, a few thousand rows) equal one
    batch bit for bit; receiver j's series is bit-identical alone, among 1024, and at another index; the two identical
    words give identical bits."""
    import torch
    M, hop, S = 1024, 512, 6000
    rows = random_rows(dev, S, M)
    words = TR.receiver_set(M, 1024)
    h = TR.random_lowpass(T)
    one = run(pkg, rows, grid(M, hop), words, h, decim)
    assert one.shape[1] == TR.noutputs_of(S, T, decim) > 0
    cuts = [0, 1, decim - 1, T, 3000, 0, 7, 1, 2 * T + 1]
    cuts.append(S - sum(cuts))
    ragged = run(pkg, rows, grid(M, hop), words, h, decim, cuts=cuts)
    assert ragged.shape == one.shape and torch.equal(bits(ragged), bits(one))
    assert words[21] == words[22] and torch.equal(bits(one[21]), bits(one[22]))
    for j in (0, 4, 20, 22, 500, 1023):
        alone = run(pkg, rows, grid(M, hop), words[j:j + 1], h, decim, cuts=cuts[::-1])
        assert torch.equal(bits(alone[0]), bits(one[j])), j
    rev = run(pkg, rows, grid(M, hop), words[::-1], h, decim)
    assert torch.equal(bits(rev), bits(one.flip(0)))
    few = run(pkg, rows, grid(M, hop), words[100:107], h, decim)
    assert torch.equal(bits(few), bits(one[100:107]))


def test_a_narrowed_range_gives_the_same_bits(pkg, dev, lcg19):
    """Channelizer -> Tuner with 1024 receivers and the full range, against receiver j alone behind a channelizer whose
    range is narrowed to just cover it between two batches (set_range on both objects): no output lost, the same bits."""
    import torch
    packed, _ = lcg19
    M, hop, T, decim = 1024, 512, 64, 4
    d = torch.from_numpy(packed).to(dev)
    ns = packed.size // 6
    w, h = pkg.tuner_prototype(M, 4), pkg.tuner_lowpass(T, decim)
    words = TR.receiver_set(M, 1024)
    ch = pkg.Channelizer(M, w, hop)
    t = pkg.Tuner(ch, words, h, decim)
    full = t.process(ch.process(d))
    torch.cuda.synchronize()
    t.close()
    ch.close()
    cut = ns // 2 + 8 * 33
    for j in (3, 20, 700):
        k = TR.channel_of(M, words[j])[0]
        ch = pkg.Channelizer(M, w, hop)
        t = pkg.Tuner(ch, [words[j]], h, decim)
        a = t.process(ch.process(d[:6 * cut]))
        ch.set_range(k, 1)
        t.set_range(k, 1)
        rows = ch.process(d[6 * cut:])
        assert rows.shape[1] == 1
        b = t.process(rows)
        torch.cuda.synchronize()
        got = torch.cat([a, b], dim=1)
        assert got.shape == (1, full.shape[1]) and torch.equal(bits(got[0]), bits(full[j])), j
        with pytest.raises(pkg.PddcError) as e:             # a range that leaves the receiver out: refused, nothing changed
            t.set_range((k + 1) % M, 5)
        assert e.value.code == pkg.PDDC_EINVAL and (t.first, t.count) == (k, 1)
        t.close()
        ch.close()


def test_retune_and_refused_calls(pkg, dev):
    """Retunes between batches against the streaming reference with the rule phi' = phi + (F - F') s0 D (double, on the
    same complex64 rows) <= TOL_TUNER; a refused set_freq (channel outside the range) and refused process calls
    (out_stride too small, misaligned pointers) queue nothing and move nothing: the outputs equal those of a tuner that
    never saw them, bit for bit."""
    import torch
    M, hop, T, decim, S = 1024, 512, 64, 4, 3000
    first, count = 100, 50
    rows = random_rows(dev, S, count, seed=5)
    b = 22
    words = [((first + i) << b) + 1000 * i - 20000 for i in range(0, count, 3)]
    h = pkg.tuner_lowpass(T, decim)
    g = grid(M, hop, first, count)
    cuts = [1000, 1, 999, 1000]
    retunes = {1: [(0, ((first + 7) << b) + 5), (3, ((first + 49) << b) - (1 << 21))], 2: [(0, (first << b) - 1234)],
               3: [(5, ((first + 20) << b) + (1 << 21) - 1), (3, words[3])]}

    def play(disturb):
        t = pkg.Tuner(g, words, h, decim)
        outs, off = [], 0
        for i, n in enumerate(cuts):
            for j, f in retunes.get(i, ()):
                t.set_freq(j, f)
            if disturb:
                with pytest.raises(pkg.PddcError) as e:
                    t.set_freq(1, 500 << b)                  # channel 500 is outside 100 .. 149
                assert e.value.code == pkg.PDDC_EINVAL
                with pytest.raises(pkg.PddcError) as e:
                    t.set_freq(len(words), words[0])
                assert e.value.code == pkg.PDDC_EINVAL
                want = t.next_outputs(n)
                if want > 1:
                    small = torch.empty((len(words), want - 1), dtype=torch.complex64, device=dev)
                    with pytest.raises(pkg.PddcError) as e:
                        t.process(rows[off:off + n], out=small)
                    assert e.value.code == pkg.PDDC_ECAPACITY
                with pytest.raises(pkg.PddcError) as e:
                    t.process(rows[off:off + n].data_ptr() + 4, nrows=n)
                assert e.value.code == pkg.PDDC_EINVAL
                assert t.next_outputs(n) == want
            outs.append(t.process(rows[off:off + n]))
            off += n
        torch.cuda.synchronize()
        t.close()
        return torch.cat(outs, dim=1)

    clean, disturbed = play(False), play(True)
    assert torch.equal(bits(clean), bits(disturbed))
    ref = TR.TunerRef(M, hop, words, h, decim)
    yd = np.zeros((S, M), np.complex128)
    yd[:, first:first + count] = rows.cpu().numpy().astype(np.complex128)
    outs, off = [], 0
    for i, n in enumerate(cuts):
        for j, f in retunes.get(i, ()):
            ref.set_freq(j, f)
        outs.append(ref.process(yd[off:off + n]))
        off += n
    want = np.concatenate(outs, axis=1)
    e = TR.err(clean.cpu().numpy(), want)
    print(f"retune: outputs {clean.shape[1]} err {e:.2e}")
    assert clean.shape == want.shape and e <= TR.TOL_TUNER


def test_tone_between_two_centres(pkg, O, dev):
    """A 24-bit tone 0.11 channel spacings above a word midway between two centres (r = -2^(31-b)) comes out of that
    receiver as the closed form of the CPU test, within the tone's quantisation plus TOL_CHAIN of the value; a receiver
    two spacings away reads at least 53.7 dB less than the tone (tuner_prototype's stop-band level for 4 taps per branch,
    tests/test_tuner_cpu.py::test_design_helpers)."""
    import torch
    M, P, T, decim, A = 1024, 4, 64, 4, 0.5
    hop = M // 2
    word = (300 << 22) - (1 << 21)
    delta = 0.11 / M
    w, h = pkg.tuner_prototype(M, P), pkg.tuner_lowpass(T, decim)
    n = np.arange(1 << 18, dtype=np.int64)
    xt = A * np.exp(2j * np.pi * (((word * n) & TR.MASK).astype(np.float64) / 2.0 ** 32 + delta * n))
    i = np.clip(np.rint(xt.real * 8388607.0), -8388608, 8388607).astype(np.int64)
    q = np.clip(np.rint(xt.imag * 8388607.0), -8388608, 8388607).astype(np.int64)
    d = torch.from_numpy(O.pack24(i, q).reshape(-1)).to(dev)
    ch = pkg.Channelizer(M, w, hop)
    t = pkg.Tuner(ch, [word, word + (2 << 22)], h, decim)
    out = t.process(ch.process(d)).cpu().numpy().astype(np.complex128)
    t.close()
    ch.close()
    r = TR.channel_of(M, word)[1]
    assert r == -(1 << 21)
    W = np.sum(w * np.exp(2j * np.pi * (delta + r / 2.0 ** 32) * np.arange(w.size)))
    H = np.sum(h * np.exp(-2j * np.pi * delta * hop * np.arange(T)))
    m = np.arange(out.shape[1])
    want = A * W * H * np.exp(2j * np.pi * delta * hop * (m * decim + T - 1))
    bound = 2.0 ** -23 * np.sum(np.abs(w)) * np.sum(np.abs(h)) * 2 + TR.TOL_CHAIN * abs(A * W * H)
    dev_ = float(np.max(np.abs(out[0] - want)))
    far = float(np.max(np.abs(out[1])))
    print(f"tone: |out| {abs(want[0]):.4f} deviation {dev_:.2e} (bound {bound:.2e}); two spacings away {20 * np.log10(far / A):.1f} dB")
    assert out.shape[1] > 100 and dev_ <= bound
    assert far <= A * 10 ** (-53.7 / 20)


@pytest.mark.perf
@pytest.mark.parametrize("lg", [24, 28])
def test_tuner_time_against_the_torch_path(pkg, dev, perf_record, lg):
    """Tuner.process against the path a host has today on the same device and the same tensor -- rows[:, idx] times a
    phasor table (built outside the timed region, in the torch path's favour), then a strided conv1d with h -- for
    K = 256 and 1024, M = 4096, hop 2048, T = 64, R = 4, the rows of 2^24 and 2^28 samples, median of 15 by events after
    a settle second.  The tuner must be faster at each point.  Recorded beside it, without an assertion:
    Channelizer.process for the same batch."""
    import torch
    M, hop, T, decim, ns = 4096, 2048, 64, 4, 1 << lg
    d = synth(pkg, dev, ns)
    w, hn = pkg.tuner_prototype(M, 4), pkg.tuner_lowpass(T, decim)
    ch = pkg.Channelizer(M, w, hop)
    S = ch.next_rows(ns)
    buf = torch.empty((S + 16, M), dtype=torch.complex64, device=dev)
    rows = ch.process(d, out=buf)
    assert rows.shape == (S, M)

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

    t_chan = None
    for K in (256, 1024):
        words = TR.receiver_set(M, K)
        kr = [TR.channel_of(M, f) for f in words]
        idx = torch.tensor([k for k, _ in kr], device=dev)
        th = TR.phase_words([r for _, r in kr], [0] * K, hop, np.arange(S))
        ph = torch.from_numpy(np.exp(-2j * np.pi * th.astype(np.float64) / 2.0 ** 32).astype(np.complex64)).to(dev)
        wt = torch.from_numpy(hn[::-1].copy()).to(dev).view(1, 1, T).repeat(2, 1, 1)
        tun = pkg.Tuner(ch, words, hn, decim)
        nout = TR.noutputs_of(S, T, decim)
        out = torch.empty((K, nout + T), dtype=torch.complex64, device=dev)

        def torch_path():
            z = rows[:, idx] * ph
            zr = torch.view_as_real(z).permute(1, 2, 0)                  # [K, 2, S]
            return torch.nn.functional.conv1d(zr, wt, stride=decim, groups=2)

        def new():
            tun.process(rows, out=out)

        ref = torch_path()
        tun.reset()
        got = tun.process(rows, out=out)
        torch.cuda.synchronize()
        assert got.shape == (K, nout) and tuple(ref.shape) == (K, 2, nout)
        scale = float(ref.abs().max())
        assert float((torch.view_as_real(got).permute(0, 2, 1) - ref).abs().max()) <= 1e-4 * scale
        del ref
        time.sleep(1.0)                      # freshly allocated buffers are slow at first
        t_torch = timed(torch_path)
        t_new = timed(new)
        if t_chan is None:
            t_chan = timed(lambda: ch.process(d, out=buf))
        tun.close()
        del ph, out
        torch.cuda.empty_cache()
        perf_record(f"tuner_2p{lg}_k{K}_ms", round(t_new, 4), unit="ms", torch_path_ms=round(t_torch, 4),
                    ratio=round(t_torch / t_new, 2), channelizer_ms=round(t_chan, 4), rows=S)
        assert t_new < t_torch, (lg, K, t_new, t_torch)
    ch.close()
