"""Audio (pddc_audio_*, k_audio) on the GPU against the numpy reference in double (tests/audio_ref.py).  Tolerance:
audio_ref.TOL_AUDIO, 7 x the float32 model's worst case on these very inputs (tests/test_audio_cpu.py), never taken from
k_audio."""
import numpy as np
import pytest

import audio_ref as AR
import demod_ref as DR
import tuner_ref as TR

pytestmark = pytest.mark.gpu


def run(pkg, x, L, M, P, T, g, cuts=None, i16=False, before=None, scale=32767.0):
    """all of x (torch float32 [nrx, n], any row stride) through a fresh Audio in the given batches -> float32
    [nrx, count] (and int16 if i16); every batch's count is checked against audio_outputs; before(i, a) is called ahead
    of batch i"""
    import torch
    a = pkg.Audio(x.shape[0], L, M, P, T, g, scale=scale)
    outs, pcm, off = [], [], 0
    for i, b in enumerate(cuts or [x.shape[1]]):
        if before:
            before(i, a)
        want = pkg.audio_outputs(L, M, off, b)
        assert a.next_outputs(b) == want == AR.outputs(L, M, off, b)
        o = a.process(x[:, off:off + b], i16=i16)
        if i16:
            o, p = o
            assert p.shape == (x.shape[0], want) and p.dtype == torch.int16
            pcm.append(p)
        assert o.shape == (x.shape[0], want) and o.dtype == torch.float32
        outs.append(o)
        off += b
    assert off == x.shape[1]
    torch.cuda.synchronize()
    a.close()
    return (torch.cat(outs, dim=1), torch.cat(pcm, dim=1)) if i16 else torch.cat(outs, dim=1)


def bits(t):
    import torch
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("nrx", [1, 5, 9, 1024])
def test_parity(pkg, dev, nrx):
    """Every ratio (3072/625, 128/625, 1/1, 3/1, 1/3, 16/1 and 1/16, the M = 16 L limit) with every (P, T) of (32, 1),
    (128, 32), (128, 64), (1024, 8): 700 inputs per receiver (nrx = 1024: 300), uniform in [-1, 1], one batch;
    |out - audio_ref| <= TOL_AUDIO, the count is audio_outputs'."""
    import torch
    x = AR.parity_inputs(nrx)
    xd = torch.from_numpy(x).to(dev)
    worst = 0.0
    for L, M in AR.RATIOS:
        for P, T in AR.SHAPES:
            g = AR.parity_prototype(L, M, P, T)
            out = run(pkg, xd, L, M, P, T, g).cpu().numpy()
            ref = AR.audio_ref(x, L, M, P, T, g)
            assert out.shape == ref.shape == (nrx, pkg.audio_outputs(L, M, 0, x.shape[1]))
            e = float(np.max(np.abs(out.astype(np.float64) - ref)))
            worst = max(worst, e)
            print(f"nrx {nrx} {L}/{M} P {P} T {T}: {out.shape[1]} outputs, err {e:.2e} (bar {AR.TOL_AUDIO:.2e})")
            assert e <= AR.TOL_AUDIO, (nrx, L, M, P, T, e)
    print(f"nrx {nrx}: worst {worst:.2e}")


CUTS = [0, 1, 2, 30, 0, 31, 255, 256, 125]


def test_bits_against_the_cut_and_the_company(pkg, dev):
    """700 values per receiver, T = 64.  One batch against the cuts 0, 1, 2, 30, 0, 31, 255, 256, 125 -- several batches
    shorter than T - 1 = 63, so the carried record spans three of them -- for 3072/625, 3/1 and 1/16, where batches of
    1 .. 15 inputs give no output: equal int32 views.  Receiver j's bits are the same alone, as index 0 or 6 of seven
    receivers, and with input rows n or n + 13 apart."""
    import torch
    assert sum(CUTS) == 700
    x = torch.from_numpy(AR.parity_inputs(9)).to(dev)
    for L, M in ((3072, 625), (3, 1), (1, 16)):
        P, T = 128, 64
        g = AR.parity_prototype(L, M, P, T)
        one = run(pkg, x, L, M, P, T, g)
        assert torch.isfinite(one).all() and one.shape[1] == -(-700 * L // M)
        cut = run(pkg, x, L, M, P, T, g, CUTS)
        assert torch.equal(bits(cut), bits(one)), (L, M)
        if (L, M) == (1, 16):
            assert [pkg.audio_outputs(L, M, sum(CUTS[:i]), b) for i, b in enumerate(CUTS)][:5] == [0, 1, 0, 2, 0]
            fine = [1] * 40 + [660]                                   # 37 of the 40 one-input batches give nothing
            assert torch.equal(bits(run(pkg, x, L, M, P, T, g, fine)), bits(one))
        for j in (2, 8):
            alone = run(pkg, x[j:j + 1], L, M, P, T, g, CUTS)
            assert torch.equal(bits(alone[0]), bits(one[j])), (L, M, j)
            others = [k for k in range(9) if k != j][:6]
            for at in (0, 6):
                rows = others[:at] + [j] + others[at:]
                seven = run(pkg, x[rows].contiguous(), L, M, P, T, g, CUTS)
                assert torch.equal(bits(seven[at]), bits(one[j])), (L, M, j, at)
        wide = torch.zeros((9, 713), dtype=torch.float32, device=dev)
        wide[:, :700] = x
        view = wide[:, :700]
        assert view.stride(0) == 713
        assert torch.equal(bits(run(pkg, view, L, M, P, T, g, CUTS)), bits(one))


@pytest.mark.parametrize("count", [255, 256, 257, 513])
def test_tile_seams(pkg, dev, count):
    """One batch whose output count is 255, 256, 257 and 513 (tiles of 256 outputs), for every one of three ratios that
    reaches the count exactly (1/3 reaches all of them): against the reference, and the bits of the same series cut in
    two."""
    import torch
    hit = 0
    for L, M, P, T in ((3072, 625, 128, 32), (1, 3, 32, 1), (16, 1, 1024, 8)):
        n = next(n for n in range(1, 2000) if AR.outputs(L, M, 0, n) >= count)
        if AR.outputs(L, M, 0, n) != count:
            continue                                                   # this ratio steps over the count
        x = AR.parity_inputs(5)[:, :n] if n <= 700 else np.random.default_rng(n).uniform(-1, 1, (5, n)).astype(np.float32)
        g = AR.parity_prototype(L, M, P, T)
        xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        one = run(pkg, xd, L, M, P, T, g)
        assert one.shape == (5, count)
        e = float(np.max(np.abs(one.cpu().numpy().astype(np.float64) - AR.audio_ref(x, L, M, P, T, g))))
        print(f"{count} outputs at {L}/{M}: {n} inputs, err {e:.2e}")
        assert e <= AR.TOL_AUDIO
        assert torch.equal(bits(run(pkg, xd, L, M, P, T, g, [n // 3, n - n // 3])), bits(one))
        hit += 1
    assert hit >= 1


def identity(P=32):
    g = np.zeros(P, np.float32)
    g[0] = 1.0
    return g


def test_pcm(pkg, dev):
    """L = M = 1 with g = [1, 0, ...] hands the input through bit for bit.  Then the inputs (h + 0.5) / scale for
    h = -5 .. 5, +-1.5, +-inf and NaN give exactly pcm_ref: ties to even, -32768 / 32767, 0.  For a resampling case the
    int16 output is pcm_ref of the device's own float32 output, and the float32 bits do not depend on whether int16 is
    asked for; int16 alone gives the same PCM."""
    import torch
    s = 32767.0
    x = AR.parity_inputs(5).copy()
    special = np.array([(h + 0.5) / s for h in range(-5, 6)] + [1.5, -1.5, np.inf, -np.inf, np.nan], np.float32)
    x[3, 100:100 + special.size] = special
    xd = torch.from_numpy(x).to(dev)
    y, p = run(pkg, xd, 1, 1, 32, 1, identity(), i16=True, scale=s)
    assert torch.equal(bits(y), bits(xd))
    want = AR.pcm_ref(x, s)
    got = p.cpu().numpy()
    assert list(got[3, 100:100 + special.size]) == list(want[3, 100:100 + special.size])
    assert list(want[3, 111:116]) == [32767, -32768, 32767, -32768, 0]
    assert np.array_equal(got, want)
    for scale in (s, 1000.0):
        L, M, P, T = 3072, 625, 128, 32
        g = AR.parity_prototype(L, M, P, T)
        xs = torch.from_numpy(AR.parity_inputs(5) * np.float32(1.3)).to(dev)         # some outputs past full scale
        y, p = run(pkg, xs, L, M, P, T, g, CUTS, i16=True, scale=scale)
        want = AR.pcm_ref(y.cpu().numpy(), scale)
        assert np.array_equal(p.cpu().numpy(), want)
        if scale == s:
            assert want.max() == 32767 and want.min() == -32768
        assert torch.equal(bits(run(pkg, xs, L, M, P, T, g, CUTS, scale=scale)), bits(y))
        a = pkg.Audio(5, L, M, P, T, g, scale=scale)
        only = a.process(xs, f32=False, i16=True)
        torch.cuda.synchronize()
        assert only.dtype == torch.int16 and torch.equal(only, p)
        a.close()


def test_a_refused_process_changes_nothing_and_reset(pkg, dev):
    """process calls refused for capacity (either output too small, an x stride below n) and for a misaligned or missing
    pointer, between the batches: the object stays usable and the next correct call's bits are those of a twin that
    never saw them.  After reset the outputs repeat those after create."""
    import ctypes as C
    import torch
    L_, M_, P, T = 3072, 625, 128, 64
    g = AR.parity_prototype(L_, M_, P, T)
    nrx, n = 9, 700
    cuts = [300, 150, 250]
    x = torch.from_numpy(AR.parity_inputs(9)).to(dev)
    clean, clean_p = run(pkg, x, L_, M_, P, T, g, cuts, i16=True)
    lib = pkg.ddc_lib()

    def disturb(i, a):
        b = cuts[i]
        c = a.next_outputs(b)
        assert c > 1
        for kw in (dict(out_f32=torch.empty((nrx, c - 1), dtype=torch.float32, device=dev)),
                   dict(out_i16=torch.empty((nrx, c - 1), dtype=torch.int16, device=dev))):
            with pytest.raises(pkg.PddcError) as e:
                a.process(x[:, :b], **kw)
            assert e.value.code == pkg.PDDC_ECAPACITY
        with pytest.raises(pkg.PddcError) as e:
            a.process(x[:, :b], f32=False, i16=False)
        f = torch.empty((nrx, c), dtype=torch.float32, device=dev)
        p = torch.empty((nrx, c + 1), dtype=torch.int16, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        k = C.c_size_t(12345)
        call = lambda *args: lib.pddc_audio_process(a._h, *args, C.byref(k), st)
        assert call(x.data_ptr(), b, b - 1, f.data_ptr(), c, None, 0) == pkg.PDDC_ECAPACITY
        assert call(x.data_ptr(), b, n, f.data_ptr(), c - 1, p.data_ptr(), c + 1) == pkg.PDDC_ECAPACITY
        assert call(x.data_ptr(), b, n, f.data_ptr(), c, p.data_ptr(), c - 1) == pkg.PDDC_ECAPACITY
        assert call(x.data_ptr() + 2, b, n, f.data_ptr(), c, None, 0) == pkg.PDDC_EINVAL
        assert call(x.data_ptr(), b, n, f.data_ptr() + 2, c, None, 0) == pkg.PDDC_EINVAL
        assert call(x.data_ptr(), b, n, None, 0, p.data_ptr() + 1, c + 1) == pkg.PDDC_EINVAL
        assert call(None, b, n, f.data_ptr(), c, None, 0) == pkg.PDDC_EINVAL
        assert call(x.data_ptr(), b, n, None, 0, None, 0) == pkg.PDDC_EINVAL
        assert k.value == 12345 and a.next_outputs(b) == c
        assert call(None, 0, 0, None, 0, None, 0) == pkg.PDDC_OK and k.value == 0

    got, got_p = run(pkg, x, L_, M_, P, T, g, cuts, i16=True, before=disturb)
    assert torch.equal(bits(got), bits(clean)) and torch.equal(got_p, clean_p)
    a = pkg.Audio(nrx, L_, M_, P, T, g)
    first = [a.process(x[:, :300]), a.process(x[:, 300:])]
    a.reset()
    assert a.next_outputs(700) == pkg.audio_outputs(L_, M_, 0, 700)
    again = a.process(x)
    torch.cuda.synchronize()
    assert torch.equal(bits(torch.cat(first, dim=1)), bits(again)) and torch.equal(bits(again), bits(clean))
    a.close()


def test_chain(pkg, dev):
    """2^17 LCG samples through Channelizer (M = 1024, hop 512) -> Tuner (T = 64, R = 4, 4 receivers) -> Demod (AM and
    SSB) -> Audio at 128/125, fed Demod's view directly, on one stream: the run cut at three places is bit-identical to
    the uncut run, and the audio is within TOL_AUDIO of audio_ref applied to the device's own Demod output."""
    import torch
    M, hop, T, Rd, ns = 1024, 512, 64, 4, 1 << 17
    L_, M_, P, Ta = 128, 125, 128, 32
    g = pkg.audio_prototype(P, Ta, 0.45)
    words = TR.receiver_set(M, 4)
    rx = [(DR.AM, 0, 0), (DR.SSB, 0x01234567, 0), (DR.AM, 0, DR.DC), (DR.SSB, 0x0FEDCBA9, DR.DC | DR.AGC)]
    packed = pkg.synth_lcg(6 * ns, 12345, 0, dev)
    w, h = pkg.tuner_prototype(M, 4), pkg.tuner_lowpass(T, Rd)

    def chain(cuts):
        ch = pkg.Channelizer(M, w, hop)
        tu = pkg.Tuner(ch, words, h, Rd)
        de = pkg.Demod(rx, **{k: DR.PARAMS[k] for k in ("rho", "lam", "target", "gmax")})
        au = pkg.Audio(4, L_, M_, P, Ta, g)
        outs, pcm, dem, off = [], [], [], 0
        for b in cuts:
            d = de.process(tu.process(ch.process(packed[6 * off:6 * (off + b)])))
            y, p = au.process(d, i16=True)
            dem.append(d.clone())
            outs.append(y)
            pcm.append(p)
            off += b
        assert off == ns
        torch.cuda.synchronize()
        for o in (au, de, tu, ch):
            o.close()
        return torch.cat(outs, dim=1), torch.cat(pcm, dim=1), torch.cat(dem, dim=1)

    y, p, d = chain([ns])
    assert d.shape[1] >= 40 and y.shape[1] == pkg.audio_outputs(L_, M_, 0, d.shape[1])
    yc, pc, dc = chain([40000, 8, 50000, ns - 90008])
    assert torch.equal(bits(dc), bits(d))
    assert torch.equal(bits(yc), bits(y)) and torch.equal(pc, p)
    dn = d.cpu().numpy()
    ref = AR.audio_ref(dn, L_, M_, P, Ta, g)
    e = float(np.max(np.abs(y.cpu().numpy().astype(np.float64) - ref)))
    scale = float(np.max(np.abs(dn)))
    print(f"chain: {y.shape[1]} audio outputs from {d.shape[1]} demod outputs, max |demod| {scale:.3f}, err {e:.2e}")
    assert scale <= 1.0 and e <= AR.TOL_AUDIO
    assert np.array_equal(p.cpu().numpy(), AR.pcm_ref(y.cpu().numpy()))
